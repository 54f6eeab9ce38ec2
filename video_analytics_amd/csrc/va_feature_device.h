// Device helpers the classical feature chains share (svm.hip, ksvm.hip, fisher.hip, codebook.hip, dtraj.hip, stip.hip): one copy of every
// sum whose written order reaches a result, of the scans, and of the orientation votes.
#pragma once
#include "va_internal.h"

// ---- float64 sums and the float64 MFMA

// The operands of v_mfma_f64_16x16x4_f64: one f64 of A and of B per lane, A[row lane&15][k lane>>4], B[k lane>>4][col lane&15];
// four results per lane in a v4d: col lane&15, row (lane>>4) + 4 reg.
typedef double v4d __attribute__((ext_vector_type(4)));

// The sum of v over the 256 threads of a workgroup, the same bits in every thread: an xor butterfly over the lanes of each
// wave (offsets 32, 16, ..., 1), then the four waves as ((w0 + w1) + w2) + w3.  red: 4 doubles of LDS.
__device__ __forceinline__ double va_wg_sum256(double v, double* red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// p[at] + p[stride + at] + ... + p[(n - 1) stride + at], added in that order
__device__ __forceinline__ double va_strided_sum(const double* __restrict__ p, int n, size_t stride, size_t at)
{
    double acc = p[at];
    for (int i = 1; i < n; ++i) acc = acc + p[(size_t)i * stride + at];
    return acc;
}

// True when any of the (at most 64) class rows j0 .. j0+63 has its flag set; the same answer in every lane and wave (svm.hip
// and ksvm.hip skip the tiles of finished rows with it).
__device__ __forceinline__ bool va_tile_is_live(const int* __restrict__ flags, int j0, int c, int lane)
{
    const int j = j0 + lane;
    return __any(j < c ? flags[j] : 0) != 0;
}

// ---- integer scans (sums mod 2^32: the order is free)

// inclusive scan over the 64 lanes of a wave; lane = threadIdx.x & 63
template <typename T>
__device__ __forceinline__ T va_wave_scan_incl(T v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// exclusive scan of one int per thread over a workgroup of NT lanes, and their total: the waves scan, thread 0 scans the wave
// totals one after the other.  sh: NT / 64 + 1 ints of LDS, free again on return.
template <int NT>
__device__ __forceinline__ int va_wg_scan_excl(int v, int& total, int* sh)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = va_wave_scan_incl(v, lane);
    if (lane == 63) sh[wv] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < NT / 64; ++i) {
            const int t = sh[i];
            sh[i] = run;
            run += t;
        }
        sh[NT / 64] = run;
    }
    __syncthreads();
    const int r = sh[wv] + x - v;
    total = sh[NT / 64];
    __syncthreads();
    return r;
}

// ---- orientation votes (dtraj.hip with 8 bins, stip.hip with va_stip_params.bins): DESIGN.md S70-S71

// S70: p(s) ~ atan(s) 4 / pi on [0,1], odd, Horner in s^2
constexpr float kAtanC0 = 1.2732345f, kAtanC1 = -0.4242086f, kAtanC2 = 0.25219768f, kAtanC3 = -0.16850284f, kAtanC4 = 0.10143076f,
                kAtanC5 = -0.042850755f, kAtanC6 = 0.0086996285f;

// S70: magnitude and bin coordinate in [0,8] of the vector (x, y)
__device__ __forceinline__ void va_orient(float x, float y, float& m, float& a)
{
    m = sqrtf(x * x + y * y);
    const float ax = fabsf(x), ay = fabsf(y);
    const float lo = fminf(ax, ay), hi = fmaxf(ax, ay);
    const float s = lo / (hi > 0.0f ? hi : 1.0f);
    const float s2 = s * s;
    float p = kAtanC6;
    p = p * s2 + kAtanC5;
    p = p * s2 + kAtanC4;
    p = p * s2 + kAtanC3;
    p = p * s2 + kAtanC2;
    p = p * s2 + kAtanC1;
    p = p * s2 + kAtanC0;
    p = p * s;
    if (ay > ax) p = 2.0f - p;
    if (x < 0.0f) p = 4.0f - p;
    if (y < 0.0f) p = 8.0f - p;
    a = p;
}

// S70-S71: the two quantised votes of one group of `bins` circular bins (S70's coordinate times bins / 8, which is exact for
// the powers of two and changes nothing at 8); a magnitude that is not finite votes nothing
__device__ __forceinline__ void va_votes_of(float x, float y, float vmax, float scale, int bins, int& b0, unsigned& q0, unsigned& q1,
                                            float& m)
{
    float a;
    va_orient(x, y, m, a);
    b0 = 0, q0 = 0u, q1 = 0u;
    if (!(fabsf(m) <= 3.4028234663852886e38f)) return;
    if (bins != 8) a = a * ((float)bins * 0.125f);
    const float fl = floorf(a), f = a - fl;
    b0 = (int)fl % bins;
    q0 = (unsigned)rintf(fminf(m * (1.0f - f), vmax) * scale);
    q1 = (unsigned)rintf(fminf(m * f, vmax) * scale);
}

// one pixel's group of `bins` planes, fl words apart: q0 in bin b0, q1 in the next one around the circle, 0 elsewhere
__device__ __forceinline__ void va_store_bins(unsigned* o, size_t fl, int bins, int b0, unsigned q0, unsigned q1)
{
    const int b1 = b0 + 1 == bins ? 0 : b0 + 1;
    for (int b = 0; b < bins; ++b) o[b * fl] = b == b0 ? q0 : (b == b1 ? q1 : 0u);
}
