// Brox optical flow for gfx950 (MI355X): hand-written HIP, no CPU fallback.
//
// The flow method of the two-stream paper (Sheet03/notes.txt:11-16): Brox, Bruhn, Papenberg, Weickert, ECCV 2004, in the
// form of IPOL's "Robust Optical Flow Estimation".  DESIGN.md S57-S62 fix every expression and its operation order; this
// file must be compiled with -ffp-contract=off and writes no fmaf in any stage of its own, so that results are independent
// of the tiling and comparable bit for bit with an independent float32 implementation.
//
// Frames (S0), pyramid (S1) and derivatives (S2) are the flow methods' shared front end (va_stage_*, flow_common.hip);
// upsampling (S8) and the output copy are TV-L1's kernels (va_stage_*, tvl1.hip).  The layout is the shared one: rows
// `pitch` = width rounded up to 4 floats, planes rounded up to 64 floats.
//   pyramid  3 x [level][frame][3][plane]: (I, Ix, Iy), (Ix, Ixx, -) and (Iy, Ixy, Iyy): S2 applied to I, Ix and Iy
//   state    [pair][6][plane]: u, v and two of the three (du, dv) buffers; the third is [pair][2][plane]
//   ro       [pair][8][plane]: I1wx, I1wy, I1wxx, I1wxy, I1wyy, Iz, Ixz, Iyz of the current warp
//
// The hot path is k_brox_inner: one lagged-nonlinearity step (S60) and K of its red-black SOR sweeps (S61) per launch.
// A workgroup owns a region of the field: du, dv in LDS (8 B per pixel, a frame of one pixel around it), the nine
// coefficients of each of its pixels in registers.  A lane owns pairs of horizontally adjacent pixels, one of each colour,
// so that every lane works in both half-sweeps.  A field that fits one workgroup is one region without a halo and the
// launch runs all solver_iters sweeps in place; a larger field is cut into tiles whose regions overlap by 2K + 2 pixels
// (a sweep carries information 2 pixels, the coefficient stencil reaches 2 more), and the launches of a step ping-pong
// between two buffers while the step's entry (du, dv) stays where the coefficients are read from.
#include "va_internal.h"
#include <cmath>
#include <cstring>

namespace {

constexpr int kRoPlanes = 8;
constexpr int kMaxPairs = 3072;  // pixel pairs of the largest region: 1024 lanes x 3 pairs (a fourth pair spills: 128 registers)
constexpr int kMaxK = 17;  // halo 36: a tile of 6 x 6 is left
constexpr int kDefaultK = 5;
constexpr int kMaxSide = 78;  // the largest square region: 39 x 78 pairs

enum { F_IX = 0, F_IY, F_IXX, F_IXY, F_IYY, F_IZ, F_IXZ, F_IYZ, F_U, F_V, F_COUNT };

struct InnerArgs {
    const float* fld[F_COUNT];  // per field: pointer to field 0, fs[] floats between two fields
    size_t fs[F_COUNT];
    const float* d0[2];   // du, dv at the head of the inner step: the coefficients are computed from them
    const float* din[2];  // du, dv before this launch's sweeps
    float* dout[2];       // du, dv after them (the core of every tile)
    size_t d0s, dins, douts;
    int w, h, pitch;
    int TW, TH, ntx, H, K;
    float alpha, gamma, eps2, omega, om1;
};

// value -> cell i of a framed LDS array, and into the frame where the cell lies on the region's edge (a field border
// then reads its own pixel: the clamped index of S60; an inner region edge reads something finite that never reaches the core)
template <typename T>
__device__ __forceinline__ void put_framed(T* s, int i, int x, int y, int RW, int RH, int RWp, T v)
{
    s[i] = v;
    if (x == 0) s[i - 1] = v;
    if (x == RW - 1) s[i + 1] = v;
    if (y == 0) s[i - RWp] = v;
    if (y == RH - 1) s[i + RWp] = v;
}

// S60 + S61.  grid (tiles, fields), NT lanes, PPT pixel pairs per lane; dynamic LDS: 12 B per cell of the framed region.
template <int NT, int PPT>
__global__ void __launch_bounds__(NT) k_brox_inner(InnerArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int n = blockIdx.y;
    const int ty = blockIdx.x / a.ntx, tx = blockIdx.x - ty * a.ntx;
    const int cx0 = tx * a.TW, cy0 = ty * a.TH;
    const int cx1 = d_min(cx0 + a.TW, a.w), cy1 = d_min(cy0 + a.TH, a.h);
    const int rx0 = d_max(cx0 - a.H, 0), ry0 = d_max(cy0 - a.H, 0);
    const int rx1 = d_min(cx1 + a.H, a.w), ry1 = d_min(cy1 + a.H, a.h);
    const int RW = rx1 - rx0, RH = ry1 - ry0, RWp = RW + 2, PW = (RW + 1) >> 1;
    const int npairs = PW * RH;
    float2* sd = reinterpret_cast<float2*>(lds);  // [(RH + 2) * RWp]
    float* ps = lds + 2 * (RH + 2) * RWp;         // [(RH + 2) * RWp]

    // this lane's pairs: pixel e of pair k is the one with (x + y) % 2 == e (global coordinates); lx[k][e] < 0: no such pixel
    int lx[PPT][2], ly[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int q = threadIdx.x + k * NT;
        const bool ok = q < npairs;
        const int row = ok ? q / PW : 0, x0 = 2 * (q - row * PW);
        const int c0 = (rx0 + x0 + ry0 + row) & 1;  // colour of the pair's left pixel
        ly[k] = row;
        const int xa = ok ? x0 : -1, xb = ok && x0 + 1 < RW ? x0 + 1 : -1;
        lx[k][0] = c0 ? xb : xa;
        lx[k][1] = c0 ? xa : xb;
    }
#define BROX_FOR_PIXELS                      \
    _Pragma("unroll") for (int k = 0; k < PPT; ++k) _Pragma("unroll") for (int e = 0; e < 2; ++e) if (lx[k][e] >= 0)
#define BROX_PIXEL                                                                      \
    const int x = lx[k][e], y = ly[k], gx = rx0 + x, gy = ry0 + y;                      \
    const int i = (y + 1) * RWp + x + 1;                                                \
    const size_t g = (size_t)gy * a.pitch + gx;                                         \
    (void)gx; (void)gy; (void)i; (void)g

    // U = u + du, V = v + dv of the step's entry
    BROX_FOR_PIXELS
    {
        BROX_PIXEL;
        const float U = a.fld[F_U][n * a.fs[F_U] + g] + a.d0[0][n * a.d0s + g];
        const float V = a.fld[F_V][n * a.fs[F_V] + g] + a.d0[1][n * a.d0s + g];
        put_framed(sd, i, x, y, RW, RH, RWp, make_float2(U, V));
    }
    __syncthreads();
    // PsiS
    BROX_FOR_PIXELS
    {
        BROX_PIXEL;
        const float2 l = sd[i - 1], r = sd[i + 1], t = sd[i - RWp], b = sd[i + RWp];
        const float ux = 0.5f * (r.x - l.x), uy = 0.5f * (b.x - t.x);
        const float vx = 0.5f * (r.y - l.y), vy = 0.5f * (b.y - t.y);
        const float s = a.alpha / sqrtf(((ux * ux + uy * uy) + (vx * vx + vy * vy)) + a.eps2);
        put_framed(ps, i, x, y, RW, RH, RWp, s);
    }
    __syncthreads();
    // u, v for the constant part of the divergence
    BROX_FOR_PIXELS
    {
        BROX_PIXEL;
        put_framed(sd, i, x, y, RW, RH, RWp, make_float2(a.fld[F_U][n * a.fs[F_U] + g], a.fld[F_V][n * a.fs[F_V] + g]));
    }
    __syncthreads();
    // the coefficients of every pixel this lane owns
    float A12[PPT][2], D1[PPT][2], D2[PPT][2], b1[PPT][2], b2[PPT][2], wL[PPT][2], wR[PPT][2], wU[PPT][2], wD[PPT][2];
    BROX_FOR_PIXELS
    {
        BROX_PIXEL;
        const float pc = ps[i];
        const float l = gx > 0 ? 0.5f * (pc + ps[i - 1]) : 0.0f;
        const float r = gx < a.w - 1 ? 0.5f * (pc + ps[i + 1]) : 0.0f;
        const float t = gy > 0 ? 0.5f * (pc + ps[i - RWp]) : 0.0f;
        const float b = gy < a.h - 1 ? 0.5f * (pc + ps[i + RWp]) : 0.0f;
        const float sw = (l + r) + (t + b);
        const float2 c = sd[i], cl = sd[i - 1], cr = sd[i + 1], ct = sd[i - RWp], cb = sd[i + RWp];
        const float divu = (l * (cl.x - c.x) + r * (cr.x - c.x)) + (t * (ct.x - c.x) + b * (cb.x - c.x));
        const float divv = (l * (cl.y - c.y) + r * (cr.y - c.y)) + (t * (ct.y - c.y) + b * (cb.y - c.y));
        const float du = a.d0[0][n * a.d0s + g], dv = a.d0[1][n * a.d0s + g];
        const float Ix = a.fld[F_IX][n * a.fs[F_IX] + g], Iy = a.fld[F_IY][n * a.fs[F_IY] + g];
        const float Ixx = a.fld[F_IXX][n * a.fs[F_IXX] + g], Ixy = a.fld[F_IXY][n * a.fs[F_IXY] + g];
        const float Iyy = a.fld[F_IYY][n * a.fs[F_IYY] + g];
        const float Iz = a.fld[F_IZ][n * a.fs[F_IZ] + g], Ixz = a.fld[F_IXZ][n * a.fs[F_IXZ] + g];
        const float Iyz = a.fld[F_IYZ][n * a.fs[F_IYZ] + g];
        const float q = (Iz + Ix * du) + Iy * dv;
        const float pD = 1.0f / sqrtf(q * q + a.eps2);
        const float g1 = (Ixz + Ixx * du) + Ixy * dv, g2 = (Iyz + Ixy * du) + Iyy * dv;
        const float pG = a.gamma / sqrtf((g1 * g1 + g2 * g2) + a.eps2);
        const float A11 = pD * (Ix * Ix) + pG * (Ixx * Ixx + Ixy * Ixy);
        const float A22 = pD * (Iy * Iy) + pG * (Ixy * Ixy + Iyy * Iyy);
        A12[k][e] = pD * (Ix * Iy) + pG * (Ixx * Ixy + Ixy * Iyy);
        b1[k][e] = divu - (pD * (Ix * Iz) + pG * (Ixx * Ixz + Ixy * Iyz));
        b2[k][e] = divv - (pD * (Iy * Iz) + pG * (Ixy * Ixz + Iyy * Iyz));
        D1[k][e] = A11 + sw;
        D2[k][e] = A22 + sw;
        wL[k][e] = l, wR[k][e] = r, wU[k][e] = t, wD[k][e] = b;
    }
    __syncthreads();
    // du, dv as this launch finds them
    BROX_FOR_PIXELS
    {
        BROX_PIXEL;
        put_framed(sd, i, x, y, RW, RH, RWp, make_float2(a.din[0][n * a.dins + g], a.din[1][n * a.dins + g]));
    }
    __syncthreads();
    // K red-black sweeps: (x + y) even first
    for (int s = 0; s < a.K; ++s) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
#pragma unroll
            for (int k = 0; k < PPT; ++k)
                if (lx[k][e] >= 0) {
                    const int i = (ly[k] + 1) * RWp + lx[k][e] + 1;
                    const float2 c = sd[i], l = sd[i - 1], r = sd[i + 1], t = sd[i - RWp], b = sd[i + RWp];
                    const float su = (wL[k][e] * l.x + wR[k][e] * r.x) + (wU[k][e] * t.x + wD[k][e] * b.x);
                    const float du = a.om1 * c.x + a.omega * (((b1[k][e] + su) - A12[k][e] * c.y) / D1[k][e]);
                    const float sv = (wL[k][e] * l.y + wR[k][e] * r.y) + (wU[k][e] * t.y + wD[k][e] * b.y);
                    const float dv = a.om1 * c.y + a.omega * (((b2[k][e] + sv) - A12[k][e] * du) / D2[k][e]);
                    sd[i] = make_float2(du, dv);
                }
            __syncthreads();
        }
    }
    BROX_FOR_PIXELS
    {
        BROX_PIXEL;
        if (gx >= cx0 && gx < cx1 && gy >= cy0 && gy < cy1) {
            const float2 c = sd[i];
            a.dout[0][n * a.douts + g] = c.x;
            a.dout[1][n * a.douts + g] = c.y;
        }
    }
#undef BROX_FOR_PIXELS
#undef BROX_PIXEL
}

// S58, S59: the second frame's derivatives at (x + u, y + v), the three differences, and du = dv = 0 (pitch padding included).
// One lane per run of four pixels of a row: 16-byte loads of u, v and the first frame, 16-byte stores of the ten outputs.
__global__ void __launch_bounds__(256) k_brox_warp(const float* __restrict__ pa, const float* __restrict__ pb, const float* __restrict__ pc,
                                                   size_t plane, int w, int h, int pitch, int fps, const float* __restrict__ state,
                                                   float* __restrict__ ro, float* __restrict__ du, float* __restrict__ dv, size_t ds)
{
    const int pair = blockIdx.y, p4 = pitch >> 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= p4 * h) return;
    const int y = idx / p4, x0 = 4 * (idx - y * p4);
    const int seq = pair / (fps - 1), f0 = seq * fps + (pair - seq * (fps - 1));
    const size_t o = (size_t)y * pitch + x0;
    const float* A0 = pa + (size_t)f0 * 3 * plane;
    const float* A1 = pa + (size_t)(f0 + 1) * 3 * plane;
    const float* B1 = pb + (size_t)(f0 + 1) * 3 * plane;
    const float* C1 = pc + (size_t)(f0 + 1) * 3 * plane;
    const float* st = state + (size_t)pair * 6 * plane;
    const float4 u4 = *reinterpret_cast<const float4*>(st + o), v4 = *reinterpret_cast<const float4*>(st + plane + o);
    const float4 i0 = *reinterpret_cast<const float4*>(A0 + o), i0x = *reinterpret_cast<const float4*>(A0 + plane + o);
    const float4 i0y = *reinterpret_cast<const float4*>(A0 + 2 * plane + o);
    const float uu[4] = {u4.x, u4.y, u4.z, u4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
    const float z0[4] = {i0.x, i0.y, i0.z, i0.w}, zx[4] = {i0x.x, i0x.y, i0x.z, i0x.w}, zy[4] = {i0y.x, i0y.y, i0y.z, i0y.w};
    float out[kRoPlanes][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = x0 + j < w;  // (a padding lane samples at a clamped position, whatever its u, v hold, and stores 0)
        const float px = (float)(x0 + j) + uu[j], py = (float)y + vv[j];
        const float Iw = va_bilinear_plain(A1, w, h, pitch, px, py);
        const float Iwx = va_bilinear_plain(A1 + plane, w, h, pitch, px, py);
        const float Iwy = va_bilinear_plain(A1 + 2 * plane, w, h, pitch, px, py);
        out[F_IX][j] = in ? Iwx : 0.0f;
        out[F_IY][j] = in ? Iwy : 0.0f;
        out[F_IXX][j] = in ? va_bilinear_plain(B1 + plane, w, h, pitch, px, py) : 0.0f;
        out[F_IXY][j] = in ? va_bilinear_plain(C1 + plane, w, h, pitch, px, py) : 0.0f;
        out[F_IYY][j] = in ? va_bilinear_plain(C1 + 2 * plane, w, h, pitch, px, py) : 0.0f;
        out[F_IZ][j] = in ? Iw - z0[j] : 0.0f;
        out[F_IXZ][j] = in ? Iwx - zx[j] : 0.0f;
        out[F_IYZ][j] = in ? Iwy - zy[j] : 0.0f;
    }
    float* r = ro + (size_t)pair * kRoPlanes * plane + o;
#pragma unroll
    for (int f = 0; f < kRoPlanes; ++f) *reinterpret_cast<float4*>(r + f * plane) = make_float4(out[f][0], out[f][1], out[f][2], out[f][3]);
    *reinterpret_cast<float4*>(du + (size_t)pair * ds + o) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    *reinterpret_cast<float4*>(dv + (size_t)pair * ds + o) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// S61's last line: u += du, v += dv, four pixels per lane (rows and planes are multiples of four floats)
__global__ void k_brox_update(float* __restrict__ state, size_t plane, int n4, const float* __restrict__ du, const float* __restrict__ dv,
                              size_t ds)
{
    const int pair = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n4) return;
    float4* u = reinterpret_cast<float4*>(state + (size_t)pair * 6 * plane) + idx;
    float4* v = reinterpret_cast<float4*>(state + (size_t)pair * 6 * plane + plane) + idx;
    const float4 a = *u, b = *v;
    const float4 x = reinterpret_cast<const float4*>(du + (size_t)pair * ds)[idx], y = reinterpret_cast<const float4*>(dv + (size_t)pair * ds)[idx];
    *u = make_float4(a.x + x.x, a.y + x.y, a.z + x.z, a.w + x.w);
    *v = make_float4(b.x + y.x, b.y + y.y, b.z + y.z, b.w + y.w);
}

// ---------------------------------------------------------------- host side ------------------

int region_pairs(int rw, int rh) { return ((rw + 1) / 2) * rh; }

// The shape one level's inner steps run in.  whole: one region, all sweeps in one launch, in place.
struct Shape {
    bool whole;
    int TW, TH, ntx, nty, H, K;
    int max_pairs;  // of the largest region
    size_t lds;
};

int pick_shape(const va_brox_params* p, int w, int h, Shape* s)
{
    const int* t = p->tuning;
    if (t[VA_BROX_TUNE_WHOLE] == -1 && region_pairs(w, h) <= kMaxPairs) {
        s->whole = true;
        s->TW = w, s->TH = h, s->ntx = s->nty = 1, s->H = 0, s->K = p->solver_iters;
        s->max_pairs = region_pairs(w, h);
        s->lds = (size_t)(w + 2) * (h + 2) * 12;
        return VA_OK;
    }
    s->whole = false;
    int K = t[VA_BROX_TUNE_K] > 0 ? t[VA_BROX_TUNE_K] : kDefaultK;
    if (K > p->solver_iters) K = p->solver_iters;
    s->K = K;
    s->H = 2 * K + 2;
    const int T = (kMaxSide - 2 * s->H) & ~1;  // the largest square tile
    // (the library's own tiles: as many as tiles of T need, of equal size -- 224 is five tiles of 45, not four of 54 and one of 8)
    s->TW = t[VA_BROX_TUNE_TILE_W] > 0 ? t[VA_BROX_TUNE_TILE_W] : va_cdiv(w, va_cdiv(w, T));
    s->TH = t[VA_BROX_TUNE_TILE_H] > 0 ? t[VA_BROX_TUNE_TILE_H] : va_cdiv(h, va_cdiv(h, T));
    if (s->TW > w) s->TW = w;
    if (s->TH > h) s->TH = h;
    s->ntx = va_cdiv(w, s->TW);
    s->nty = va_cdiv(h, s->TH);
    const int rw = s->TW + 2 * s->H < w ? s->TW + 2 * s->H : w, rh = s->TH + 2 * s->H < h ? s->TH + 2 * s->H : h;
    s->max_pairs = region_pairs(rw, rh);
    s->lds = (size_t)(rw + 2) * (rh + 2) * 12;
    VA_CHECK_ARG(s->max_pairs <= kMaxPairs,
                 "va_brox: tuning: a %d x %d tile with %d sweeps per launch has a region of %d x %d pixels, more than one workgroup holds "
                 "(%d pixel pairs)", s->TW, s->TH, K, rw, rh, kMaxPairs);
    return VA_OK;
}

template <int NT, int PPT>
int launch_inner_as(const InnerArgs& a, dim3 grid, size_t lds, hipStream_t st)
{
    if (int rc = va_allow_lds(&k_brox_inner<NT, PPT>, lds)) return rc;
    k_brox_inner<NT, PPT><<<grid, NT, lds, st>>>(a);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

int launch_inner(const Shape& s, const InnerArgs& a, int n, hipStream_t st)
{
    const dim3 grid(s.ntx * s.nty, n);
    if (s.max_pairs <= 256) return launch_inner_as<256, 1>(a, grid, s.lds, st);
    if (s.max_pairs <= 1024) return launch_inner_as<256, 4>(a, grid, s.lds, st);
    if (s.max_pairs <= 2048) return launch_inner_as<1024, 2>(a, grid, s.lds, st);
    return launch_inner_as<1024, 3>(a, grid, s.lds, st);
}

struct DBuf {
    float *du, *dv;
    size_t stride;
};

// One inner step on n fields: entry (du, dv) in b[*cur]; on return *cur names the buffer that holds the result.  A whole-field
// shape works in place; a tiled one leaves the entry where it is and ping-pongs between the other two buffers.
int run_inner_step(const va_brox_params* p, const Shape& s, InnerArgs a, const DBuf b[3], int* cur, int n, hipStream_t st)
{
    a.TW = s.TW, a.TH = s.TH, a.ntx = s.ntx, a.H = s.H;
    const DBuf& e = b[*cur];
    a.d0[0] = e.du, a.d0[1] = e.dv, a.d0s = e.stride;
    if (s.whole) {
        a.din[0] = e.du, a.din[1] = e.dv, a.dins = e.stride;
        a.dout[0] = e.du, a.dout[1] = e.dv, a.douts = e.stride;
        a.K = p->solver_iters;
        return launch_inner(s, a, n, st);
    }
    const int nl = va_cdiv(p->solver_iters, s.K), base = p->solver_iters / nl, extra = p->solver_iters % nl;
    const int other[2] = {(*cur + 1) % 3, (*cur + 2) % 3};
    int in = *cur;
    for (int i = 0; i < nl; ++i) {
        const int out = other[i & 1];
        a.K = base + (i < extra ? 1 : 0);
        a.din[0] = b[in].du, a.din[1] = b[in].dv, a.dins = b[in].stride;
        a.dout[0] = b[out].du, a.dout[1] = b[out].dv, a.douts = b[out].stride;
        if (int rc = launch_inner(s, a, n, st)) return rc;
        in = out;
    }
    *cur = in;
    return VA_OK;
}

int check_params(const va_brox_params* p)
{
    VA_CHECK_ARG(p != nullptr, "va_brox: params is NULL");
    VA_CHECK_ARG(p->struct_bytes >= (int)sizeof(va_brox_params), "va_brox: params.struct_bytes is %d, need at least %d", p->struct_bytes,
                 (int)sizeof(va_brox_params));
    VA_CHECK_ARG(p->alpha > 0.0f && p->alpha <= 1e6f, "va_brox: alpha must be > 0 (and <= 1e6), got %g", (double)p->alpha);
    VA_CHECK_ARG(p->gamma >= 0.0f && p->gamma <= 1e6f, "va_brox: gamma must be >= 0 (and <= 1e6), got %g", (double)p->gamma);
    VA_CHECK_ARG(p->scale_step > 0.0f && p->scale_step < 1.0f, "va_brox: scale_step must be in (0,1), got %g", (double)p->scale_step);
    VA_CHECK_ARG(p->omega > 0.0f && p->omega < 2.0f, "va_brox: omega must be in (0,2), got %g", (double)p->omega);
    VA_CHECK_ARG(p->epsilon > 0.0f && p->epsilon * p->epsilon > 0.0f && p->epsilon <= 1e6f,
                 "va_brox: epsilon must be > 0 (its square too, and <= 1e6), got %g", (double)p->epsilon);
    VA_CHECK_ARG(p->nscales >= 1, "va_brox: nscales must be >= 1, got %d", p->nscales);
    VA_CHECK_ARG(p->warps >= 1, "va_brox: warps must be >= 1, got %d", p->warps);
    VA_CHECK_ARG(p->inner_iters >= 1, "va_brox: inner_iters must be >= 1, got %d", p->inner_iters);
    VA_CHECK_ARG(p->solver_iters >= 1, "va_brox: solver_iters must be >= 1, got %d", p->solver_iters);
    const int* t = p->tuning;
    VA_CHECK_ARG(t[VA_BROX_TUNE_WHOLE] == -1 || t[VA_BROX_TUNE_WHOLE] == 0, "va_brox: tuning[0] (whole field) must be -1 or 0");
    VA_CHECK_ARG(t[VA_BROX_TUNE_TILE_W] == 0 || (t[VA_BROX_TUNE_TILE_W] >= 2 && t[VA_BROX_TUNE_TILE_W] <= 16384),
                 "va_brox: tuning[1] (tile width) must be 0 or in [2,16384]");
    VA_CHECK_ARG(t[VA_BROX_TUNE_TILE_H] == 0 || (t[VA_BROX_TUNE_TILE_H] >= 2 && t[VA_BROX_TUNE_TILE_H] <= 16384),
                 "va_brox: tuning[2] (tile height) must be 0 or in [2,16384]");
    VA_CHECK_ARG(t[VA_BROX_TUNE_K] >= 0 && t[VA_BROX_TUNE_K] <= kMaxK, "va_brox: tuning[3] (sweeps per launch) must be in [0,%d]", kMaxK);
    VA_CHECK_ARG(t[4] == 0 && t[5] == 0 && t[6] == 0 && t[7] == 0, "va_brox: tuning[4..7] are reserved, must be 0");
    return VA_OK;
}

struct Plan : va_flow_levels {
    Shape shape[kVaMaxScales];
    size_t off_pyr[3][kVaMaxScales], off_tmp, off_state, off_extra, off_ro, total;
};

int make_plan(Plan& P, int w, int h, int n_seq, int fps, const va_brox_params* p)
{
    if (int rc = check_params(p)) return rc;
    if (int rc = va_flow_check_shape("va_brox", w, h, n_seq, fps, true)) return rc;
    va_flow_levels_fill(&P, w, h, n_seq, fps, p->scale_step, p->nscales);
    size_t off = 0;
    for (int s = 0; s < P.ns; ++s) {
        if (int rc = pick_shape(p, P.ws[s], P.hs[s], &P.shape[s])) return rc;
        for (int k = 0; k < 3; ++k) {
            P.off_pyr[k][s] = off;
            off += va_align_up((size_t)P.NF * 3 * P.plane[s] * sizeof(float), 256);
        }
    }
    P.off_tmp = off;
    off += va_align_up((size_t)P.NF * 2 * P.plane_max * sizeof(float), 256);
    P.off_state = off;
    off += va_align_up((size_t)P.NP * 6 * P.plane_max * sizeof(float), 256);
    P.off_extra = off;
    off += va_align_up((size_t)P.NP * 2 * P.plane_max * sizeof(float), 256);
    P.off_ro = off;
    off += va_align_up((size_t)P.NP * kRoPlanes * P.plane_max * sizeof(float), 256);
    P.total = off;
    return VA_OK;
}

void fill_consts(InnerArgs& a, const va_brox_params* p)
{
    a.alpha = p->alpha;
    a.gamma = p->gamma;
    a.eps2 = p->epsilon * p->epsilon;
    a.omega = p->omega;
    a.om1 = 1.0f - p->omega;
}

}  // namespace

extern "C" void va_brox_default_params(va_brox_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_bytes = (int)sizeof(va_brox_params);
    p->alpha = 0.197f;
    p->gamma = 50.0f;
    p->scale_step = 0.8f;
    p->omega = 1.9f;
    p->epsilon = 1e-3f;
    p->nscales = 16;
    p->warps = 1;
    p->inner_iters = 10;
    p->solver_iters = 10;
    p->tuning[VA_BROX_TUNE_WHOLE] = -1;
}

extern "C" size_t va_brox_workspace_bytes(int w, int h, int n_seq, int frames_per_seq, const va_brox_params* p)
{
    Plan P;
    if (make_plan(P, w, h, n_seq, frames_per_seq, p) != VA_OK) return 0;
    return P.total;
}

extern "C" int va_brox_flow(va_ctx* ctx, const void* frames, int frames_are_u8, int n_seq, int frames_per_seq, int w, int h,
                            const va_brox_params* p, void* flow, void* workspace, size_t workspace_bytes, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_brox_flow: ctx is NULL");
    VA_USE_DEVICE(ctx);
    if (int rc = va_flow_check_buffers("va_brox_flow", frames, flow, workspace, 0, 0)) return rc;
    Plan P;
    if (int rc = make_plan(P, w, h, n_seq, frames_per_seq, p)) return rc;
    if (int rc = va_flow_check_buffers("va_brox_flow", frames, flow, workspace, workspace_bytes, P.total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* pyr[3][kVaMaxScales];
    for (int k = 0; k < 3; ++k)
        for (int s = 0; s < P.ns; ++s) pyr[k][s] = (float*)(ws + P.off_pyr[k][s]);
    float* tmp1 = (float*)(ws + P.off_tmp);
    float* tmp2 = tmp1 + (size_t)P.NF * P.plane_max;
    float* state = (float*)(ws + P.off_state);
    float* extra = (float*)(ws + P.off_extra);
    float* ro = (float*)(ws + P.off_ro);
    const int TPB = 256;

    // S57: frames / 255, S1's pyramid, S2 applied to I, then to Ix and to Iy
    if (int rc = va_stage_frames(frames, frames_are_u8, true, pyr[0][0], w, h, P.pitch[0], P.plane[0], P.NF, st)) return rc;
    if (int rc = va_stage_pyramid(pyr[0], P.ws, P.hs, P.pitch, P.plane, P.ns, P.NF, tmp1, tmp2, P.plane_max, p->scale_step, st)) return rc;
    for (int s = 0; s < P.ns; ++s) {
        const size_t pl = P.plane[s], row = 3 * pl * sizeof(float);
        if (int rc = va_stage_gradient(pyr[0][s], P.ws[s], P.hs[s], P.pitch[s], pl, P.NF, st)) return rc;
        for (int k = 1; k < 3; ++k) {  // plane 0 of block k <- Ix (k = 1) or Iy (k = 2), then its gradient
            VA_HIP(hipMemcpy2DAsync(pyr[k][s], row, pyr[0][s] + k * pl, row, pl * sizeof(float), P.NF, hipMemcpyDeviceToDevice, st));
            if (int rc = va_stage_gradient(pyr[k][s], P.ws[s], P.hs[s], P.pitch[s], pl, P.NF, st)) return rc;
        }
    }

    // u = v = 0 at the coarsest level (padding included)
    const int sc = P.ns - 1;
    VA_HIP(hipMemsetAsync(state, 0, (size_t)P.NP * 6 * P.plane[sc] * sizeof(float), st));
    for (int s = sc; s >= 0; --s) {
        const int lw = P.ws[s], lh = P.hs[s], lp = P.pitch[s];
        const size_t pl = P.plane[s];
        const DBuf bufs[3] = {{state + 2 * pl, state + 3 * pl, 6 * pl}, {state + 4 * pl, state + 5 * pl, 6 * pl}, {extra, extra + pl, 2 * pl}};
        InnerArgs a{};
        fill_consts(a, p);
        a.w = lw, a.h = lh, a.pitch = lp;
        for (int f = 0; f < kRoPlanes; ++f) a.fld[f] = ro + f * pl, a.fs[f] = kRoPlanes * pl;
        a.fld[F_U] = state, a.fld[F_V] = state + pl, a.fs[F_U] = a.fs[F_V] = 6 * pl;
        for (int wp = 0; wp < p->warps; ++wp) {
            int cur = 0;
            k_brox_warp<<<dim3(va_cdiv((lp / 4) * lh, TPB), P.NP), TPB, 0, st>>>(pyr[0][s], pyr[1][s], pyr[2][s], pl, lw, lh, lp, P.F, state, ro,
                                                                                  bufs[0].du, bufs[0].dv, bufs[0].stride);
            VA_LAUNCH_CHECK();
            for (int it = 0; it < p->inner_iters; ++it)
                if (int rc = run_inner_step(p, P.shape[s], a, bufs, &cur, P.NP, st)) return rc;
            const int n4 = (lp / 4) * lh;
            k_brox_update<<<dim3(va_cdiv(n4, TPB), P.NP), TPB, 0, st>>>(state, pl, n4, bufs[cur].du, bufs[cur].dv, bufs[cur].stride);
            VA_LAUNCH_CHECK();
        }
        if (s > 0) {  // S8 (ro is free between levels: the upsampling's target)
            if (int rc = va_stage_upsample(state, lw, lh, lp, pl, ro, state, P.ws[s - 1], P.hs[s - 1], P.pitch[s - 1], P.plane[s - 1],
                                           1.0f / p->scale_step, P.NP, st))
                return rc;
        }
    }
    return va_stage_flow_out(state, w, h, P.pitch[0], P.plane[0], (float*)flow, P.NP, st);
}

extern "C" int va_brox_inner_step(va_ctx* ctx, const void* I0x, const void* I0y, const void* I1w, const void* I1wx, const void* I1wy,
                                  const void* I1wxx, const void* I1wxy, const void* I1wyy, const void* Iz, const void* Ixz,
                                  const void* Iyz, const void* u, const void* v, void* du, void* dv, int n, int w, int h,
                                  const va_brox_params* p, void* scratch, size_t scratch_bytes, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_brox_inner_step: ctx is NULL");
    VA_USE_DEVICE(ctx);
    (void)I0x, (void)I0y, (void)I1w;
    VA_CHECK_ARG(I1wx && I1wy && I1wxx && I1wxy && I1wyy && Iz && Ixz && Iyz && u && v && du && dv, "va_brox_inner_step: NULL field");
    if (int rc = check_params(p)) return rc;
    if (int rc = va_flow_check_fields("va_brox_inner_step", n, w, h)) return rc;
    Shape s;
    if (int rc = pick_shape(p, w, h, &s)) return rc;
    const size_t fl = (size_t)w * h;
    if (!s.whole) {
        VA_CHECK_ARG(scratch != nullptr && ((uintptr_t)scratch & 255) == 0, "va_brox_inner_step: scratch must be a 256-byte aligned buffer");
        if (scratch_bytes < 4 * (size_t)n * fl * sizeof(float)) {
            va_set_error("va_brox_inner_step: scratch too small (%zu < %zu bytes)", scratch_bytes, 4 * (size_t)n * fl * sizeof(float));
            return VA_ERR_WORKSPACE;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    float* sc = (float*)scratch;
    const DBuf bufs[3] = {{(float*)du, (float*)dv, fl}, {sc, sc + n * fl, fl}, {sc + 2 * n * fl, sc + 3 * n * fl, fl}};
    InnerArgs a{};
    fill_consts(a, p);
    a.w = w, a.h = h, a.pitch = w;
    const void* f[F_COUNT] = {I1wx, I1wy, I1wxx, I1wxy, I1wyy, Iz, Ixz, Iyz, u, v};
    for (int k = 0; k < F_COUNT; ++k) a.fld[k] = (const float*)f[k], a.fs[k] = fl;
    int cur = 0;
    if (int rc = run_inner_step(p, s, a, bufs, &cur, n, st)) return rc;
    if (cur != 0) {
        VA_HIP(hipMemcpyAsync(du, bufs[cur].du, (size_t)n * fl * sizeof(float), hipMemcpyDeviceToDevice, st));
        VA_HIP(hipMemcpyAsync(dv, bufs[cur].dv, (size_t)n * fl * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return VA_OK;
}
