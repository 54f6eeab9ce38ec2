// The motion inputs of the two-stream paper's temporal-ConvNet comparison on full-frame float flow:
// per-field means (mean flow subtraction) and the trajectory-stacking resampler.  Both read the TV-L1 buffer
// [B*L][2][h][w] and the resampler writes another array of the same shape and pair order, so that every S9 / S10 consumer
// applies to its output unchanged.  Bi-directional flow (S13) is a reordering of the gray frames before TV-L1 and needs no
// kernel of its own.
#include "va_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// S11: one workgroup per (pair, component) plane.  Each value is clamped to [-32768, 32768] (a NaN becomes -32768) and
// scaled by 2^16 into an integer, exactly; the int64 sum of those integers is the same in any order, so the per-thread,
// per-wave and per-workgroup partial sums below give the numpy restatement's bits.  No atomics, no workspace.
constexpr int kMeansThreads = 512;
constexpr int kMeansUnroll = 4;

__device__ __forceinline__ long long fixed16(float v)
{
    const float a = fminf(fmaxf(v, -32768.0f), 32768.0f);
    return (long long)rintf(a * 65536.0f);  // |a * 2^16| <= 2^31: exact in float, and in int64
}

__global__ void __launch_bounds__(kMeansThreads) k_flow_field_means(const float* __restrict__ flow, float* __restrict__ means,
                                                                   int w, int h, int vec4)
{
    const int n = w * h;
    const float* __restrict__ plane = flow + (size_t)blockIdx.x * n;
    long long s = 0;
    if (vec4) {  // 16-byte aligned planes of a multiple of 4 floats
        const f32x4* __restrict__ p4 = reinterpret_cast<const f32x4*>(plane);
        const int n4 = n >> 2;
        int i = threadIdx.x;
        for (; i + (kMeansUnroll - 1) * kMeansThreads < n4; i += kMeansUnroll * kMeansThreads) {
            f32x4 v[kMeansUnroll];
#pragma unroll
            for (int u = 0; u < kMeansUnroll; ++u) v[u] = p4[i + u * kMeansThreads];
#pragma unroll
            for (int u = 0; u < kMeansUnroll; ++u) s += fixed16(v[u][0]) + fixed16(v[u][1]) + fixed16(v[u][2]) + fixed16(v[u][3]);
        }
        for (; i < n4; i += kMeansThreads) {
            const f32x4 v = p4[i];
            s += fixed16(v[0]) + fixed16(v[1]) + fixed16(v[2]) + fixed16(v[3]);
        }
    } else {
        for (int i = threadIdx.x; i < n; i += kMeansThreads) s += fixed16(plane[i]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    __shared__ long long part[kMeansThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
#pragma unroll
        for (int k = 0; k < kMeansThreads / 64; ++k) t += part[k];
        means[blockIdx.x] = (float)((double)t / ((double)n * 65536.0));
    }
}

// S12's bilinear sample of plane f at (px, py): va_bilinear_plain (va_internal.h) on dense rows
__device__ __forceinline__ float bilinear(const float* __restrict__ f, int w, int h, float px, float py)
{
    return va_bilinear_plain(f, w, h, w, px, py);
}

// S12: flow f32 [n_chains*chain_len][2][h][w] -> out of the same shape.  Block (blockIdx.x, blockIdx.y = chain b): the
// blocks of one chain are adjacent in dispatch order, so that the taps of its pairs come from L2 / the Infinity Cache.
// Each thread owns kMotionPx consecutive pixels of the frame (horizontally adjacent trajectories) and walks all chain_len
// pairs of the chain:
//   TRAJ:  out[n][c](y, x) = bilinear(flow[n][c], p_k) (- m[n][c]), p_0 = (x, y), p_{k+1} = p_k + d (the raw flow);
//   !TRAJ: out[n][c] = flow[n][c] - m[n][c] (mean flow subtraction of the stacked flow).
// vec4 bit 0: 16-byte aligned out and planes of a multiple of 4 floats: one 16-byte store per pair and component (and,
// for !TRAJ with bit 1, an aligned flow: one 16-byte load).
constexpr int kMotionThreads = 256;
constexpr int kMotionPx = 4;

template <bool TRAJ>
__global__ void __launch_bounds__(kMotionThreads) k_flow_motion(const float* __restrict__ flow, const float* __restrict__ means,
                                                                float* __restrict__ out, int w, int h, int chain_len, int vec4)
{
    const int n = w * h;
    const int i0 = (blockIdx.x * kMotionThreads + threadIdx.x) * kMotionPx;
    if (i0 >= n) return;
    const size_t chain0 = (size_t)blockIdx.y * chain_len;
    float px[kMotionPx], py[kMotionPx];
    if (TRAJ) {
        int y = i0 / w, x = i0 - y * w;
#pragma unroll
        for (int j = 0; j < kMotionPx; ++j) {
            px[j] = (float)x;
            py[j] = (float)y;
            if (++x == w) x = 0, ++y;
        }
    }
    for (int k = 0; k < chain_len; ++k) {
        const size_t pair = chain0 + k;
        const float* __restrict__ fx = flow + pair * 2 * n;
        const float* __restrict__ fy = fx + n;
        float dx[kMotionPx], dy[kMotionPx];
        if (TRAJ) {
#pragma unroll
            for (int j = 0; j < kMotionPx; ++j) {
                dx[j] = bilinear(fx, w, h, px[j], py[j]);
                dy[j] = bilinear(fy, w, h, px[j], py[j]);
            }
        } else if (vec4 & 2) {
            const f32x4 vx = *reinterpret_cast<const f32x4*>(fx + i0), vy = *reinterpret_cast<const f32x4*>(fy + i0);
#pragma unroll
            for (int j = 0; j < kMotionPx; ++j) dx[j] = vx[j], dy[j] = vy[j];
        } else {
#pragma unroll
            for (int j = 0; j < kMotionPx; ++j) {
                dx[j] = i0 + j < n ? fx[i0 + j] : 0.0f;
                dy[j] = i0 + j < n ? fy[i0 + j] : 0.0f;
            }
        }
        float ox[kMotionPx], oy[kMotionPx];
        const float mx = means ? means[2 * pair] : 0.0f, my = means ? means[2 * pair + 1] : 0.0f;
#pragma unroll
        for (int j = 0; j < kMotionPx; ++j) {
            ox[j] = means ? dx[j] - mx : dx[j];
            oy[j] = means ? dy[j] - my : dy[j];
            if (TRAJ) {  // the trajectory follows the raw flow
                px[j] = px[j] + dx[j];
                py[j] = py[j] + dy[j];
            }
        }
        float* __restrict__ ox_dst = out + pair * 2 * n;
        float* __restrict__ oy_dst = ox_dst + n;
        if (vec4 & 1) {
            *reinterpret_cast<f32x4*>(ox_dst + i0) = f32x4{ox[0], ox[1], ox[2], ox[3]};
            *reinterpret_cast<f32x4*>(oy_dst + i0) = f32x4{oy[0], oy[1], oy[2], oy[3]};
        } else {
#pragma unroll
            for (int j = 0; j < kMotionPx; ++j)
                if (i0 + j < n) ox_dst[i0 + j] = ox[j], oy_dst[i0 + j] = oy[j];
        }
    }
}

static constexpr int kMaxGridY = 65535;
static constexpr long long kMaxPlane = 0x7fffffffLL - 3 * kMotionThreads * kMotionPx;  // w*h and i0 + 3 stay in int

extern "C" int va_flow_field_means(va_ctx* ctx, const void* flow, int n_pairs, int w, int h, void* means, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_flow_field_means: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(flow != nullptr && means != nullptr, "va_flow_field_means: NULL buffer");
    VA_CHECK_ARG(n_pairs >= 1 && w >= 1 && h >= 1, "va_flow_field_means: bad shape");
    VA_CHECK_ARG((long long)w * h <= kMaxPlane, "va_flow_field_means: %dx%d planes exceed one launch", w, h);
    VA_CHECK_ARG(2LL * n_pairs <= 0x7fffffffLL, "va_flow_field_means: %d pairs exceed one launch", n_pairs);
    const int vec4 = (w * h) % 4 == 0 && reinterpret_cast<uintptr_t>(flow) % 16 == 0;
    k_flow_field_means<<<(unsigned)(2 * n_pairs), kMeansThreads, 0, (hipStream_t)stream>>>((const float*)flow, (float*)means,
                                                                                          w, h, vec4);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_flow_motion(va_ctx* ctx, const void* flow, int n_chains, int chain_len, int trajectory, int w, int h,
                              const void* means, void* out, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_flow_motion: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(flow != nullptr && out != nullptr, "va_flow_motion: NULL buffer");
    VA_CHECK_ARG(n_chains >= 1 && chain_len >= 1 && w >= 1 && h >= 1, "va_flow_motion: bad shape");
    VA_CHECK_ARG(trajectory == 0 || trajectory == 1, "va_flow_motion: trajectory must be 0 or 1");
    VA_CHECK_ARG(trajectory || means != nullptr, "va_flow_motion: nothing to do (no trajectory and no means)");
    VA_CHECK_ARG(n_chains <= kMaxGridY, "va_flow_motion: %d chains exceed %d per call", n_chains, kMaxGridY);
    VA_CHECK_ARG((long long)w * h <= kMaxPlane, "va_flow_motion: %dx%d planes exceed one launch", w, h);
    const int n = w * h;
    const int vec4 = (n % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0 ? 1 : 0) |
                     (n % 4 == 0 && reinterpret_cast<uintptr_t>(flow) % 16 == 0 ? 2 : 0);
    const dim3 g((unsigned)va_cdiv(n, kMotionThreads * kMotionPx), (unsigned)n_chains);
    if (trajectory)
        k_flow_motion<true><<<g, kMotionThreads, 0, (hipStream_t)stream>>>((const float*)flow, (const float*)means,
                                                                            (float*)out, w, h, chain_len, vec4);
    else
        k_flow_motion<false><<<g, kMotionThreads, 0, (hipStream_t)stream>>>((const float*)flow, (const float*)means,
                                                                             (float*)out, w, h, chain_len, vec4);
    VA_LAUNCH_CHECK();
    return VA_OK;
}
