// Video-level aggregation and two-stream fusion on the device:
// the AverageMeter bank of validate() (Sheet03/utils.py:154-171, Sheet03/spatialModel.py:223-228)
// and LinearSVC.predict of the fusion step (Sheet03/combinedModel.py:38); the consensus over a video's snippets and
// views and the weighted average of the two streams' scores (the test protocols of
// Sheet03/notes.txt:113-116,121-124,225-230).  All are small,
// HBM/latency-bound byte-and-index work: plain coalesced kernels, no MFMA.  (The fit of the SVM, which does use the f64
// MFMA, is in svm.hip.)
#include "va_internal.h"

namespace {

// One thread per descriptor column walks the batch in order: a video that occurs several times in
// one batch receives its adds in batch order, exactly like the reference's Python loop, so the f32
// sums are bit-identical to AverageMeter.update() called row by row.
__global__ void k_meter_update(const float* __restrict__ desc, const int* __restrict__ slot, int B, int D, float* __restrict__ sums,
                               int* __restrict__ counts, int n_slots)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    for (int b = 0; b < B; ++b) {
        const int s = slot[b];
        if (s < 0 || s >= n_slots) continue;  // padding rows
        sums[(size_t)s * D + d] += desc[(size_t)b * D + d];
        if (d == 0) counts[s] += 1;
    }
}

__global__ void k_meter_average(const float* __restrict__ sums, const int* __restrict__ counts, int n_slots, int D, float* __restrict__ avg)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_slots * D) return;
    const int c = counts[i / D];
    avg[i] = c > 0 ? sums[i] / (float)c : 0.0f;
}

// scores[n][c] = sum_k x[n][k] * coef[c][k] (k ascending, IEEE double multiply then add: -ffp-contract=off)
// + intercept[c].  One workgroup per row n: the row is staged in LDS, thread c walks coef row c.
template <bool STAGED>
__global__ void k_svm_scores(const double* __restrict__ x, int dim, const double* __restrict__ coef, const double* __restrict__ intercept,
                             int C, double* __restrict__ scores)
{
    extern __shared__ double sx[];
    const int n = blockIdx.x;
    const double* __restrict__ xr = x + (size_t)n * dim;  // !STAGED (dim > 8192 doubles of LDS): the row is read in place
    if (STAGED) {
        for (int k = threadIdx.x; k < dim; k += blockDim.x) sx[k] = xr[k];
        __syncthreads();
    }
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const double* w = coef + (size_t)c * dim;
        double acc = 0.0;
        for (int k = 0; k < dim; ++k) acc = acc + (STAGED ? sx[k] : xr[k]) * w[k];
        scores[(size_t)n * C + c] = acc + intercept[c];
    }
}

// LinearSVC.predict: arg-max over classes (first maximum, like numpy.argmax); one class row
// (binary problem): index of (score > 0).
__global__ void k_svm_argmax(const double* __restrict__ scores, int N, int C, int* __restrict__ pred)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const double* s = scores + (size_t)n * C;
    if (C == 1) {
        pred[n] = s[0] > 0.0 ? 1 : 0;
        return;
    }
    double mx = s[0];
    int am = 0;
    for (int c = 1; c < C; ++c)
        if (s[c] > mx) { mx = s[c]; am = c; }
    pred[n] = am;
}

// Wave-wide max and sum over 64 lanes as xor butterflies (offsets 32, 16, ..., 1): every lane ends with the same bits, and
// the order of the additions is fixed by the lane numbers, not by scheduling.  fmaxf skips NaNs; the sums carry them.
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// The softmax terms of one row x[0..c) for a whole wave: m = max_j x_j and s = sum_j exp(x_j - m), lane l adding its
// classes l, l + 64, ... in ascending order before the butterfly.  A NaN in the row makes s NaN (exp(NaN - m)); a row of
// -inf or one holding +inf makes it NaN too (inf - inf).
__device__ __forceinline__ void wave_softmax_terms(const float* __restrict__ x, int c, int lane, float& m, float& s)
{
    float mx = -INFINITY;
    for (int j = lane; j < c; j += 64) mx = fmaxf(mx, x[j]);
    m = wave_max(mx);
    float acc = 0.0f;
    for (int j = lane; j < c; j += 64) acc = acc + expf(x[j] - m);
    s = wave_sum(acc);
}

// S16, the consensus of one video per workgroup: logits [n][k][c] -> scores [n][c].
//   mode 0: phase one, wave per item (items wave, wave + 4, ...): the item's max and exp-sum into LDS; phase two, thread per
//           class (classes t, t + 256, ...): acc = p_0 + p_1 + ... in item order with p_i = exp(x_ij - m_i) / s_i, then
//           acc / (float)k.
//   mode 1: thread per class: the mean of the logits in item order into LDS, then every wave computes the one softmax's
//           max and sum for itself (the same bits in all four) and the threads write exp(mean_j - m) / s.
// LDS: 2k floats (m, s) followed by c floats (the mean logits).  No atomics.
__global__ void __launch_bounds__(256) k_score_consensus(const float* __restrict__ logits, int k, int c, int mode,
                                                         float* __restrict__ scores)
{
    extern __shared__ float lds[];
    const float* __restrict__ x = logits + (size_t)blockIdx.x * k * c;
    float* __restrict__ out = scores + (size_t)blockIdx.x * c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (mode == 0) {
        float* im = lds;
        float* is = lds + k;
        for (int i = wave; i < k; i += 4) {
            float m, s;
            wave_softmax_terms(x + (size_t)i * c, c, lane, m, s);
            if (lane == 0) im[i] = m, is[i] = s;
        }
        __syncthreads();
        for (int j = threadIdx.x; j < c; j += 256) {
            float acc = expf(x[j] - im[0]) / is[0];
            for (int i = 1; i < k; ++i) acc = acc + expf(x[(size_t)i * c + j] - im[i]) / is[i];
            out[j] = acc / (float)k;
        }
    } else {
        float* mean = lds + 2 * k;
        for (int j = threadIdx.x; j < c; j += 256) {
            float acc = x[j];
            for (int i = 1; i < k; ++i) acc = acc + x[(size_t)i * c + j];
            mean[j] = acc / (float)k;
        }
        __syncthreads();
        float m, s;
        wave_softmax_terms(mean, c, lane, m, s);
        for (int j = threadIdx.x; j < c; j += 256) out[j] = expf(mean[j] - m) / s;
    }
}

// S16, the fusion of one video per workgroup: fused = (wa*a + wb*b) / (wa + wb), each operation rounded to f32; thread 0
// then walks the classes as k_svm_argmax does (strict >, so the first maximum wins), recomputing the same expression.
__global__ void __launch_bounds__(256) k_fuse_scores(const float* __restrict__ a, const float* __restrict__ b, int c, float wa,
                                                     float wb, float* __restrict__ fused, int* __restrict__ pred)
{
    const float* __restrict__ pa = a + (size_t)blockIdx.x * c;
    const float* __restrict__ pb = b + (size_t)blockIdx.x * c;
    const float wsum = wa + wb;
    for (int j = threadIdx.x; j < c; j += 256) fused[(size_t)blockIdx.x * c + j] = (wa * pa[j] + wb * pb[j]) / wsum;
    if (threadIdx.x == 0) {
        float mx = (wa * pa[0] + wb * pb[0]) / wsum;
        int am = 0;
        for (int j = 1; j < c; ++j) {
            const float f = (wa * pa[j] + wb * pb[j]) / wsum;
            if (f > mx) { mx = f; am = j; }
        }
        pred[blockIdx.x] = am;
    }
}

// S24, the fusion of m streams: fused = (((w0*a0 + w1*a1) + w2*a2) + ...) / (((w0 + w1) + w2) + ...), every operation
// rounded to f32 in stream order; the arg-max as k_fuse_scores'.  m = 2 is k_fuse_scores' expression.
constexpr int kFuseMaxStreams = 8;
struct FuseStreams {
    const float* p[kFuseMaxStreams];
    float w[kFuseMaxStreams];
};

__device__ __forceinline__ float fuse_n(const FuseStreams& s, int m, size_t i, float wsum)
{
    float acc = s.w[0] * s.p[0][i];
#pragma unroll  // constant indices into the kernel arguments: no private copy of the struct
    for (int k = 1; k < kFuseMaxStreams; ++k)
        if (k < m) acc = acc + s.w[k] * s.p[k][i];
    return acc / wsum;
}

__global__ void __launch_bounds__(256) k_fuse_scores_n(FuseStreams s, int m, int c, float* __restrict__ fused, int* __restrict__ pred)
{
    const size_t row = (size_t)blockIdx.x * c;
    float wsum = s.w[0];
#pragma unroll
    for (int k = 1; k < kFuseMaxStreams; ++k)
        if (k < m) wsum = wsum + s.w[k];
    for (int j = threadIdx.x; j < c; j += 256) fused[row + j] = fuse_n(s, m, row + j, wsum);
    if (threadIdx.x == 0) {
        float mx = fuse_n(s, m, row, wsum);
        int am = 0;
        for (int j = 1; j < c; ++j) {
            const float f = fuse_n(s, m, row + j, wsum);
            if (f > mx) { mx = f; am = j; }
        }
        pred[blockIdx.x] = am;
    }
}

}  // namespace

static constexpr int kConsensusMaxItems = 4096, kConsensusMaxClasses = 4096;  // (2k + c) floats of LDS: at most 48 KB

extern "C" int va_score_consensus(va_ctx* ctx, const void* logits, int n, int k, int c, int mode, void* scores, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_score_consensus: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(logits && scores, "va_score_consensus: NULL pointer");
    VA_CHECK_ARG(n >= 1 && k >= 1 && c >= 1 && k <= kConsensusMaxItems && c <= kConsensusMaxClasses,
                 "va_score_consensus: need n >= 1, 1 <= k <= %d items, 1 <= c <= %d classes (got %d, %d, %d)", kConsensusMaxItems,
                 kConsensusMaxClasses, n, k, c);
    VA_CHECK_ARG(mode == 0 || mode == 1, "va_score_consensus: mode must be 0 (softmax) or 1 (logits), got %d", mode);
    k_score_consensus<<<n, 256, (size_t)(2 * k + c) * sizeof(float), (hipStream_t)stream>>>((const float*)logits, k, c, mode,
                                                                                            (float*)scores);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_fuse_scores(va_ctx* ctx, const void* a, const void* b, int n, int c, float wa, float wb, void* fused, void* pred,
                              void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_fuse_scores: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(a && b && fused && pred, "va_fuse_scores: NULL pointer");
    VA_CHECK_ARG(n >= 1 && c >= 1, "va_fuse_scores: need n >= 1 and c >= 1 (got %d, %d)", n, c);
    VA_CHECK_ARG(wa >= 0.0f && wb >= 0.0f && wa + wb > 0.0f && wa + wb <= 3.0e38f,
                 "va_fuse_scores: need finite weights >= 0 with a positive sum (got %g, %g)", (double)wa, (double)wb);
    k_fuse_scores<<<n, 256, 0, (hipStream_t)stream>>>((const float*)a, (const float*)b, c, wa, wb, (float*)fused, (int*)pred);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_fuse_scores_n(va_ctx* ctx, const void* const* scores, const float* weights, int m, int n, int c, void* fused,
                                void* pred, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_fuse_scores_n: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(m >= 2 && m <= kFuseMaxStreams, "va_fuse_scores_n: need 2 <= m <= %d streams (got %d)", kFuseMaxStreams, m);
    VA_CHECK_ARG(scores && weights && fused && pred, "va_fuse_scores_n: NULL pointer");
    VA_CHECK_ARG(n >= 1 && c >= 1, "va_fuse_scores_n: need n >= 1 and c >= 1 (got %d, %d)", n, c);
    FuseStreams s = {};
    float wsum = 0.0f;
    for (int k = 0; k < m; ++k) {
        VA_CHECK_ARG(scores[k] != nullptr, "va_fuse_scores_n: scores[%d] is NULL", k);
        VA_CHECK_ARG(weights[k] >= 0.0f && weights[k] <= 3.0e38f, "va_fuse_scores_n: need finite weights >= 0 (weights[%d] = %g)", k,
                     (double)weights[k]);
        s.p[k] = (const float*)scores[k];
        s.w[k] = weights[k];
        wsum = k == 0 ? weights[0] : wsum + weights[k];
    }
    VA_CHECK_ARG(wsum > 0.0f && wsum <= 3.0e38f, "va_fuse_scores_n: the weights need a positive finite sum (got %g)", (double)wsum);
    k_fuse_scores_n<<<n, 256, 0, (hipStream_t)stream>>>(s, m, c, (float*)fused, (int*)pred);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_meter_update(va_ctx* ctx, const void* desc, const void* slot, int batch, int dim, void* sums, void* counts, int n_slots,
                               void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_meter_update: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(desc && slot && sums && counts, "va_meter_update: NULL pointer");
    VA_CHECK_ARG(batch >= 1 && dim >= 1 && n_slots >= 1, "va_meter_update: batch, dim, n_slots must be >= 1 (got %d, %d, %d)", batch, dim, n_slots);
    k_meter_update<<<va_cdiv(dim, 256), 256, 0, (hipStream_t)stream>>>((const float*)desc, (const int*)slot, batch, dim, (float*)sums,
                                                                       (int*)counts, n_slots);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_meter_average(va_ctx* ctx, const void* sums, const void* counts, int n_slots, int dim, void* avg, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_meter_average: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(sums && counts && avg, "va_meter_average: NULL pointer");
    VA_CHECK_ARG(dim >= 1 && n_slots >= 1, "va_meter_average: dim, n_slots must be >= 1 (got %d, %d)", dim, n_slots);
    const size_t n = (size_t)n_slots * dim;
    k_meter_average<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>((const float*)sums, (const int*)counts, n_slots, dim, (float*)avg);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_linear_svm_predict(va_ctx* ctx, const void* x, int n, int dim, const void* coef, const void* intercept, int n_class_rows,
                                     void* scores, void* pred, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_linear_svm_predict: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x && coef && intercept && scores && pred, "va_linear_svm_predict: NULL pointer");
    VA_CHECK_ARG(n >= 1 && dim >= 1 && dim <= 65536 && n_class_rows >= 1,
                 "va_linear_svm_predict: need n >= 1, 1 <= dim <= 65536, n_class_rows >= 1 (got %d, %d, %d)", n, dim, n_class_rows);
    if (dim <= 8192)  // 64 KB of LDS hold 8192 doubles
        k_svm_scores<true><<<n, 128, (size_t)dim * sizeof(double), (hipStream_t)stream>>>((const double*)x, dim, (const double*)coef,
                                                                                         (const double*)intercept, n_class_rows, (double*)scores);
    else
        k_svm_scores<false><<<n, 128, 0, (hipStream_t)stream>>>((const double*)x, dim, (const double*)coef, (const double*)intercept,
                                                                n_class_rows, (double*)scores);
    VA_LAUNCH_CHECK();
    k_svm_argmax<<<va_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>((const double*)scores, n, n_class_rows, (int*)pred);
    VA_LAUNCH_CHECK();
    return VA_OK;
}
