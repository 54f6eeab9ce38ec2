// Gradient accumulation and the separate update: what va_vgg16_train_accumulate adds to the training step
// beside the finishing kernels' STORE / ADD forms (train.hip), and va_vgg16_train_apply, the momentum-SGD update of all 34
// parameter tensors from the caller's gradient buffer with torch's clip_grad_norm_ in front of it.  The kernels live in a file
// of their own, as multitask.hip's: tests/test_train_kernels_gpu.py pins the set of kernels train.hip launches to its own
// table, and these kernels' tests are tests/test_accum_gpu.py's.
#include "vgg_internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSegs = 34;
constexpr int kTileFloats = 4096;  // a tile = 256 threads x 4 x 16 bytes of one segment
constexpr int kNormBlocks = 1024;  // FIXED: the partial sums of the norm, and with them its bits, do not depend on the device
constexpr int kApplyBlocks = 2048; // 256 CUs x 8 workgroups of 256 threads

struct Scales {
    float s[VA_MAX_HEADS];
};

// dlogits[r][c] *= s[head of column c]: a micro-batch's share of the full batch's mean
__global__ void k_scale_dlogits(float* __restrict__ d, int rows, int C, va_heads h, Scales sc)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)rows * C) return;
    const int c = (int)(i % (size_t)C);
    float s = sc.s[0];
#pragma unroll
    for (int q = 1; q < VA_MAX_HEADS; ++q)  // constant indices only: both tables stay in registers
        if (q < h.n && c >= h.off[q]) s = sc.s[q];
    d[i] = d[i] * s;
}

// The 34 segments by value: one launch walks them all.  tile0[s] = the first tile of segment s, tile0[34] = the number of tiles.
// lr[s], wd[s]: the tensor's lr_t and wd_t under the model's solver.  frozen[s]: the tensor takes no update and
// does not enter the norm -- such a segment owns NO tiles (tile0[s + 1] == tile0[s]), so no workgroup ever meets it.
struct SegTable {
    float* w[kSegs];
    float* v[kSegs];
    unsigned long long goff[kSegs], cnt[kSegs];
    unsigned tile0[kSegs + 1];
    float lr[kSegs], wd[kSegs];
    unsigned char frozen[kSegs];
};

struct Seg {
    float* w;
    float* v;
    unsigned long long goff, cnt;
    unsigned tile0;
    float lr, wd;
};

// The table is the FIRST argument of its kernels and is read where it lies, in the kernel-argument segment (constant address
// space: uniform scalar loads, any index): indexing the by-value copy with a run-time index would move all of it to scratch.
typedef const SegTable __attribute__((address_space(4))) * SegTablePtr;
__device__ __forceinline__ SegTablePtr seg_table_arg() { return (SegTablePtr)__builtin_amdgcn_kernarg_segment_ptr(); }

// the segment of a tile: the last one whose first tile is not above it (uniform over the workgroup); a frozen segment's
// first tile is its successor's, so the walk passes it
__device__ __forceinline__ Seg seg_of(SegTablePtr T, unsigned tile)
{
    int q = 0;
    while (q + 1 < kSegs && tile >= T->tile0[q + 1]) ++q;
    return Seg{T->w[q], T->v[q], T->goff[q], T->cnt[q], T->tile0[q], T->lr[q], T->wd[q]};
}

// Stage 1 of the norm: part[block] = the float64 sum of squares of the block's tiles (tile = block, block + grid, ...), every
// thread over its own elements in ascending order, then a fixed tree over the 256 threads.  x*x is exact in float64.
__global__ void __launch_bounds__(256) k_grad_sumsq_partial(SegTable T, const float* __restrict__ G, double* __restrict__ part)
{
    __shared__ double red[256];
    double acc = 0.0;
    const SegTablePtr Tp = seg_table_arg();
    for (unsigned tile = blockIdx.x; tile < Tp->tile0[kSegs]; tile += gridDim.x) {
        const Seg s = seg_of(Tp, tile);
        const float* g = G + s.goff;
        const unsigned long long base = (unsigned long long)(tile - s.tile0) * kTileFloats;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long e = base + (unsigned long long)(j * 256 + threadIdx.x) * 4;
            if (e + 3 < s.cnt) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(g + e);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc = fma((double)q[i], (double)q[i], acc);
            } else {
                for (unsigned long long i = e; i < s.cnt; ++i) acc = fma((double)g[i], (double)g[i], acc);
            }
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// Stage 2, one workgroup: thread t adds part[t], part[t + 256], ... in that order, the same tree, norm = sqrt(sum)
__global__ void __launch_bounds__(256) k_grad_norm_finish(const double* __restrict__ part, int n, double* __restrict__ norm,
                                                          double* __restrict__ norm_out)
{
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc = acc + part[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double nrm = sqrt(red[0]);
        norm[0] = nrm;
        if (norm_out) norm_out[0] = nrm;
    }
}

// one element of the update: finish_grad's UPD_SGD statements (train.hip) on g, or on c g under clipping.  wd == 0 is a path
// of its own (an infinite weight keeps its result); otherwise the decay joins the clipped gradient, then the momentum.
__device__ __forceinline__ void sgd_element(float g, float v, float w, float lr, float mu, float wd, float& nv, float& nw)
{
    if (wd == 0.0f) {
        nv = fmaf(mu, v, g);
    } else {
        nv = fmaf(mu, v, fmaf(wd, w, g));
    }
    nw = fmaf(-lr, nv, w);
}

// V = fmaf(mu, V, c G); W = fmaf(-lr_t, V, W) over all unfrozen segments, with wd_t != 0: V = fmaf(mu, V, fmaf(wd_t, W, c G)):
// the fused multiply-adds of the fused step's finishing kernels, lr_t and wd_t per segment.  CLIP: c = min(1, clip / (norm +
// 1e-6)) (torch.nn.utils.clip_grad_norm_), read from the device; without CLIP G is used as it is.  A thread loads its four
// 16-byte pieces of G, V and W (twelve loads in flight), then stores V and W.
template <bool CLIP>
__global__ void __launch_bounds__(256) k_sgd_apply(SegTable T, const float* __restrict__ G, float mu, double clip,
                                                   const double* __restrict__ norm)
{
    float c = 1.0f;
    if (CLIP) {
        const double cc = clip / (norm[0] + 1e-6);
        c = cc < 1.0 ? (float)cc : 1.0f;
    }
    const SegTablePtr Tp = seg_table_arg();
    for (unsigned tile = blockIdx.x; tile < Tp->tile0[kSegs]; tile += gridDim.x) {
        const Seg s = seg_of(Tp, tile);
        const float* g = G + s.goff;
        const unsigned long long base = (unsigned long long)(tile - s.tile0) * kTileFloats;
        f32x4 qg[4], qv[4], qw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long e = base + (unsigned long long)(j * 256 + threadIdx.x) * 4;
            if (e + 3 < s.cnt) {
                qg[j] = *reinterpret_cast<const f32x4*>(g + e);
                qv[j] = *reinterpret_cast<const f32x4*>(s.v + e);
                qw[j] = *reinterpret_cast<const f32x4*>(s.w + e);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long e = base + (unsigned long long)(j * 256 + threadIdx.x) * 4;
            if (e + 3 < s.cnt) {
                f32x4 nv, nw;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float a, b;
                    sgd_element(CLIP ? c * qg[j][i] : qg[j][i], qv[j][i], qw[j][i], s.lr, mu, s.wd, a, b);
                    nv[i] = a;
                    nw[i] = b;
                }
                *reinterpret_cast<f32x4*>(s.v + e) = nv;
                *reinterpret_cast<f32x4*>(s.w + e) = nw;
            } else {
                for (unsigned long long i = e; i < s.cnt; ++i) {  // the last one to three elements of a segment
                    float nv, nw;
                    sgd_element(CLIP ? c * g[i] : g[i], s.v[i], s.w[i], s.lr, mu, s.wd, nv, nw);
                    s.v[i] = nv;
                    s.w[i] = nw;
                }
            }
        }
    }
}

SegTable seg_table(const va_vgg16* m, const va_grad_layout& GL, float lr)
{
    SegTable T{};
    for (int i = 0; i < 13; ++i) {
        T.w[2 * i] = m->conv[i].wp;
        T.v[2 * i] = m->conv[i].mom_w;
        T.w[2 * i + 1] = m->conv[i].bias;
        T.v[2 * i + 1] = m->conv[i].mom_b;
    }
    for (int i = 0; i < 4; ++i) {
        T.w[26 + 2 * i] = m->fcw[i];
        T.v[26 + 2 * i] = m->fc_mom_w[i];
        T.w[27 + 2 * i] = m->fcb[i];
        T.v[27 + 2 * i] = m->fc_mom_b[i];
    }
    unsigned t = 0;
    for (int s = 0; s < kSegs; ++s) {
        T.goff[s] = GL.off[s];
        T.cnt[s] = GL.cnt[s];
        T.tile0[s] = t;
        T.lr[s] = va_solver_lr(m->solver, lr, s & 1);  // odd segments are the biases
        T.wd[s] = va_solver_wd(m->solver, s & 1);
        T.frozen[s] = va_solver_frozen(m->solver, s / 2);
        if (!T.frozen[s]) t += (unsigned)((GL.cnt[s] + kTileFloats - 1) / kTileFloats);
    }
    T.tile0[kSegs] = t;
    return T;
}

}  // namespace

va_grad_layout va_grad_layout_of(const va_vgg16* m)
{
    va_grad_layout GL{};
    size_t off = 0;
    auto take = [&](int s, size_t n) {
        GL.off[s] = off;
        GL.cnt[s] = n;
        off += va_align_up(n, 64);
    };
    for (int i = 0; i < 13; ++i) {
        take(2 * i, (size_t)m->conv[i].cout * 9 * m->conv[i].cin_pad);
        take(2 * i + 1, (size_t)m->conv[i].cout);
    }
    for (int i = 0; i < 4; ++i) {
        take(26 + 2 * i, (size_t)m->fc_out[i] * m->fc_in[i]);
        take(27 + 2 * i, (size_t)m->fc_out[i]);
    }
    GL.total = off;
    return GL;
}

int va_scale_dlogits(float* dlogits, int rows, const va_heads& h, const float* scales, hipStream_t st)
{
    Scales sc{};
    bool all_one = true;
    for (int t = 0; t < VA_MAX_HEADS; ++t) {
        sc.s[t] = t < h.n ? scales[t] : 1.0f;
        all_one = all_one && sc.s[t] == 1.0f;
    }
    if (all_one) return VA_OK;
    const int C = h.off[h.n];
    const size_t n = (size_t)rows * C;
    k_scale_dlogits<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(dlogits, rows, C, h, sc);
    return VA_OK;
}

extern "C" size_t va_vgg16_train_apply_workspace_bytes(void) { return (size_t)(kNormBlocks + 1) * sizeof(double); }

extern "C" int va_vgg16_train_apply(va_vgg16* m, const void* grad, size_t grad_floats, float lr, float momentum, float clip_norm,
                                    void* norm_out, void* workspace, size_t workspace_bytes, void* stream)
{
    const char* who = "va_vgg16_train_apply";
    VA_CHECK_ARG(m != nullptr && grad != nullptr, "%s: NULL argument", who);
    VA_USE_DEVICE(m->ctx);
    VA_CHECK_ARG(m->dtype == VA_DTYPE_F32, "%s: training is fp32 only", who);
    VA_CHECK_ARG(m->conv[0].mom_w != nullptr, "%s: call va_vgg16_train_init first", who);
    VA_CHECK_ARG(((uintptr_t)grad & 15) == 0, "%s: grad must be 16-byte aligned", who);
    VA_CHECK_ARG(lr - lr == 0.0f && momentum - momentum == 0.0f && clip_norm - clip_norm == 0.0f, "%s: lr, momentum and clip_norm must be finite", who);
    const va_grad_layout GL = va_grad_layout_of(m);
    VA_CHECK_ARG(grad_floats >= GL.total, "%s: gradient buffer of %zu floats needed (va_vgg16_train_grad_floats), %zu given", who, GL.total,
                 grad_floats);
    const bool clip = clip_norm > 0.0f, want_norm = clip || norm_out != nullptr;
    if (want_norm && (workspace == nullptr || ((uintptr_t)workspace & 7) != 0 || workspace_bytes < va_vgg16_train_apply_workspace_bytes())) {
        va_set_error("%s: an 8-byte aligned workspace of %zu bytes needed, %zu given", who, va_vgg16_train_apply_workspace_bytes(), workspace_bytes);
        return VA_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const SegTable T = seg_table(m, GL, lr);
    const float* G = (const float*)grad;
    double* part = (double*)workspace;
    double* norm = want_norm ? part + kNormBlocks : nullptr;
    if (want_norm) {
        k_grad_sumsq_partial<<<kNormBlocks, 256, 0, st>>>(T, G, part);
        k_grad_norm_finish<<<1, 256, 0, st>>>(part, kNormBlocks, norm, (double*)norm_out);
    }
    const unsigned blocks = T.tile0[kSegs] < (unsigned)kApplyBlocks ? T.tile0[kSegs] : (unsigned)kApplyBlocks;
    if (clip) k_sgd_apply<true><<<blocks, 256, 0, st>>>(T, G, momentum, (double)clip_norm, norm);
    else k_sgd_apply<false><<<blocks, 256, 0, st>>>(T, G, momentum, 0.0, nullptr);
    VA_LAUNCH_CHECK();
    return VA_OK;
}
