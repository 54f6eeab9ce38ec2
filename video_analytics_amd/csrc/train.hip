// Training step of the two-stream VGG-16 on gfx950: the body of the batch loop of
// SpatialNetwork.train() / TemporalNetwork.train() (Sheet03/spatialModel.py:165-182, Sheet03/temporalModel.py:194-211):
// forward in train mode (Dropout p = 0.5 after the three hidden classifier ReLUs), mean cross-entropy, backward
// through the whole network, momentum-SGD update (torch.optim.SGD: buf = momentum*buf + grad; w -= lr*buf; no
// weight decay, no Nesterov -- Sheet03/spatialModel.py:116) of every parameter.  fp32 throughout.  The model's solver
// (va_vgg16_set_solver) adds what both papers train with: L2 weight decay, the ratio of each Dropout layer
// and frozen layers; its defaults are the step just described, bit for bit.
//
// Convolution backward reuses the forward implicit-GEMM kernel for the data gradient (a 3x3 convolution of the
// output gradient with the flipped, transposed weights) and adds one MFMA kernel for the weight gradient
// (dW[co][tap][ci] = sum over pixels of dY[p][co] * X[p + tap][ci]: a GEMM whose K dimension is the pixels,
// split over workgroups and reduced in a fixed order together with the SGD update).
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <type_traits>
#include "vgg_internal.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));


// ---------------------------------------------------------------- small kernels ----------------

// NHWC 2x2/2 max-pool, 4 channels per thread
__global__ void k_maxpool(const float* __restrict__ y, float* __restrict__ p, int B, int H, int C)
{
    const int Ho = H >> 1, C4 = C >> 2;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * Ho * Ho * C4) return;
    const int c4 = (int)(idx % C4);
    size_t r = idx / C4;
    const int xo = (int)(r % Ho);
    r /= Ho;
    const int yo = (int)(r % Ho), b = (int)(r / Ho);
    const f32x4* src = reinterpret_cast<const f32x4*>(y) + (((size_t)b * H + 2 * yo) * H + 2 * xo) * C4 + c4;
    const f32x4 a0 = src[0], a1 = src[C4], a2 = src[(size_t)H * C4], a3 = src[(size_t)H * C4 + C4];
    f32x4 m;
#pragma unroll
    for (int j = 0; j < 4; ++j)  // IEEE maximum, as max_pool2d: a NaN in the window gives NaN (fmaxf would skip it)
        m[j] = __builtin_elementwise_maximum(__builtin_elementwise_maximum(a0[j], a1[j]), __builtin_elementwise_maximum(a2[j], a3[j]));
    reinterpret_cast<f32x4*>(p)[idx] = m;
}

// Max-pool backward (torch semantics: the gradient goes to the FIRST maximum of the window in row-major order)
// fused with the ReLU mask of the pooled value: dY = (Y == P at the first such position && P > 0) ? dP : 0.
__global__ void k_unpool(const float* __restrict__ dp, const float* __restrict__ y, const float* __restrict__ p,
                         float* __restrict__ dy, int B, int H, int C)
{
    const int Ho = H >> 1, C4 = C >> 2;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * Ho * Ho * C4) return;
    const int c4 = (int)(idx % C4);
    size_t r = idx / C4;
    const int xo = (int)(r % Ho);
    r /= Ho;
    const int yo = (int)(r % Ho), b = (int)(r / Ho);
    const size_t o00 = (((size_t)b * H + 2 * yo) * H + 2 * xo) * C4 + c4;
    const size_t off[4] = {o00, o00 + C4, o00 + (size_t)H * C4, o00 + (size_t)H * C4 + C4};
    const f32x4 pv = reinterpret_cast<const f32x4*>(p)[idx], g = reinterpret_cast<const f32x4*>(dp)[idx];
    f32x4 a[4], out[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = reinterpret_cast<const f32x4*>(y)[off[q]];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bool taken = !(pv[j] > 0.0f);  // ReLU mask: nothing flows where the pooled activation is 0
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool hit = !taken && a[q][j] == pv[j];
            out[q][j] = hit ? g[j] : 0.0f;
            taken = taken || hit;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) reinterpret_cast<f32x4*>(dy)[off[q]] = out[q];
}

__device__ __forceinline__ unsigned mix32(unsigned x)
{
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

// Dropout(p) in place: element i is kept (and multiplied by s = 1 / (1 - p)) iff the top 24 bits of h = mix(mix(i ^ key) + key2)
// reach T = ceil(p * 2^24), i.e. iff synth.hash_uniform(seed, stream)[i] = (h >> 8) / 2^24 >= p (the host derives key/key2 from
// (seed, stream), and T and s from p: dropout_layer).  p = 0.5: T = 2^23, the top bit of h, and s = 2.  A product with the
// 0 / s mask, as nn.Dropout's: a dropped negative element becomes -0, a dropped NaN stays NaN (the step's inputs are >= 0).
__global__ void k_dropout(float* __restrict__ x, size_t n, unsigned key, unsigned key2, unsigned T, float s)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned h = mix32(mix32((unsigned)i ^ key) + key2);
    x[i] = x[i] * ((h >> 8) >= T ? s : 0.0f);
}

// logits [B][C], labels i64 -> dlogits = (softmax - onehot) / B; out[0] = mean CE, out[1] = #(argmax == label)
__global__ void k_ce_fwd_bwd(const float* __restrict__ logits, const long long* __restrict__ labels, int B, int C,
                             float* __restrict__ dlogits, float* __restrict__ out)
{
    __shared__ float sloss[256];
    __shared__ int scorr[256];
    float loss = 0.0f;
    int corr = 0;
    const float invB = 1.0f / (float)B;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float* l = logits + (size_t)b * C;
        float mx = l[0];
        int am = 0;
        for (int c = 1; c < C; ++c)
            if (l[c] > mx) { mx = l[c]; am = c; }
        float se = 0.0f;
        for (int c = 0; c < C; ++c) se += expf(l[c] - mx);
        // label outside [0, C): no out-of-bounds read; loss and this row's gradient become NaN (nn.CrossEntropyLoss
        // refuses such a target; the Python wrapper raises ValueError first when the labels are on the host)
        const long long y = labels[b];
        const bool yok = y >= 0 && y < (long long)C;
        loss += yok ? (logf(se) + mx) - l[yok ? y : 0] : __builtin_nanf("");
        corr += (yok && am == (int)y);
        const float inv = yok ? 1.0f / se : __builtin_nanf("");
        for (int c = 0; c < C; ++c) dlogits[(size_t)b * C + c] = (expf(l[c] - mx) * inv - (c == (int)y ? 1.0f : 0.0f)) * invB;
    }
    sloss[threadIdx.x] = loss;
    scorr[threadIdx.x] = corr;
    __syncthreads();
    if (threadIdx.x == 0) {
        float L = 0.0f;
        int Cc = 0;
        for (int i = 0; i < (int)blockDim.x; ++i) { L += sloss[i]; Cc += scorr[i]; }
        out[0] = L * invB;
        out[1] = (float)Cc;
    }
}

// Consensus loss (TSN's segmental consensus, Sheet03/notes.txt:165-185): logits z[B][K][C] of B videos of K
// snippets each, labels i64 [B].  m[v][c] = (((z[v][0][c] + z[v][1][c]) + ...) + z[v][K-1][c]) / (float)K (consensus mode 1's
// mean, va_score_consensus); loss, hits and g[v][c] are k_ce_fwd_bwd's expressions on m with B videos, and every snippet
// receives dz[v][j][c] = g[v][c] / (float)K.  Row 0 of a video's K gradient rows holds m until the gradient replaces it
// element by element, so no workspace is added.  K = 1: every added operation is a division by 1 -- k_ce_fwd_bwd's bits.
__global__ void k_ce_consensus_fwd_bwd(const float* __restrict__ logits, const long long* __restrict__ labels, int B, int K, int C,
                                       float* __restrict__ dlogits, float* __restrict__ out)
{
    __shared__ float sloss[256];
    __shared__ int scorr[256];
    float loss = 0.0f;
    int corr = 0;
    const float invB = 1.0f / (float)B;
    const float fk = (float)K;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float* z = logits + (size_t)b * K * C;
        float* l = dlogits + (size_t)b * K * C;
        for (int c = 0; c < C; ++c) {
            float s = z[c];
            for (int j = 1; j < K; ++j) s += z[(size_t)j * C + c];
            l[c] = s / fk;
        }
        float mx = l[0];
        int am = 0;
        for (int c = 1; c < C; ++c)
            if (l[c] > mx) { mx = l[c]; am = c; }
        float se = 0.0f;
        for (int c = 0; c < C; ++c) se += expf(l[c] - mx);
        const long long y = labels[b];  // outside [0, C): NaN loss and NaN gradient rows, as k_ce_fwd_bwd
        const bool yok = y >= 0 && y < (long long)C;
        loss += yok ? (logf(se) + mx) - l[yok ? y : 0] : __builtin_nanf("");
        corr += (yok && am == (int)y);
        const float inv = yok ? 1.0f / se : __builtin_nanf("");
        for (int c = 0; c < C; ++c) {
            const float g = (expf(l[c] - mx) * inv - (c == (int)y ? 1.0f : 0.0f)) * invB;
            const float gk = g / fk;
            for (int j = 0; j < K; ++j) l[(size_t)j * C + c] = gk;
        }
    }
    sloss[threadIdx.x] = loss;
    scorr[threadIdx.x] = corr;
    __syncthreads();
    if (threadIdx.x == 0) {
        float L = 0.0f;
        int Cc = 0;
        for (int i = 0; i < (int)blockDim.x; ++i) { L += sloss[i]; Cc += scorr[i]; }
        out[0] = L * invB;
        out[1] = (float)Cc;
    }
}

// ---------------------------------------------------------------- the finishing statement -----

// What the four kernels that complete a gradient element g do with it.  UPD_SGD: the fused momentum-SGD
// update of va_vgg16_train_step, V = mu*V + g; W -= lr*V, and with weight decay (wd is the tensor's wd_t,
// uniform over the launch) V = mu*V + (wd*W + g): torch.optim.SGD's order, one more fused multiply-add on the W that is
// read anyway.  wd == 0 is a path of its own, not fmaf(0, W, g): an infinite weight keeps its result.  UPD_STORE / UPD_ADD
// (va_vgg16_train_accumulate): `v` is the element's place in the caller's gradient buffer, G = g or G = G + g (one
// rounding); `w` is not touched.
enum { UPD_SGD = 0, UPD_STORE = 1, UPD_ADD = 2 };

template <int MODE>
__device__ __forceinline__ void finish_grad(float g, size_t idx, float* __restrict__ w, float* __restrict__ v, float lr, float mu,
                                            float wd)
{
    if (MODE == UPD_SGD) {
        if (wd == 0.0f) {
            const float nv = fmaf(mu, v[idx], g);
            v[idx] = nv;
            w[idx] = fmaf(-lr, nv, w[idx]);
        } else {
            const float wv = w[idx];
            const float nv = fmaf(mu, v[idx], fmaf(wd, wv, g));
            v[idx] = nv;
            w[idx] = fmaf(-lr, nv, wv);
        }
    } else if (MODE == UPD_STORE) {
        v[idx] = g;
    } else {
        v[idx] = v[idx] + g;
    }
}

// ---------------------------------------------------------------- classifier backward ----------

// dX[b][i] = sum_o dZ[b][o] * W[o][i], then * scale where mask[b][i] > 0, else 0 (mask may be NULL).
// A workgroup owns 64 columns i; its four 64-thread groups take the output rows o = 4q + g of every 64-row chunk
// and keep all BMAX batch rows in registers (dZ staged in LDS as [o][b]); the four partial sums are added in
// the fixed order g = 0..3 (deterministic).  25088 / 64 = 392 workgroups for FC1.
template <int BMAX>
__global__ void __launch_bounds__(256) k_fc_dx(const float* __restrict__ dz, const float* __restrict__ w, float* __restrict__ dx,
                                               int B, int O, int I, const float* __restrict__ mask, float scale)
{
    constexpr int OC = 64;
    __shared__ __attribute__((aligned(16))) float sdz[OC][BMAX];
    __shared__ float spart[3][BMAX][64];
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + col;
    float acc[BMAX];
#pragma unroll
    for (int b = 0; b < BMAX; ++b) acc[b] = 0.0f;
    for (int o0 = 0; o0 < O; o0 += OC) {
        __syncthreads();
        for (int t = threadIdx.x; t < OC * BMAX; t += 256) {
            const int oo = t / BMAX, b = t - oo * BMAX;
            sdz[oo][b] = (b < B && o0 + oo < O) ? dz[(size_t)b * O + o0 + oo] : 0.0f;
        }
        __syncthreads();
        if (i < I) {
            const int on = O - o0 < OC ? O - o0 : OC;
#pragma unroll 4
            for (int oo = grp; oo < on; oo += 4) {
                const float wv = w[(size_t)(o0 + oo) * I + i];
#pragma unroll
                for (int b4 = 0; b4 < BMAX / 4; ++b4) {
                    const f32x4 d = *reinterpret_cast<const f32x4*>(&sdz[oo][4 * b4]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[4 * b4 + j] = fmaf(d[j], wv, acc[4 * b4 + j]);
                }
            }
        }
    }
    if (grp > 0) {
#pragma unroll
        for (int b = 0; b < BMAX; ++b) spart[grp - 1][b][col] = acc[b];
    }
    __syncthreads();
    if (grp != 0 || i >= I) return;
#pragma unroll
    for (int b = 0; b < BMAX; ++b)
        if (b < B) {
            float v = ((acc[b] + spart[0][b][col]) + spart[1][b][col]) + spart[2][b][col];
            if (mask) v = mask[(size_t)b * I + i] > 0.0f ? v * scale : 0.0f;
            dx[(size_t)b * I + i] = v;
        }
}

// g[o][i] = sum_b dZ[b][o] * X[b][i] (b ascending); V = mu*V + g; W -= lr*V.  One thread per column i keeps X[:, i]
// in registers and walks a slice of the output rows; blockIdx.y selects the slice.  MODE: finish_grad.
template <int BMAX, int MODE>
__global__ void __launch_bounds__(256) k_fc_wgrad_sgd(const float* __restrict__ dz, const float* __restrict__ x, float* __restrict__ w,
                                                      float* __restrict__ v, int B, int O, int I, int orows, float lr, float mu, float wd)
{
    extern __shared__ __attribute__((aligned(16))) float sdz[];  // [orows][BMAX]
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int o0 = blockIdx.y * orows;
    const int on = O - o0 < orows ? O - o0 : orows;
    for (int t = threadIdx.x; t < orows * BMAX; t += 256) {
        const int oo = t / BMAX, b = t - oo * BMAX;
        sdz[t] = (b < B && oo < on) ? dz[(size_t)b * O + o0 + oo] : 0.0f;
    }
    __syncthreads();
    if (i >= I) return;
    float xr[BMAX];
#pragma unroll
    for (int b = 0; b < BMAX; ++b) xr[b] = b < B ? x[(size_t)b * I + i] : 0.0f;
    for (int oo = 0; oo < on; ++oo) {
        float g = 0.0f;
#pragma unroll
        for (int b4 = 0; b4 < BMAX / 4; ++b4) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(&sdz[oo * BMAX + 4 * b4]);
#pragma unroll
            for (int j = 0; j < 4; ++j) g = fmaf(d[j], xr[4 * b4 + j], g);
        }
        finish_grad<MODE>(g, (size_t)(o0 + oo) * I + i, w, v, lr, mu, wd);
    }
}

// bias: g[o] = sum_b dZ[b][o]; momentum-SGD (MODE: finish_grad)
template <int MODE>
__global__ void k_fc_bgrad_sgd(const float* __restrict__ dz, float* __restrict__ bias, float* __restrict__ vb, int B, int O, float lr, float mu,
                               float wd)
{
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= O) return;
    float g = 0.0f;
    for (int b = 0; b < B; ++b) g += dz[(size_t)b * O + o];
    finish_grad<MODE>(g, (size_t)o, bias, vb, lr, mu, wd);
}

// ---------------------------------------------------------------- convolution backward ---------

// data-gradient weights: wt[ci][kp][co] = wp[co][8 - kp][ci]   (ci < cin: the real input channels)
__global__ void k_pack_dgrad_w(const float* __restrict__ wp, float* __restrict__ wt, int Cout, int cin_pad, int Cin)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Cin * 9 * Cout) return;
    const int co = (int)(idx % Cout);
    const int kp = (int)((idx / Cout) % 9);
    const int ci = (int)(idx / ((size_t)Cout * 9));
    wt[idx] = wp[((size_t)co * 9 + (8 - kp)) * cin_pad + ci];
}

struct WgradArgs {
    const float* dy;  // NHWC [B][H][W][Cout] (the gradient at the layer's pre-pool, post-ReLU output, ReLU mask applied)
    const float* x;   // NHWC [B][H][W][cin_pad] (the layer's input)
    float* slab;      // [S][Mpad][Npad]
    int B, H, Cout, cin_pad;
    int N, Npad, Mpad;  // N = 9*cin_pad
    long P;             // pixels = B*H*H
    int chunk;          // pixels per split (multiple of 16)
};

// (WM*64) output channels x (WN*64) (tap, input channel) columns per workgroup of WM*WN = 4 waves (64 x 64 per wave:
// 128 x 128, or 64 x 256 for the 64-channel layers), K = a run of `chunk` pixels, 16 per step.  LDS tiles are
// pixel-major ([k][m], [k][n], row stride = width + 32 floats: the two k rows of an MFMA fragment read fall in
// different bank halves), operands one float per lane for v_mfma_f32_32x32x2_f32.
template <int WM, int WN>
__global__ void __launch_bounds__(WM * WN * 64) k_conv_wgrad(WgradArgs a)
{
    constexpr int BK = 16, BM = WM * 64, BN = WN * 64, LSA = BM + 32, LSB = BN + 32, NT = WM * WN * 64;
    static_assert(NT % (BM / 4) == 0 && NT % (BN / 4) == 0, "a loader thread keeps one float4 column over its passes");
    constexpr int RA = NT / (BM / 4), RB = NT / (BN / 4);        // pixel rows one pass of the loader threads covers
    constexpr int A_PER = (BK + RA - 1) / RA, B_PER = (BK + RB - 1) / RB;  // float4 loads per thread and step (the last pass may be partial)
    __shared__ __attribute__((aligned(16))) float sA[2][BK * LSA], sB[2][BK * LSB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const long p0 = (long)blockIdx.z * a.chunk;
    const long p1 = p0 + a.chunk < a.P ? p0 + a.chunk : a.P;
    const int H = a.H, Cout = a.Cout, cpad = a.cin_pad;

    // loader roles: one float4 column per thread (fixed over the passes), pixel rows krow + R * i
    const int ca4 = (tid % (BM / 4)) * 4, krowa = tid / (BM / 4);
    const int cb4 = (tid % (BN / 4)) * 4, krowb = tid / (BN / 4);
    const bool mok = m0 + ca4 < Cout;
    const int n = n0 + cb4;
    const bool nok = n < a.N;
    const int kp = nok ? n / cpad : 0, ci = nok ? n - kp * cpad : 0;
    const int ky = kp / 3 - 1, kx = kp % 3 - 1;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    f32x4 ra[A_PER], rb[B_PER];
    auto gload = [&](long pbase) {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const long p = pbase + krowa + RA * i;
            ra[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (BK % RA != 0 && krowa + RA * i >= BK) continue;
            if (p < p1 && mok) ra[i] = *reinterpret_cast<const f32x4*>(a.dy + p * Cout + m0 + ca4);
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const long p = pbase + krowb + RB * i;
            rb[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (BK % RB != 0 && krowb + RB * i >= BK) continue;
            if (p < p1 && nok) {
                const int x = (int)(p % H);
                const long r = p / H;
                const int y = (int)(r % H);
                const int yy = y + ky, xx = x + kx;
                if (yy >= 0 && yy < H && xx >= 0 && xx < H) rb[i] = *reinterpret_cast<const f32x4*>(a.x + (p + (long)ky * H + kx) * cpad + ci);
            }
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_PER; ++i)
            if (BK % RA == 0 || krowa + RA * i < BK) *reinterpret_cast<f32x4*>(&sA[buf][(krowa + RA * i) * LSA + ca4]) = ra[i];
#pragma unroll
        for (int i = 0; i < B_PER; ++i)
            if (BK % RB == 0 || krowb + RB * i < BK) *reinterpret_cast<f32x4*>(&sB[buf][(krowb + RB * i) * LSB + cb4]) = rb[i];
    };

    const int r31 = lane & 31, hh = lane >> 5;
    const long steps = (p1 - p0 + BK - 1) / BK;
    if (steps > 0) {
        gload(p0);
        lstore(0);
    }
    __syncthreads();
    for (long t = 0; t < steps; ++t) {
        const int buf = (int)(t & 1);
        if (t + 1 < steps) gload(p0 + (t + 1) * BK);
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks) {
            float fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = sA[buf][(2 * ks + hh) * LSA + (wm * 2 + i) * 32 + r31];
                fb[i] = sB[buf][(2 * ks + hh) * LSB + (wn * 2 + i) * 32 + r31];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < steps) lstore(buf ^ 1);
        __syncthreads();
    }

    // slab[s][m][n]: accumulator register r of lane (r31, hh) is row 8*(r/4) + 4*hh + (r%4), column r31
    float* slab = a.slab + (size_t)blockIdx.z * a.Mpad * a.Npad;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int nn = n0 + (wn * 2 + j) * 32 + r31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int mm = m0 + (wm * 2 + i) * 32 + 8 * (r >> 2) + 4 * hh + (r & 3);
                slab[(size_t)mm * a.Npad + nn] = acc[i][j][r];
            }
        }
}

// g = sum over the S slabs in a FIXED order; V = mu*V + g; W -= lr*V   (W, V: [M][N] = the packed conv weight layout).
// A block = 32 weights x 8 groups of consecutive slabs: a thread adds its group's slabs (four interleaved partial sums, so
// that four loads are in flight; combined as (a0 + a1) + (a2 + a3)), the eight group sums are added ascending.  One thread
// per weight walking all S slabs (round 1) was a chain of S dependent-latency loads on 9 216 ... 36 864 threads: 804 us
// for the first layer's 256 slabs, 267 us for conv1_2's.  MODE: finish_grad.
template <int MODE>
__global__ void __launch_bounds__(256) k_wgrad_reduce_sgd(const float* __restrict__ slab, float* __restrict__ w, float* __restrict__ v,
                                                          int M, int N, int Mpad, int Npad, int S, float lr, float mu, float wd)
{
    __shared__ float part[8][32];
    const int o = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const size_t idx = (size_t)blockIdx.x * 32 + o;
    const bool ok = idx < (size_t)M * N;
    float acc = 0.0f;
    if (ok) {
        const int n = (int)(idx % N), m = (int)(idx / N);
        const int sg = (S + 7) / 8, s0 = grp * sg, s1 = s0 + sg < S ? s0 + sg : S;
        const size_t stride = (size_t)Mpad * Npad;
        const float* p = slab + ((size_t)s0 * Mpad + m) * Npad + n;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        int t = s0;
        for (; t + 3 < s1; t += 4) {
            a0 += p[0];
            a1 += p[stride];
            a2 += p[2 * stride];
            a3 += p[3 * stride];
            p += 4 * stride;
        }
        for (; t < s1; ++t) {
            a0 += p[0];
            p += stride;
        }
        acc = (a0 + a1) + (a2 + a3);
    }
    part[grp][o] = acc;
    __syncthreads();
    if (grp == 0 && ok) {
        float g = part[0][o];
#pragma unroll
        for (int k = 1; k < 8; ++k) g += part[k][o];
        finish_grad<MODE>(g, idx, w, v, lr, mu, wd);
    }
}

// bias gradient, pass 1: part[blk][co] = sum of dy[p][co] over the block's pixel range.  256 threads = (256 / cw)
// pixel rows x cw channels per pass over the channels; four independent partial sums per thread keep four loads
// in flight; the combination order is fixed (deterministic).
__global__ void __launch_bounds__(256) k_conv_bgrad_partial(const float* __restrict__ dy, float* __restrict__ part, long P, int Cout, long chunk)
{
    __shared__ float red[256];
    const long p0 = (long)blockIdx.x * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
    for (int c0 = 0; c0 < Cout; c0 += 256) {
        const int cw = Cout - c0 < 256 ? Cout - c0 : 256;
        const int rows = 256 / cw;
        const int c = threadIdx.x % cw, r = threadIdx.x / cw;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
        if (r < rows) {
            long p = p0 + r;
            for (; p + 3L * rows < p1; p += 4L * rows) {
                s0 += dy[p * Cout + c0 + c];
                s1 += dy[(p + rows) * Cout + c0 + c];
                s2 += dy[(p + 2L * rows) * Cout + c0 + c];
                s3 += dy[(p + 3L * rows) * Cout + c0 + c];
            }
            for (; p < p1; p += rows) s0 += dy[p * Cout + c0 + c];
        }
        float s = (s0 + s1) + (s2 + s3);
        red[threadIdx.x] = s;
        __syncthreads();
        if (r == 0) {
            for (int q = 1; q < rows; ++q) s += red[q * cw + c];
            part[(size_t)blockIdx.x * Cout + c0 + c] = s;
        }
        __syncthreads();
    }
}

// pass 2 + momentum SGD (MODE: finish_grad): 64 channels per workgroup, four 64-thread groups each add a quarter of the partials
template <int MODE>
__global__ void __launch_bounds__(256) k_conv_bgrad_sgd(const float* __restrict__ part, int nblk, float* __restrict__ bias, float* __restrict__ vb,
                                                        int Cout, float lr, float mu, float wd)
{
    __shared__ float red[3][64];
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + col;
    float g = 0.0f;
    if (c < Cout)
        for (int i = grp; i < nblk; i += 4) g += part[(size_t)i * Cout + c];
    if (grp > 0) red[grp - 1][col] = g;
    __syncthreads();
    if (grp != 0 || c >= Cout) return;
    g = ((g + red[0][col]) + red[1][col]) + red[2][col];
    finish_grad<MODE>(g, (size_t)c, bias, vb, lr, mu, wd);
}

// ---------------------------------------------------------------- export / import --------------

// packed conv [Cout][9][cpad] -> OIHW [Cout][Cin][3][3]
__global__ void k_unpack_conv_w(const float* __restrict__ wp, float* __restrict__ w, int Cout, int Cin, int cpad)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Cout * Cin * 9) return;
    const int kp = (int)(idx % 9);
    const int ci = (int)((idx / 9) % Cin);
    const int co = (int)(idx / ((size_t)Cin * 9));
    w[idx] = wp[((size_t)co * 9 + kp) * cpad + ci];
}
__global__ void k_repack_conv_w(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin, int cpad)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Cout * 9 * cpad) return;
    const int ci = (int)(idx % cpad);
    const int kp = (int)((idx / cpad) % 9);
    const int co = (int)(idx / ((size_t)cpad * 9));
    wp[idx] = ci < Cin ? w[((size_t)co * Cin + ci) * 9 + kp] : 0.0f;
}
// FC1: [out][p*C + c] <-> [out][c*HW + p]
__global__ void k_unpack_fc1(const float* __restrict__ wp, float* __restrict__ w, int O, int C, int HW)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)O * C * HW) return;
    const int p = (int)(idx % HW);
    const int c = (int)((idx / HW) % C);
    const size_t o = idx / ((size_t)C * HW);
    w[idx] = wp[(o * HW + p) * C + c];
}
__global__ void k_repack_fc1(const float* __restrict__ w, float* __restrict__ wp, int O, int C, int HW)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)O * C * HW) return;
    const int c = (int)(idx % C);
    const int p = (int)((idx / C) % HW);
    const size_t o = idx / ((size_t)C * HW);
    wp[idx] = w[(o * C + c) * HW + p];
}

// ---------------------------------------------------------------- host side --------------------

struct WgradPlan {
    int BM, BN, Mpad, Npad, S, chunk;
    size_t slab_floats;
};

WgradPlan plan_wgrad(int B, int hw, int cout, int cin_pad)
{
    WgradPlan p;
    const int N = 9 * cin_pad;
    p.BM = cout <= 64 ? 64 : 128;  // 64 x 192 tiles (three waves) for the 64-channel layers, 128 x 128 otherwise:
    p.BN = cout <= 64 ? 192 : 128;  // conv1_2's 576 columns are three tiles (256-column tiles: 2.25), the first layer's 144 one
    p.Mpad = va_cdiv(cout, p.BM) * p.BM;
    p.Npad = va_cdiv(N, p.BN) * p.BN;
    const long P = (long)B * hw * hw;
    const int tiles = (p.Mpad / p.BM) * (p.Npad / p.BN);
    long S = va_cdiv(2048, tiles);  // aim for ~2048 workgroups
    const long maxS = P / 256 > 0 ? P / 256 : 1;
    if (S > maxS) S = maxS;
    if (S < 1) S = 1;
    long chunk = (P + S - 1) / S;
    chunk = (chunk + 15) / 16 * 16;
    p.chunk = (int)chunk;
    p.S = (int)((P + chunk - 1) / chunk);
    p.slab_floats = (size_t)p.S * p.Mpad * p.Npad;
    return p;
}

struct TrainPlan {
    size_t x0, y[13], p[13], a_d[3], logits, dlogits, dd[3], da0, g[2], wt, slab, bpart, total;
};

constexpr int kBgradBlocks = 1024;

TrainPlan plan_train(const va_vgg16* m, int B)
{
    TrainPlan t{};
    size_t off = 0;
    auto take = [&](size_t floats) {
        const size_t o = off;
        off += va_align_up(floats * sizeof(float), 256);
        return o;
    };
    t.x0 = take((size_t)B * 224 * 224 * m->c_in_pad);
    size_t slab = 0;
    for (int i = 0; i < 13; ++i) {
        const ConvLayer& L = m->conv[i];
        t.y[i] = take((size_t)B * L.hw * L.hw * L.cout);
        t.p[i] = L.pool ? take((size_t)B * (L.hw / 2) * (L.hw / 2) * L.cout) : 0;
        const WgradPlan w = plan_wgrad(B, L.hw, L.cout, L.cin_pad);
        if (w.slab_floats > slab) slab = w.slab_floats;
    }
    for (int i = 0; i < 4; ++i) {
        const size_t s = va_fc_slab_floats(B, m->fc_out[i], m->fc_in[i]);
        if (s > slab) slab = s;
    }
    t.a_d[0] = take((size_t)B * 4096);
    t.a_d[1] = take((size_t)B * 4096);
    t.a_d[2] = take((size_t)B * m->desc_dim);
    t.logits = take((size_t)B * m->n_classes);
    t.dlogits = take((size_t)B * m->n_classes);
    t.dd[0] = take((size_t)B * 4096);
    t.dd[1] = take((size_t)B * 4096);
    t.dd[2] = take((size_t)B * m->desc_dim);
    t.da0 = take((size_t)B * 512 * 49);
    t.g[0] = take((size_t)B * 224 * 224 * 64);
    t.g[1] = take((size_t)B * 224 * 224 * 64);
    t.wt = take((size_t)512 * 9 * 512);
    t.slab = take(slab);
    t.bpart = take((size_t)kBgradBlocks * 512);
    t.total = off;
    return t;
}

void keys_for(unsigned long long seed, unsigned stream, unsigned& key, unsigned& key2)
{
    auto mix = [](unsigned x) {
        x ^= x >> 16;
        x *= 0x7FEB352Du;
        x ^= x >> 15;
        x *= 0x846CA68Bu;
        x ^= x >> 16;
        return x;
    };
    key = mix((unsigned)(seed * 0x9E3779B1ull + (unsigned long long)stream * 0x85EBCA77ull + 0x1234567ull));
    key2 = mix(key + 0x68E31DA4u);
}

template <typename F>
int fc_backward_dispatch(int B, F&& f)
{
    if (B <= 32) return f(std::integral_constant<int, 32>());
    return f(std::integral_constant<int, 64>());
}

template <typename F>
int update_dispatch(int mode, F&& f)
{
    if (mode == UPD_STORE) return f(std::integral_constant<int, UPD_STORE>());
    if (mode == UPD_ADD) return f(std::integral_constant<int, UPD_ADD>());
    return f(std::integral_constant<int, UPD_SGD>());
}

// ---- the per-layer bodies of the step: train_step and the testing entry points (va_train_*) call these ----

void pool_forward(const float* y, float* p, int B, int hw, int C, hipStream_t st)
{
    const size_t n = (size_t)B * (hw / 2) * (hw / 2) * (C / 4);
    k_maxpool<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(y, p, B, hw, C);
}

void pool_backward(const float* dp, const float* y, const float* p, float* dy, int B, int hw, int C, hipStream_t st)
{
    const size_t n = (size_t)B * (hw / 2) * (hw / 2) * (C / 4);
    k_unpool<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(dp, y, p, dy, B, hw, C);
}

// s = 1 / (1 - p) in float32, the factor of a kept element (p in [0, 1): 1 - p is exact for p >= 0.5 and never 0)
float dropout_scale(float p) { return 1.0f / (1.0f - p); }

// Dropout with ratio p in [0, 1): T = ceil(p * 2^24) (p * 2^24 is exact in double), kept iff (h >> 8) >= T.  p = 0: no launch.
void dropout_layer(float* x, size_t n, unsigned long long seed, int layer, float p, hipStream_t st)
{
    if (p == 0.0f) return;
    unsigned key, key2;
    keys_for(seed, 100u + (unsigned)layer, key, key2);
    const unsigned T = (unsigned)ceil((double)p * 16777216.0);
    k_dropout<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(x, n, key, key2, T, dropout_scale(p));
}

// lr_t and wd_t of a layer's two tensors (include/va.h, "Update of one tensor") and the momentum
struct Upd {
    float lr, lr_b, mu, wd, wd_b;
};
Upd plain_update(float lr, float mu) { return Upd{lr, lr, mu, 0.0f, 0.0f}; }
Upd solver_update(const va_solver& s, float lr, float mu)
{
    return Upd{va_solver_lr(s, lr, false), va_solver_lr(s, lr, true), mu, va_solver_wd(s, false), va_solver_wd(s, true)};
}

// The heads of the multi-task form of the loss: tasks i32 [videos] on the device
struct MultiTask {
    const int* tasks;
    va_heads heads;
};

// segments = 0: the loss of every row of logits [B][C]; segments = K >= 1: of the consensus of B / K videos; mt != NULL: the
// multi-task consensus loss of B / max(K, 1) videos (k_ce_multitask_fwd_bwd in multitask.hip), every head on its own columns
int loss_layer(const float* logits, const long long* labels, int B, int segments, int C, float* dlogits, float* out, hipStream_t st,
               const MultiTask* mt = nullptr)
{
    if (mt) return va_ce_multitask(logits, labels, mt->tasks, B / (segments > 0 ? segments : 1), segments > 0 ? segments : 1, mt->heads, dlogits, out, st);
    if (segments == 0) k_ce_fwd_bwd<<<1, 256, 0, st>>>(logits, labels, B, C, dlogits, out);
    else k_ce_consensus_fwd_bwd<<<1, 256, 0, st>>>(logits, labels, B / segments, segments, C, dlogits, out);
    return VA_OK;
}

// dx (with mask and scale; dx == NULL: the layer below is frozen, no input gradient), then the weight and bias updates in
// place; *inst (may be NULL): the batch instantiation, 32 or 64.
// mode UPD_STORE / UPD_ADD: vw / vb are the layer's places in the gradient buffer, w is only read (dx), bias not at all.
int fc_backward_layer(int B, int O, int I, const float* dz, const float* x, float* w, float* bias, float* vw, float* vb, float* dx,
                      const float* mask, float scale, const Upd& u, hipStream_t st, int* inst, int mode = UPD_SGD)
{
    return update_dispatch(mode, [&](auto MD) {
        constexpr int md = decltype(MD)::value;
        int rc = fc_backward_dispatch(B, [&](auto BM) {
            constexpr int bm = decltype(BM)::value;
            if (inst) *inst = bm;
            if (dx) k_fc_dx<bm><<<va_cdiv(I, 64), 256, 0, st>>>(dz, w, dx, B, O, I, mask, scale);
            const int orows = 16;
            k_fc_wgrad_sgd<bm, md><<<dim3(va_cdiv(I, 256), va_cdiv(O, orows)), 256, (size_t)orows * bm * sizeof(float), st>>>(
                dz, x, w, vw, B, O, I, orows, u.lr, u.mu, u.wd);
            return VA_OK;
        });
        if (rc) return rc;
        k_fc_bgrad_sgd<md><<<va_cdiv(O, 256), 256, 0, st>>>(dz, bias, vb, B, O, u.lr_b, u.mu, u.wd_b);
        return VA_OK;
    });
}

// bias gradient, pass 1: pixels per block and the number of blocks (at most kBgradBlocks)
long bgrad_chunk(long P) { return (P + kBgradBlocks - 1) / kBgradBlocks; }
int bgrad_blocks(long P) { return (int)((P + bgrad_chunk(P) - 1) / bgrad_chunk(P)); }

// Backward of one conv layer.  dx != NULL: the data gradient first (it needs this step's weights): k_pack_dgrad_w into wt,
// then a linear 3x3 convolution of dy through the forward dispatch, zeroed where mask <= 0 (mask may be NULL).  Then the
// weight and bias gradients with the momentum-SGD update in place (dy stays intact).  mode UPD_STORE / UPD_ADD: vw / vb are
// the layer's places in the gradient buffer, w is only read (dx), bias not at all.
int conv_backward_layer(int B, int hw, int cin, int cin_pad, int cout, const float* dy, const float* x, float* w, float* bias, float* vw,
                        float* vb, float* dx, const float* mask, const float* zeros, int f32_conv, float* wt, float* slab, float* bpart,
                        const Upd& u, hipStream_t st, const char** dgrad_launched = nullptr, int mode = UPD_SGD)
{
    if (dx) {
        const size_t nwt = (size_t)cin * 9 * cout;
        k_pack_dgrad_w<<<(unsigned)((nwt + 255) / 256), 256, 0, st>>>(w, wt, cout, cin_pad, cin);
        if (int rc = va_conv3x3_f32(hw, cout, cin, wt, zeros, dy, dx, mask, 1, 0, B, zeros, f32_conv, st, dgrad_launched)) return rc;
    }
    const WgradPlan wp = plan_wgrad(B, hw, cout, cin_pad);
    WgradArgs a{};
    a.dy = dy;
    a.x = x;
    a.slab = slab;
    a.B = B;
    a.H = hw;
    a.Cout = cout;
    a.cin_pad = cin_pad;
    a.N = 9 * cin_pad;
    a.Npad = wp.Npad;
    a.Mpad = wp.Mpad;
    a.P = (long)B * hw * hw;
    a.chunk = wp.chunk;
    if (wp.BM == 64) k_conv_wgrad<1, 3><<<dim3(wp.Npad / 192, wp.Mpad / 64, wp.S), 192, 0, st>>>(a);
    else k_conv_wgrad<2, 2><<<dim3(wp.Npad / 128, wp.Mpad / 128, wp.S), 256, 0, st>>>(a);
    const size_t nw = (size_t)cout * a.N;
    const int nblk = bgrad_blocks(a.P);
    return update_dispatch(mode, [&](auto MD) {
        constexpr int md = decltype(MD)::value;
        k_wgrad_reduce_sgd<md><<<(unsigned)((nw + 31) / 32), 256, 0, st>>>(slab, w, vw, cout, a.N, wp.Mpad, wp.Npad, wp.S, u.lr, u.mu, u.wd);
        k_conv_bgrad_partial<<<nblk, 256, 0, st>>>(dy, bpart, a.P, cout, bgrad_chunk(a.P));
        k_conv_bgrad_sgd<md><<<va_cdiv(cout, 64), 256, 0, st>>>(bpart, nblk, bias, vb, cout, u.lr_b, u.mu, u.wd_b);
        VA_LAUNCH_CHECK();
        return VA_OK;
    });
}

}  // namespace

extern "C" int va_vgg16_train_init(va_vgg16* m, void* stream)
{
    VA_CHECK_ARG(m != nullptr, "va_vgg16_train_init: model is NULL");
    VA_USE_DEVICE(m->ctx);
    VA_CHECK_ARG(m->dtype == VA_DTYPE_F32, "va_vgg16_train_init: training is fp32 only");
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < 13; ++i) {
        ConvLayer& L = m->conv[i];
        const size_t nw = (size_t)L.cout * 9 * L.cin_pad;
        if (!L.mom_w) VA_HIP(hipMalloc(&L.mom_w, nw * sizeof(float)));
        if (!L.mom_b) VA_HIP(hipMalloc(&L.mom_b, L.cout * sizeof(float)));
        VA_HIP(hipMemsetAsync(L.mom_w, 0, nw * sizeof(float), st));
        VA_HIP(hipMemsetAsync(L.mom_b, 0, L.cout * sizeof(float), st));
    }
    for (int i = 0; i < 4; ++i) {
        const size_t nw = (size_t)m->fc_out[i] * m->fc_in[i];
        if (!m->fc_mom_w[i]) VA_HIP(hipMalloc(&m->fc_mom_w[i], nw * sizeof(float)));
        if (!m->fc_mom_b[i]) VA_HIP(hipMalloc(&m->fc_mom_b[i], m->fc_out[i] * sizeof(float)));
        VA_HIP(hipMemsetAsync(m->fc_mom_w[i], 0, nw * sizeof(float), st));
        VA_HIP(hipMemsetAsync(m->fc_mom_b[i], 0, m->fc_out[i] * sizeof(float), st));
    }
    if (!m->zeros_f32) VA_HIP(hipMalloc(&m->zeros_f32, 512 * sizeof(float)));
    VA_HIP(hipMemsetAsync(m->zeros_f32, 0, 512 * sizeof(float), st));
    return VA_OK;
}

extern "C" size_t va_vgg16_train_workspace_bytes(const va_vgg16* m, int batch)
{
    if (!m || batch < 1 || batch > 64 || m->dtype != VA_DTYPE_F32) return 0;
    return plan_train(m, batch).total;
}

// The step both entry points share.  segments = 0: va_vgg16_train_step, the loss of every image (k_ce_fwd_bwd);
// segments = K >= 1: va_vgg16_train_step_consensus, `batch` = videos * K images, video-major, and the loss of the videos'
// consensus (k_ce_consensus_fwd_bwd); mt != NULL: va_vgg16_train_step_multitask, the consensus loss of every head on its own
// videos and columns (k_ce_multitask_fwd_bwd, loss_out f32 [2 + 2H]).  Everything but that one launch is the same code.
// acc != NULL: va_vgg16_train_accumulate -- the same forward and backward with the gradient stored in, or
// added to, the caller's buffer (va_grad_layout_of) by the finishing kernels' UPD_STORE / UPD_ADD forms; weights and momentum
// buffers are only read, lr and momentum are not used.
struct Accum {
    float* grad;
    int first;            // != 0: G = g (and zeros into the alignment gaps), else G = G + g
    const float* scales;  // HOST, max(heads, 1) entries: dlogits *= scales[head of the column] after the loss launch
};

static int train_step(const char* who, va_vgg16* m, const void* x, int x_is_u8, const void* labels, int batch, int segments, float lr,
                      float momentum, unsigned long long dropout_seed, void* desc, void* loss_out, void* workspace,
                      size_t workspace_bytes, void* stream, const MultiTask* mt = nullptr, const Accum* acc = nullptr)
{
    VA_CHECK_ARG(m != nullptr && x != nullptr && labels != nullptr && loss_out != nullptr, "%s: NULL argument", who);
    VA_USE_DEVICE(m->ctx);
    VA_CHECK_ARG(m->dtype == VA_DTYPE_F32, "%s: training is fp32 only", who);
    VA_CHECK_ARG(batch >= 1 && batch <= 64, "%s: batch %d out of range [1,64]", who, batch);
    VA_CHECK_ARG(m->conv[0].mom_w != nullptr && m->zeros_f32 != nullptr, "%s: call va_vgg16_train_init first", who);
    VA_CHECK_ARG(!x_is_u8 || (m->in_mean && m->in_std), "%s: u8 input needs the model's mean/std", who);
    const TrainPlan T = plan_train(m, batch);
    if (workspace == nullptr || workspace_bytes < T.total) {
        va_set_error("%s: workspace of %zu bytes needed, %zu given", who, T.total, workspace_bytes);
        return VA_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int B = batch;
    const int mode = !acc ? UPD_SGD : acc->first ? UPD_STORE : UPD_ADD;
    const va_solver& sv = m->solver;
    const int nf = sv.frozen_layers;  // layers 0 .. nf-1 (conv 0..12, fc 13..16) take no gradient and no update
    const Upd upd = solver_update(sv, lr, momentum);
    va_grad_layout GL{};
    if (acc) {
        GL = va_grad_layout_of(m);
        if (acc->first)  // the gaps between the segments hold zeros: a sum across ranks or a norm over the whole buffer sees nothing;
            for (int s = 0; s < 34; ++s) {  // so do the segments of frozen tensors, which the backward pass never writes
                const size_t end = s < 33 ? GL.off[s + 1] : GL.total;
                const size_t from = GL.off[s] + (va_solver_frozen(sv, s / 2) ? 0 : GL.cnt[s]);
                if (end > from) VA_HIP(hipMemsetAsync(acc->grad + from, 0, (end - from) * sizeof(float), st));
            }
    }
    char* ws = (char*)workspace;
    auto F = [&](size_t off) { return (float*)(ws + off); };
    float* slab = F(T.slab);

    // ---------------- forward (train mode) ----------------
    if (int rc = va_input_to_nhwc_f32(m, x, x_is_u8, B, F(T.x0), st)) return rc;
    const float* in = F(T.x0);
    for (int i = 0; i < 13; ++i) {
        const ConvLayer& L = m->conv[i];
        if (int rc = va_conv3x3_f32(L.hw, L.cin_pad, L.cout, L.wp, L.bias, in, F(T.y[i]), nullptr, 0, 0, B, m->zeros_f32, m->f32_conv, st)) return rc;
        in = F(T.y[i]);
        if (L.pool) {
            pool_forward(F(T.y[i]), F(T.p[i]), B, L.hw, L.cout, st);
            in = F(T.p[i]);
        }
    }
    VA_LAUNCH_CHECK();
    const float* a0 = F(T.p[12]);  // NHWC flatten [B][7*7*512]; FC1's weights are stored in that order
    const float* fin[4] = {a0, F(T.a_d[0]), F(T.a_d[1]), F(T.a_d[2])};
    float* fout[4] = {F(T.a_d[0]), F(T.a_d[1]), F(T.a_d[2]), F(T.logits)};
    for (int l = 0; l < 4; ++l) {
        if (int rc = va_fc_f32(fin[l], m->fcw[l], m->fcb[l], fout[l], slab, B, m->fc_out[l], m->fc_in[l], l < 3, st)) return rc;
        if (l < 3) dropout_layer(fout[l], (size_t)B * m->fc_out[l], dropout_seed, l, sv.dropout[l], st);
    }
    if (desc) VA_HIP(hipMemcpyAsync(desc, F(T.a_d[2]), (size_t)B * m->desc_dim * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (int rc = loss_layer(F(T.logits), (const long long*)labels, B, segments, m->n_classes, F(T.dlogits), (float*)loss_out, st, mt)) return rc;
    if (acc) {  // a micro-batch's share of the full batch's mean: every head's columns times its scale (nothing when all are 1)
        va_heads one{};
        one.n = 1;
        for (int t = 1; t <= VA_MAX_HEADS; ++t) one.off[t] = m->n_classes;
        if (int rc = va_scale_dlogits(F(T.dlogits), B, mt ? mt->heads : one, acc->scales, st)) return rc;
    }
    VA_LAUNCH_CHECK();

    // ---------------- classifier backward + update ----------------
    // dz_l = gradient at FC l's pre-activation; for l < 3 it arrives through Dropout and ReLU: times the Dropout layer's own
    // s = 1 / (1 - p) where the (post-dropout) activation is positive, 0 elsewhere -- applied by the k_fc_dx that produced it.
    // The loops stop above the last frozen layer, and the first unfrozen one forms no input gradient.
    const float* dz[4] = {F(T.dd[0]), F(T.dd[1]), F(T.dd[2]), F(T.dlogits)};
    float* dxo[4] = {F(T.da0), F(T.dd[0]), F(T.dd[1]), F(T.dd[2])};
    for (int l = 3; l >= 0 && 13 + l >= nf; --l) {
        const int O = m->fc_out[l], I = m->fc_in[l];
        const float* mask = l > 0 ? fin[l] : nullptr;  // fin[l] = post-dropout activation of layer l-1
        const float scale = l > 0 ? dropout_scale(sv.dropout[l - 1]) : 1.0f;
        float* vw = acc ? acc->grad + GL.off[26 + 2 * l] : m->fc_mom_w[l];
        float* vb = acc ? acc->grad + GL.off[27 + 2 * l] : m->fc_mom_b[l];
        if (int rc = fc_backward_layer(B, O, I, dz[l], fin[l], m->fcw[l], m->fcb[l], vw, vb, 13 + l > nf ? dxo[l] : nullptr, mask, scale, upd, st,
                                       nullptr, mode))
            return rc;
    }
    VA_LAUNCH_CHECK();

    // ---------------- feature stack backward + update ----------------
    const int stop_at = m->train_stop_at;  // VA_OPT_TRAIN_STOP_AT (tests): -1 = the whole step
    const float* dout = F(T.da0);  // gradient at layer 12's pooled output
    int cur = -1;                  // which of the two gradient buffers holds `dout` (-1: neither)
    for (int i = 12; i >= nf; --i) {
        ConvLayer& L = m->conv[i];
        const float* lin = i == 0 ? F(T.x0) : (m->conv[i - 1].pool ? F(T.p[i - 1]) : F(T.y[i - 1]));
        const float* dyr = dout;
        if (L.pool) {
            const int dst = cur == 0 ? 1 : 0;
            pool_backward(dout, F(T.y[i]), F(T.p[i]), F(T.g[dst]), B, L.hw, L.cout, st);
            dyr = F(T.g[dst]);
            cur = dst;
        }
        // data gradient (not for the first unfrozen layer) into the other gradient buffer, then the weight and bias updates
        float* g = i > nf ? F(T.g[1 - cur]) : nullptr;
        const float* mask = i > nf && !m->conv[i - 1].pool ? F(T.y[i - 1]) : nullptr;
        float* vw = acc ? acc->grad + GL.off[2 * i] : L.mom_w;
        float* vb = acc ? acc->grad + GL.off[2 * i + 1] : L.mom_b;
        if (int rc = conv_backward_layer(B, L.hw, L.cin, L.cin_pad, L.cout, dyr, lin, L.wp, L.bias, vw, vb, g, mask, m->zeros_f32, m->f32_conv,
                                         F(T.wt), slab, F(T.bpart), upd, st, nullptr, mode))
            return rc;
        if (g) dout = g;
        if (g) cur = 1 - cur;
        if (stop_at == i) {  // debugging aid of the tests: leave the gradient buffers as layer i left them; NOT a completed step
            va_set_error("%s: stopped after the backward pass of conv layer %d (VA_OPT_TRAIN_STOP_AT); layers below were not updated", who, i);
            return VA_ERR_STOPPED;
        }
    }
    return VA_OK;
}

extern "C" int va_vgg16_train_step(va_vgg16* m, const void* x, int x_is_u8, const void* labels, int batch, float lr, float momentum,
                                   unsigned long long dropout_seed, void* desc, void* loss_out, void* workspace, size_t workspace_bytes,
                                   void* stream)
{
    return train_step("va_vgg16_train_step", m, x, x_is_u8, labels, batch, 0, lr, momentum, dropout_seed, desc, loss_out, workspace,
                      workspace_bytes, stream);
}

extern "C" int va_vgg16_train_step_consensus(va_vgg16* m, const void* x, int x_is_u8, const void* labels, int n, int k, float lr,
                                             float momentum, unsigned long long dropout_seed, void* desc, void* loss_out,
                                             void* workspace, size_t workspace_bytes, void* stream)
{
    VA_CHECK_ARG(n >= 1 && k >= 1 && (long long)n * k <= 64, "va_vgg16_train_step_consensus: %d videos x %d snippets out of range (n*k in [1,64])",
                 n, k);
    return train_step("va_vgg16_train_step_consensus", m, x, x_is_u8, labels, n * k, k, lr, momentum, dropout_seed, desc, loss_out,
                      workspace, workspace_bytes, stream);
}

extern "C" int va_vgg16_train_step_multitask(va_vgg16* m, const void* x, int x_is_u8, const void* labels, const void* tasks, int n, int k,
                                             int n_heads, const int* head_sizes, float lr, float momentum, unsigned long long dropout_seed,
                                             void* desc, void* loss_out, void* workspace, size_t workspace_bytes, void* stream)
{
    const char* who = "va_vgg16_train_step_multitask";
    VA_CHECK_ARG(m != nullptr && tasks != nullptr, "%s: NULL argument", who);
    VA_CHECK_ARG(n >= 1 && k >= 1 && (long long)n * k <= 64, "%s: %d videos x %d snippets out of range (n*k in [1,64])", who, n, k);
    MultiTask mt{(const int*)tasks, {}};
    if (int rc = va_heads_from_sizes(who, n_heads, head_sizes, m->n_classes, &mt.heads)) return rc;
    return train_step(who, m, x, x_is_u8, labels, n * k, k, lr, momentum, dropout_seed, desc, loss_out, workspace, workspace_bytes, stream, &mt);
}

extern "C" size_t va_vgg16_train_grad_floats(const va_vgg16* m)
{
    if (!m || m->dtype != VA_DTYPE_F32) return 0;
    return va_grad_layout_of(m).total;
}

extern "C" int va_vgg16_train_grad_layout(const va_vgg16* m, size_t* offsets, size_t* counts)
{
    VA_CHECK_ARG(m != nullptr && offsets != nullptr && counts != nullptr, "va_vgg16_train_grad_layout: NULL argument");
    VA_CHECK_ARG(m->dtype == VA_DTYPE_F32, "va_vgg16_train_grad_layout: training is fp32 only");
    const va_grad_layout GL = va_grad_layout_of(m);
    for (int s = 0; s < 34; ++s) {
        offsets[s] = GL.off[s];
        counts[s] = GL.cnt[s];
    }
    return VA_OK;
}

extern "C" int va_vgg16_train_accumulate(va_vgg16* m, const void* x, int x_is_u8, const void* labels, const void* tasks, int n, int k,
                                         int n_heads, const int* head_sizes, const float* scales, int first,
                                         unsigned long long dropout_seed, void* desc, void* loss_out, void* grad, size_t grad_floats,
                                         void* workspace, size_t workspace_bytes, void* stream)
{
    const char* who = "va_vgg16_train_accumulate";
    VA_CHECK_ARG(m != nullptr && grad != nullptr && scales != nullptr, "%s: NULL argument", who);
    VA_CHECK_ARG(m->dtype == VA_DTYPE_F32, "%s: training is fp32 only", who);
    VA_CHECK_ARG(n >= 1 && k >= 0 && (long long)n * (k > 0 ? k : 1) <= 64, "%s: %d videos x %d snippets out of range (n * max(k, 1) in [1,64])",
                 who, n, k);
    VA_CHECK_ARG(tasks == nullptr || k >= 1, "%s: the multi-task loss needs k >= 1", who);
    VA_CHECK_ARG(((uintptr_t)grad & 15) == 0, "%s: grad must be 16-byte aligned", who);
    const size_t need = va_grad_layout_of(m).total;
    VA_CHECK_ARG(grad_floats >= need, "%s: gradient buffer of %zu floats needed (va_vgg16_train_grad_floats), %zu given", who, need, grad_floats);
    MultiTask mt{(const int*)tasks, {}};
    if (tasks) {
        if (int rc = va_heads_from_sizes(who, n_heads, head_sizes, m->n_classes, &mt.heads)) return rc;
    } else {
        VA_CHECK_ARG(n_heads == 0, "%s: %d heads without tasks", who, n_heads);
    }
    for (int t = 0; t < (tasks ? n_heads : 1); ++t)
        VA_CHECK_ARG(scales[t] - scales[t] == 0.0f, "%s: scale %d is not finite", who, t);
    const Accum acc{(float*)grad, first, scales};
    return train_step(who, m, x, x_is_u8, labels, n * (k > 0 ? k : 1), k, 0.0f, 0.0f, dropout_seed, desc, loss_out, workspace, workspace_bytes,
                      stream, tasks ? &mt : nullptr, &acc);
}

// src: the 34 tensors in the packed layouts, conv 0..12 as (weight, bias), then fc 0..3 as (weight, bias) -> the reference's layouts
static int unpack_tensors(const va_vgg16* m, const float* const* src, void* const* conv_w, void* const* conv_b, void* const* fc_w,
                          void* const* fc_b, hipStream_t st)
{
    for (int i = 0; i < 13; ++i) {
        const ConvLayer& L = m->conv[i];
        const size_t n = (size_t)L.cout * L.cin * 9;
        k_unpack_conv_w<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(src[2 * i], (float*)conv_w[i], L.cout, L.cin, L.cin_pad);
        VA_HIP(hipMemcpyAsync(conv_b[i], src[2 * i + 1], L.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    for (int i = 0; i < 4; ++i) {
        const size_t n = (size_t)m->fc_out[i] * m->fc_in[i];
        if (i == 0) k_unpack_fc1<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(src[26], (float*)fc_w[0], m->fc_out[0], 512, 49);
        else VA_HIP(hipMemcpyAsync(fc_w[i], src[26 + 2 * i], n * sizeof(float), hipMemcpyDeviceToDevice, st));
        VA_HIP(hipMemcpyAsync(fc_b[i], src[27 + 2 * i], m->fc_out[i] * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    VA_LAUNCH_CHECK();
    return VA_OK;
}

// which = 0: parameters, 1: momentum buffers.  Destination tensors in the reference's layouts (conv OIHW
// [cout][cin][3][3], fc [out][in] with FC1's input CHW-major): what model.state_dict() / optimizer.state_dict() hold.
extern "C" int va_vgg16_export_state(va_vgg16* m, int which, void* const* conv_w, void* const* conv_b, void* const* fc_w,
                                     void* const* fc_b, void* stream)
{
    VA_CHECK_ARG(m != nullptr && conv_w && conv_b && fc_w && fc_b, "va_vgg16_export_state: NULL argument");
    VA_USE_DEVICE(m->ctx);
    VA_CHECK_ARG(m->dtype == VA_DTYPE_F32, "va_vgg16_export_state: fp32 models only");
    VA_CHECK_ARG(which == 0 || (which == 1 && m->conv[0].mom_w), "va_vgg16_export_state: which must be 0, or 1 after va_vgg16_train_init");
    const float* src[34];
    for (int i = 0; i < 13; ++i) {
        src[2 * i] = which ? m->conv[i].mom_w : m->conv[i].wp;
        src[2 * i + 1] = which ? m->conv[i].mom_b : m->conv[i].bias;
    }
    for (int i = 0; i < 4; ++i) {
        src[26 + 2 * i] = which ? m->fc_mom_w[i] : m->fcw[i];
        src[27 + 2 * i] = which ? m->fc_mom_b[i] : m->fcb[i];
    }
    return unpack_tensors(m, src, conv_w, conv_b, fc_w, fc_b, (hipStream_t)stream);
}

// The gradient buffer of va_vgg16_train_accumulate in the reference's layouts: what p.grad holds after loss.backward().
extern "C" int va_vgg16_unpack_grad(va_vgg16* m, const void* grad, void* const* conv_w, void* const* conv_b, void* const* fc_w,
                                    void* const* fc_b, void* stream)
{
    VA_CHECK_ARG(m != nullptr && grad != nullptr && conv_w && conv_b && fc_w && fc_b, "va_vgg16_unpack_grad: NULL argument");
    VA_USE_DEVICE(m->ctx);
    VA_CHECK_ARG(m->dtype == VA_DTYPE_F32, "va_vgg16_unpack_grad: fp32 models only");
    const va_grad_layout GL = va_grad_layout_of(m);
    const float* src[34];
    for (int s = 0; s < 34; ++s) src[s] = (const float*)grad + GL.off[s];
    return unpack_tensors(m, src, conv_w, conv_b, fc_w, fc_b, (hipStream_t)stream);
}

// The inverse: load parameters (which = 0) or momentum buffers (which = 1) from tensors in the reference's layouts.
extern "C" int va_vgg16_import_state(va_vgg16* m, int which, const void* const* conv_w, const void* const* conv_b,
                                     const void* const* fc_w, const void* const* fc_b, void* stream)
{
    VA_CHECK_ARG(m != nullptr && conv_w && conv_b && fc_w && fc_b, "va_vgg16_import_state: NULL argument");
    VA_USE_DEVICE(m->ctx);
    VA_CHECK_ARG(m->dtype == VA_DTYPE_F32, "va_vgg16_import_state: fp32 models only");
    VA_CHECK_ARG(which == 0 || (which == 1 && m->conv[0].mom_w), "va_vgg16_import_state: which must be 0, or 1 after va_vgg16_train_init");
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < 13; ++i) {
        ConvLayer& L = m->conv[i];
        const size_t n = (size_t)L.cout * 9 * L.cin_pad;
        k_repack_conv_w<<<(unsigned)((n + 255) / 256), 256, 0, st>>>((const float*)conv_w[i], which ? L.mom_w : L.wp, L.cout, L.cin, L.cin_pad);
        VA_HIP(hipMemcpyAsync(which ? L.mom_b : L.bias, conv_b[i], L.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    for (int i = 0; i < 4; ++i) {
        const size_t n = (size_t)m->fc_out[i] * m->fc_in[i];
        float* dst = which ? m->fc_mom_w[i] : m->fcw[i];
        if (i == 0) k_repack_fc1<<<(unsigned)((n + 255) / 256), 256, 0, st>>>((const float*)fc_w[0], dst, m->fc_out[0], 512, 49);
        else VA_HIP(hipMemcpyAsync(dst, fc_w[i], n * sizeof(float), hipMemcpyDeviceToDevice, st));
        VA_HIP(hipMemcpyAsync(which ? m->fc_mom_b[i] : m->fcb[i], fc_b[i], m->fc_out[i] * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    VA_LAUNCH_CHECK();
    return VA_OK;
}

// Debugging aid (tests): byte offsets inside the training workspace: out[0..12] = y[i], out[13..25] = p[i] (0 when
// the layer has no pool), out[26] = g[0], out[27] = g[1], out[28] = da0, out[29] = x0.
extern "C" int va_vgg16_train_plan(const va_vgg16* m, int batch, unsigned long long* out)
{
    VA_CHECK_ARG(m != nullptr && out != nullptr && batch >= 1 && batch <= 64, "va_vgg16_train_plan: bad argument");
    VA_USE_DEVICE(m->ctx);
    const TrainPlan T = plan_train(m, batch);
    for (int i = 0; i < 13; ++i) {
        out[i] = T.y[i];
        out[13 + i] = T.p[i];
    }
    out[26] = T.g[0];
    out[27] = T.g[1];
    out[28] = T.da0;
    out[29] = T.x0;
    return VA_OK;
}

// ---------------------------------------------------------------- testing entry points ---------
// One layer of the step at a time through the functions train_step calls (include/va.h, "testing entry points").

#define VA_ALIGNED16(...) ((va_or_ptrs({__VA_ARGS__}) & 15) == 0)
static uintptr_t va_or_ptrs(std::initializer_list<const void*> ps)
{
    uintptr_t v = 0;
    for (const void* p : ps) v |= (uintptr_t)p;
    return v;
}

// mode UPD_SGD: va_train_conv_backward_layer; UPD_STORE / UPD_ADD: va_train_conv_backward_layer_grad (bias = w_packed, unused)
static int conv_backward_entry(const char* who, int mode, va_ctx* ctx, int kernel_opt, int batch, int hw, int cin, int cin_pad, int cout,
                               const float* dy, const float* x, float* w_packed, float* bias, float* mom_w, float* mom_b, float lr,
                               float momentum, float* dx, const float* mask, const float* zeros, float* slab, float* wt, float* bpart,
                               size_t* scratch_floats, char* info, int info_len, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_USE_DEVICE(ctx);
    if (info && info_len > 0) info[0] = 0;
    VA_CHECK_ARG(scratch_floats != nullptr, "%s: scratch_floats is NULL", who);
    VA_CHECK_ARG(kernel_opt == 0 || kernel_opt == 1, "%s: kernel_opt (VA_OPT_F32_CONV_KERNEL) must be 0 or 1", who);
    VA_CHECK_ARG(batch >= 1 && batch <= 64, "%s: batch %d out of range [1,64]", who, batch);
    VA_CHECK_ARG(hw >= 1 && hw <= 224, "%s: hw %d out of range [1,224]", who, hw);
    VA_CHECK_ARG(cin_pad >= 4 && cin_pad % 4 == 0 && cin_pad <= 4096, "%s: cin_pad %d must be a multiple of 4 in [4,4096] (16-byte loads)", who, cin_pad);
    VA_CHECK_ARG(cout >= 4 && cout % 4 == 0 && cout <= 4096, "%s: cout %d must be a multiple of 4 in [4,4096] (16-byte loads)", who, cout);
    VA_CHECK_ARG(cin >= 1 && cin <= cin_pad, "%s: cin %d outside [1, cin_pad = %d]", who, cin, cin_pad);
    VA_CHECK_ARG(mask == nullptr || dx != nullptr, "%s: mask without dx", who);
    // the data gradient runs the forward dispatch: 16-channel K steps, 64-channel N tiles
    VA_CHECK_ARG(!dx || (cin == cin_pad && cin % 64 == 0 && cout % 16 == 0),
                 "%s: dx needs cin == cin_pad, cin %% 64 == 0 and cout %% 16 == 0 (got cin %d, cin_pad %d, cout %d)", who, cin, cin_pad, cout);
    const WgradPlan wp = plan_wgrad(batch, hw, cout, cin_pad);
    const int nblk = bgrad_blocks((long)batch * hw * hw);
    const size_t need[3] = {wp.slab_floats, (size_t)cin * 9 * cout, (size_t)nblk * cout};
    const size_t have[3] = {scratch_floats[0], scratch_floats[1], scratch_floats[2]};
    for (int i = 0; i < 3; ++i) scratch_floats[i] = need[i];
    char plan[160];
    snprintf(plan, sizeof plan, "k_conv_wgrad<%s> S=%d chunk=%d Mpad=%d Npad=%d bgrad_blocks=%d", wp.BM == 64 ? "1,3" : "2,2", wp.S, wp.chunk,
             wp.Mpad, wp.Npad, nblk);
    if (slab == nullptr) {  // size query
        if (info && info_len > 0) snprintf(info, (size_t)info_len, "%s dgrad=%s", plan, "none");
        return VA_OK;
    }
    VA_CHECK_ARG(dy && x && w_packed && bias && mom_w && mom_b && zeros && bpart && (wt || !dx), "%s: NULL argument", who);
    VA_CHECK_ARG(VA_ALIGNED16(dy, x, w_packed, bias, mom_w, mom_b, dx, mask, zeros, slab, wt, bpart),
                 "%s: every pointer must be 16-byte aligned (16-byte vector accesses)", who);
    if (have[0] < need[0] || have[2] < need[2] || (dx && have[1] < need[1])) {
        va_set_error("%s: scratch of {%zu, %zu, %zu} floats needed (slab, wt, bpart), {%zu, %zu, %zu} given", who, need[0], dx ? need[1] : 0,
                     need[2], have[0], have[1], have[2]);
        return VA_ERR_WORKSPACE;
    }
    const char* dname = nullptr;
    if (int rc = conv_backward_layer(batch, hw, cin, cin_pad, cout, dy, x, w_packed, bias, mom_w, mom_b, dx, mask, zeros, kernel_opt, wt, slab,
                                     bpart, plain_update(lr, momentum), (hipStream_t)stream, &dname, mode))
        return rc;
    if (info && info_len > 0) snprintf(info, (size_t)info_len, "%s dgrad=%s", plan, dname ? dname : "none");
    return VA_OK;
}

extern "C" int va_train_conv_backward_layer(va_ctx* ctx, int kernel_opt, int batch, int hw, int cin, int cin_pad, int cout, const float* dy,
                                            const float* x, float* w_packed, float* bias, float* mom_w, float* mom_b, float lr,
                                            float momentum, float* dx, const float* mask, const float* zeros, float* slab, float* wt,
                                            float* bpart, size_t* scratch_floats, char* info, int info_len, void* stream)
{
    return conv_backward_entry("va_train_conv_backward_layer", UPD_SGD, ctx, kernel_opt, batch, hw, cin, cin_pad, cout, dy, x, w_packed, bias,
                               mom_w, mom_b, lr, momentum, dx, mask, zeros, slab, wt, bpart, scratch_floats, info, info_len, stream);
}

extern "C" int va_train_conv_backward_layer_grad(va_ctx* ctx, int kernel_opt, int batch, int hw, int cin, int cin_pad, int cout,
                                                 const float* dy, const float* x, const float* w_packed, int add, float* grad_w,
                                                 float* grad_b, float* dx, const float* mask, const float* zeros, float* slab, float* wt,
                                                 float* bpart, size_t* scratch_floats, char* info, int info_len, void* stream)
{
    float* w = const_cast<float*>(w_packed);  // UPD_STORE / UPD_ADD only read it (k_pack_dgrad_w)
    return conv_backward_entry("va_train_conv_backward_layer_grad", add ? UPD_ADD : UPD_STORE, ctx, kernel_opt, batch, hw, cin, cin_pad, cout, dy,
                               x, w, w, grad_w, grad_b, 0.0f, 0.0f, dx, mask, zeros, slab, wt, bpart, scratch_floats, info, info_len, stream);
}

static int fc_backward_entry(const char* who, int mode, va_ctx* ctx, int batch, int out_f, int in_f, const float* dz, const float* x, float* w,
                             float* bias, float* mom_w, float* mom_b, float lr, float momentum, float* dx, const float* mask, float scale,
                             char* info, int info_len, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_USE_DEVICE(ctx);
    if (info && info_len > 0) info[0] = 0;
    VA_CHECK_ARG(batch >= 1 && batch <= 64, "%s: batch %d out of range [1,64]", who, batch);
    VA_CHECK_ARG(out_f >= 1 && in_f >= 1 && out_f <= 16 * 65535 && (long)out_f * in_f < 2147483647L, "%s: out_f %d / in_f %d out of range", who,
                 out_f, in_f);
    VA_CHECK_ARG(dz && x && w && bias && mom_w && mom_b && dx, "%s: NULL argument", who);
    VA_CHECK_ARG(VA_ALIGNED16(dz, x, w, bias, mom_w, mom_b, dx, mask), "%s: every pointer must be 16-byte aligned", who);
    int inst = 0;
    if (int rc = fc_backward_layer(batch, out_f, in_f, dz, x, w, bias, mom_w, mom_b, dx, mask, scale, plain_update(lr, momentum), (hipStream_t)stream, &inst, mode))
        return rc;
    VA_LAUNCH_CHECK();
    if (info && info_len > 0) snprintf(info, (size_t)info_len, "k_fc_dx<%d>", inst);
    return VA_OK;
}

extern "C" int va_train_fc_backward_layer(va_ctx* ctx, int batch, int out_f, int in_f, const float* dz, const float* x, float* w, float* bias,
                                          float* mom_w, float* mom_b, float lr, float momentum, float* dx, const float* mask, float scale,
                                          char* info, int info_len, void* stream)
{
    return fc_backward_entry("va_train_fc_backward_layer", UPD_SGD, ctx, batch, out_f, in_f, dz, x, w, bias, mom_w, mom_b, lr, momentum, dx, mask,
                             scale, info, info_len, stream);
}

extern "C" int va_train_fc_backward_layer_grad(va_ctx* ctx, int batch, int out_f, int in_f, const float* dz, const float* x, const float* w,
                                               int add, float* grad_w, float* grad_b, float* dx, const float* mask, float scale, char* info,
                                               int info_len, void* stream)
{
    float* wr = const_cast<float*>(w);  // UPD_STORE / UPD_ADD only read it (k_fc_dx)
    return fc_backward_entry("va_train_fc_backward_layer_grad", add ? UPD_ADD : UPD_STORE, ctx, batch, out_f, in_f, dz, x, wr, wr, grad_w, grad_b,
                             0.0f, 0.0f, dx, mask, scale, info, info_len, stream);
}

extern "C" int va_train_pool_layer(va_ctx* ctx, int batch, int hw, int c, const float* y, float* p, const float* dp, float* dy, void* stream)
{
    const char* who = "va_train_pool_layer";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(batch >= 1 && batch <= 64, "%s: batch %d out of range [1,64]", who, batch);
    VA_CHECK_ARG(hw >= 2 && hw % 2 == 0 && hw <= 224, "%s: hw %d must be even and in [2,224]", who, hw);
    VA_CHECK_ARG(c >= 4 && c % 4 == 0 && c <= 4096, "%s: c %d must be a multiple of 4 in [4,4096] (four channels per thread)", who, c);
    VA_CHECK_ARG(y && p && ((dp == nullptr) == (dy == nullptr)), "%s: NULL y / p, or only one of dp / dy", who);
    VA_CHECK_ARG(VA_ALIGNED16(y, p, dp, dy), "%s: every pointer must be 16-byte aligned", who);
    pool_forward(y, p, batch, hw, c, (hipStream_t)stream);
    if (dp) pool_backward(dp, y, p, dy, batch, hw, c, (hipStream_t)stream);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_train_loss(va_ctx* ctx, const float* logits, const void* labels, int n, int k, int c, float* dlogits, float* out, void* stream)
{
    const char* who = "va_train_loss";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(n >= 1 && k >= 0 && (long long)n * (k > 0 ? k : 1) <= 64, "%s: %d rows x %d snippets out of range (n * max(k, 1) in [1,64])", who, n, k);
    VA_CHECK_ARG(c >= 1 && c <= (1 << 20), "%s: c %d out of range", who, c);
    VA_CHECK_ARG(logits && labels && dlogits && out, "%s: NULL argument", who);
    if (int rc = loss_layer(logits, (const long long*)labels, n * (k > 0 ? k : 1), k, c, dlogits, out, (hipStream_t)stream)) return rc;
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_train_loss_multitask(va_ctx* ctx, const float* logits, const void* labels, const void* tasks, int n, int k, int n_heads,
                                       const int* head_sizes, float* dlogits, float* out, void* stream)
{
    const char* who = "va_train_loss_multitask";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(n >= 1 && k >= 0 && (long long)n * (k > 0 ? k : 1) <= 64, "%s: %d rows x %d snippets out of range (n * max(k, 1) in [1,64])", who, n, k);
    MultiTask mt{(const int*)tasks, {}};
    if (int rc = va_heads_from_sizes(who, n_heads, head_sizes, -1, &mt.heads)) return rc;
    const int c = mt.heads.off[n_heads];
    VA_CHECK_ARG(c >= 1 && c <= (1 << 20), "%s: c %d out of range", who, c);
    VA_CHECK_ARG(logits && labels && tasks && dlogits && out, "%s: NULL argument", who);
    if (int rc = loss_layer(logits, (const long long*)labels, n * (k > 0 ? k : 1), k, c, dlogits, out, (hipStream_t)stream, &mt)) return rc;
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_train_dropout(va_ctx* ctx, float* x, size_t n, unsigned long long dropout_seed, int layer, void* stream)
{
    const char* who = "va_train_dropout";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x != nullptr && n >= 1 && n <= (size_t)1 << 31, "%s: NULL x or n out of range [1, 2^31]", who);
    VA_CHECK_ARG(layer >= 0 && layer <= 2, "%s: layer %d out of range [0,2]", who, layer);
    dropout_layer(x, n, dropout_seed, layer, 0.5f, (hipStream_t)stream);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_train_dropout_p(va_ctx* ctx, float* x, size_t n, unsigned long long dropout_seed, int layer, float p, void* stream)
{
    const char* who = "va_train_dropout_p";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x != nullptr && n >= 1 && n <= (size_t)1 << 31, "%s: NULL x or n out of range [1, 2^31]", who);
    VA_CHECK_ARG(layer >= 0 && layer <= 2, "%s: layer %d out of range [0,2]", who, layer);
    VA_CHECK_ARG(p >= 0.0f && p < 1.0f, "%s: p %g outside [0, 1)", who, (double)p);
    dropout_layer(x, n, dropout_seed, layer, p, (hipStream_t)stream);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

// ---------------------------------------------------------------- the solver ---

extern "C" void va_solver_default(va_solver* s)
{
    if (!s) return;
    s->weight_decay = 0.0f;
    s->bias_lr_mult = 1.0f;
    s->bias_decay_mult = 1.0f;
    for (int i = 0; i < 3; ++i) s->dropout[i] = 0.5f;
    s->frozen_layers = 0;
}

extern "C" int va_vgg16_set_solver(va_vgg16* m, const va_solver* s)
{
    const char* who = "va_vgg16_set_solver";
    VA_CHECK_ARG(m != nullptr && s != nullptr, "%s: NULL argument", who);
    VA_CHECK_ARG(m->dtype == VA_DTYPE_F32, "%s: training is fp32 only (bf16 model)", who);
    auto ok = [](float v) { return v - v == 0.0f && v >= 0.0f; };  // finite and not negative
    VA_CHECK_ARG(ok(s->weight_decay), "%s: weight_decay %g must be finite and >= 0", who, (double)s->weight_decay);
    VA_CHECK_ARG(ok(s->bias_lr_mult), "%s: bias_lr_mult %g must be finite and >= 0", who, (double)s->bias_lr_mult);
    VA_CHECK_ARG(ok(s->bias_decay_mult), "%s: bias_decay_mult %g must be finite and >= 0", who, (double)s->bias_decay_mult);
    for (int i = 0; i < 3; ++i)
        VA_CHECK_ARG(s->dropout[i] >= 0.0f && s->dropout[i] < 1.0f, "%s: dropout[%d] %g outside [0, 1)", who, i, (double)s->dropout[i]);
    VA_CHECK_ARG(s->frozen_layers >= 0 && s->frozen_layers <= 16, "%s: frozen_layers %d outside 0..16", who, s->frozen_layers);
    m->solver = *s;
    return VA_OK;
}

extern "C" int va_vgg16_get_solver(const va_vgg16* m, va_solver* s)
{
    VA_CHECK_ARG(m != nullptr && s != nullptr, "va_vgg16_get_solver: NULL argument");
    *s = m->solver;
    return VA_OK;
}
