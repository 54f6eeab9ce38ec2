// TV-L1 dense optical flow for gfx950 (MI355X): hand-written HIP, no CPU fallback.
//
// Replaces the unknown upstream tool that wrote the flow_x_/flow_y_ images the reference reads
// (Sheet03/temporalModel.py:76-81, Sheet03/parameters.py:27,38-39).  The algorithm is the
// published TV-L1 (Zach/Pock/Bischof 2007; Sanchez/Meinhardt-Llopis/Facciolo, IPOL 2013) with
// every open choice fixed in DESIGN.md "TV-L1 specification" (steps S0..S9).  This file must be
// compiled with -ffp-contract=off: the arithmetic contract is IEEE binary32 in the written
// operation order with explicit fmaf only, so that results are independent of the tiling and of
// block_iters, and comparable bit for bit with an independent implementation.
//
// S0-S2 (frames, pyramid, gradient) and the level geometry are the front end the three flow methods share: flow_common.hip.
//
// Data layout in HBM (all fp32, row pitch = width rounded up to 4 floats so that a lane's
// 4-pixel run is one aligned 16-byte access):
//   pyramid  [level][frame][3 = I, Ix, Iy][h][pitch]      built once per FRAME, shared by the
//                                                          two pairs that frame belongs to
//   state    2 x [pair][6 = u1,u2,p11,p12,p21,p22][h][pitch]   ping-pong (halo reads vs writes)
//   ro       [pair][4 = I1wx, I1wy, rho_c, 1/|grad|^2][h][pitch]  per-warp constants
//
// Dominant kernels: the inner iterations (S6), in two forms that share their arithmetic operation
// for operation (and so their results, bit for bit):
//   k_iter_tile    One workgroup owns a (64*R) x (NW*C) pixel tile; every thread keeps an R x C
//                  patch of all 10 fields in REGISTERS for `K` consecutive inner iterations
//                  (temporal blocking with a K-pixel overlapped halo).  Horizontal neighbours come
//                  from the adjacent lane by DPP wave shifts, vertical neighbours of the patch's
//                  first/last row from the adjacent wave through a 2-row LDS exchange.
//   k_iter_stream  A pipeline of FOUR waves (one or two in the fallback forms) owns a strip of 128
//                  columns and streams its rows top to bottom ONCE per launch, carrying every row
//                  through K iterations on the way (time-skewed: level t works one row behind level
//                  t-1; a wave hands its rows on to the next through LDS); no y halo.  Used where
//                  the strips are well filled (level_streams()).
// Either way the HBM traffic per pixel-iteration falls from the algorithmic 64 B to about
// 64 B / K / efficiency.
#include "va_internal.h"
#include <cmath>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <type_traits>

namespace {

constexpr int kNF_STATE = 6;
constexpr int kNF_RO = 4;

// ---------------------------------------------------------------- per-warp kernel ------------

// S3 for the three warped images at once, with the wave supplying half of the taps: consecutive lanes
// are consecutive pixels of a row, and wherever the flow is smooth lane i+1's left taps (x0+1, y0),
// (x0+1, y1) ARE lane i's right taps, so they arrive by a wave shuffle instead of a second gather
// (same values, same arithmetic: the result is bit-identical to bilinear()).
__device__ __forceinline__ void bilinear3_shfl(const float* __restrict__ I1, size_t plane, int w, int h, int pitch, float x,
                                               float y, bool active, float& v0, float& v1, float& v2)
{
    x = fminf(fmaxf(x, 0.0f), (float)(w - 1));
    y = fminf(fmaxf(y, 0.0f), (float)(h - 1));
    const int x0 = (int)x, y0 = (int)y;
    const int x1 = d_min(x0 + 1, w - 1), y1 = d_min(y0 + 1, h - 1);
    const float ax = x - (float)x0, ay = y - (float)y0;
    const int o00 = y0 * pitch + x0, o10 = y1 * pitch + x0;
    float a[3], c[3], b[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = active ? I1[k * plane + o00] : 0.0f;
        c[k] = active ? I1[k * plane + o10] : 0.0f;
    }
    // the neighbouring lane's left column is my right column iff it starts one pixel to the right on the same rows
    const int nx0 = __shfl_down(x0, 1), ny0 = __shfl_down(y0, 1), ny1 = __shfl_down(y1, 1);
    const bool nact = __shfl_down((int)active, 1) != 0;
    const bool from_lane = (threadIdx.x & 63) != 63 && nact && nx0 == x1 && ny0 == y0 && ny1 == y1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float na = __shfl_down(a[k], 1), nc = __shfl_down(c[k], 1);
        if (x1 == x0) {  // clamped at the right border: the right taps are the left taps
            b[k] = a[k];
            d[k] = c[k];
        } else if (from_lane) {
            b[k] = na;
            d[k] = nc;
        } else {
            b[k] = active ? I1[k * plane + y0 * pitch + x1] : 0.0f;
            d[k] = active ? I1[k * plane + y1 * pitch + x1] : 0.0f;
        }
    }
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float top = fmaf(ax, b[k] - a[k], a[k]);
        const float bot = fmaf(ax, d[k] - c[k], c[k]);
        r[k] = fmaf(ay, bot - top, top);
    }
    v0 = r[0];
    v1 = r[1];
    v2 = r[2];
}

// S5.  One thread per pixel of one pair; the 12 bilinear taps of a pixel are 6 L1/L2-served gathers plus
// 6 wave shuffles where the flow is smooth (25 launches per pair against 7500 inner iterations:
// lower-order).
__global__ void k_warp(const float* __restrict__ pyr, size_t plane, int w, int h, int pitch, int fps,
                       const float* __restrict__ stA, const float* __restrict__ stB, const int* __restrict__ sel, int cur,
                       int* __restrict__ base, float* __restrict__ ro, int pair0, int perm)
{
    // XCD-aware workgroup order (as in k_iter_tile): the pixel blocks of a pair gather from one L2
    unsigned lid = blockIdx.y * gridDim.x + blockIdx.x;
    {
        const unsigned nb = gridDim.x * gridDim.y, q = nb / 8, r = nb % 8, xcd = lid % 8, kk = lid / 8;
        lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + kk;
    }
    const int pair = pair0 + (int)(lid / gridDim.x);
    const int idx = (int)(lid % gridDim.x) * blockDim.x + threadIdx.x;
    const int which = sel ? sel[pair] : cur;
    if (base && idx == 0) base[pair] = which;
    const bool active = idx < w * h;  // inactive lanes still take part in the shuffles
    const int y = active ? idx / w : 0, x = active ? idx - y * w : 0;
    const int seq = pair / (fps - 1), k = pair - seq * (fps - 1);
    const int f0 = seq * fps + k;
    const float* I0 = pyr + (size_t)f0 * 3 * plane;
    const float* I1 = pyr + (size_t)(f0 + 1) * 3 * plane;
    const float* st = (which ? stB : stA) + (size_t)pair * kNF_STATE * plane;
    const size_t o = (size_t)y * pitch + x, op = (size_t)y * pitch + pslot(x, perm);
    const float u1 = active ? st[op] : 0.0f, u2 = active ? st[plane + op] : 0.0f;
    float Iw, Iwx, Iwy;
    bilinear3_shfl(I1, plane, w, h, pitch, (float)x + u1, (float)y + u2, active, Iw, Iwx, Iwy);
    if (!active) return;
    const float grad = fmaf(Iwy, Iwy, Iwx * Iwx);
    float* r = ro + (size_t)pair * kNF_RO * plane;
    r[op] = Iwx;
    r[plane + op] = Iwy;
    r[2 * plane + op] = fmaf(-Iwy, u2, fmaf(-Iwx, u1, Iw - I0[o]));
    r[3 * plane + op] = grad < 1e-10f ? 0.0f : 1.0f / grad;
}

// S8.  Upsample the coarse flow (cw,ch) of buffer `which` into tmp [pair][2][fplane].  A separate
// target is needed because with the stopping rule different pairs can hold their newest state in
// different ping-pong buffers, and the coarse and fine layouts of different pairs overlap.
__global__ void k_upsample(const float* __restrict__ stA, const float* __restrict__ stB, const int* __restrict__ sel,
                           int cur, int cw, int ch, int cpitch, size_t cplane, float* __restrict__ tmp, int fw, int fh,
                           int fpitch, size_t fplane, float inv_step, int cperm)
{
    const int pair = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= fw * fh) return;
    const int which = sel ? sel[pair] : cur;
    const float* src = (which ? stB : stA) + (size_t)pair * kNF_STATE * cplane;
    float* dst = tmp + (size_t)pair * 2 * fplane;
    const int y = idx / fw, x = idx - y * fw;
    const float rx = (float)cw / (float)fw, ry = (float)ch / (float)fh;
    const size_t o = (size_t)y * fpitch + x;
    dst[o] = bilinear(src, cw, ch, cpitch, (float)x * rx, (float)y * ry, cperm) * inv_step;
    dst[fplane + o] = bilinear(src + cplane, cw, ch, cpitch, (float)x * rx, (float)y * ry, cperm) * inv_step;
}

// S4: start of a level: u from tmp, p = 0, everything in ping-pong buffer 0.
// Also zeroes the pitch padding (columns w .. pitch-1) of the state: k_iter_tile loads whole 4-pixel
// runs, and although no padding value can reach a valid pixel (the forward differences at x = w-1
// are multiplied by 0), a NaN/Inf bit pattern left there by an earlier owner of the workspace would
// (NaN * 0 = NaN).  Everything the kernels themselves write is finite.
__global__ void k_level_init(const float* __restrict__ tmp, float* __restrict__ st0, int w, int h, int pitch, size_t plane, int perm)
{
    const int pair = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= pitch * h) return;
    const int y = idx / pitch, x = idx - y * pitch;
    const size_t o = (size_t)y * pitch + x, op = (size_t)y * pitch + pslot(x, perm);  // (pitch is a multiple of 4: pslot stays inside the row)
    const float* t = tmp + (size_t)pair * 2 * plane;
    float* dst = st0 + (size_t)pair * kNF_STATE * plane;
    dst[op] = x < w ? t[o] : 0.0f;
    dst[plane + op] = x < w ? t[plane + o] : 0.0f;
    dst[2 * plane + op] = 0.0f;
    dst[3 * plane + op] = 0.0f;
    dst[4 * plane + op] = 0.0f;
    dst[5 * plane + op] = 0.0f;
}

// Zero the pitch padding of the nf planes of every pair (the per-warp constants: k_warp writes x < w only).
__global__ void k_zero_pad(float* __restrict__ buf, int nf, int w, int h, int pitch, size_t plane, int perm)
{
    const int pair = blockIdx.y, pw = pitch - w;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= pw * h * nf) return;
    const int f = idx / (pw * h), r = idx - f * pw * h, y = r / pw, x = w + r - y * pw;
    buf[((size_t)pair * nf + f) * plane + (size_t)y * pitch + pslot(x, perm)] = 0.0f;
}

__global__ void k_flow_out(const float* __restrict__ stA, const float* __restrict__ stB, const int* __restrict__ sel,
                           int cur, int w, int h, int pitch, size_t plane, float* __restrict__ flow, int perm)
{
    const int pair = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= w * h) return;
    const int which = sel ? sel[pair] : cur;
    const float* st = (which ? stB : stA) + (size_t)pair * kNF_STATE * plane;
    const int y = idx / w, x = idx - y * w;
    flow[((size_t)pair * 2) * w * h + idx] = st[(size_t)y * pitch + pslot(x, perm)];
    flow[((size_t)pair * 2 + 1) * w * h + idx] = st[plane + (size_t)y * pitch + pslot(x, perm)];
}

// S9
__global__ void k_flow_to_stack(const float* __restrict__ flow, float* __restrict__ stack, size_t n, float bound,
                                float mean, float stdv)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float t = (255.0f * (flow[i] + bound)) / (2.0f * bound);
    const float q = rintf(fminf(fmaxf(t, 0.0f), 255.0f));
    stack[i] = (q / 255.0f - mean) / stdv;
}

// ---------------------------------------------------------------- inner iterations -----------

struct IterArgs {
    const float* ro;
    const float* stA;
    const float* stB;
    float* outA;
    float* outB;
    const int* base;  // EPS mode: per-pair buffer index at the start of this warp's loop
    int* sel;         // EPS mode: per-pair index of the buffer holding the newest state
    unsigned long long* err;  // EPS mode: [pair][iters] exact integer error sums (S7)
    unsigned long long qthr;
    size_t plane;
    int cur;  // fixed mode: input buffer index
    int w, h, pitch;
    int K;    // iterations in this launch
    int ntx, nty, HX;
    int it, iters;
    int rev;  // odd launches walk the workgroup order backwards: what the previous launch wrote last is read first
    int pair0;  // first pair of this launch (a level's pairs are processed in chunks)
    float l_t, taut, theta;
};

__device__ __forceinline__ float dpp_from_left(float v)  // lane i <- lane i-1, lane 0 <- 0
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float dpp_from_right(float v)  // lane i <- lane i+1, lane 63 <- 0
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}

typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }  // v_pk_fma_f32
// a - b as one v_sub_f32 the vectoriser cannot re-pack (see the x differences in k_iter_tile)
__device__ __forceinline__ float sub_s(float a, float b)
{
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ f2 splat(float v) { return f2{v, v}; }

// Correctly rounded square root and reciprocal from the hardware seeds with packed FMAs only (one
// Newton step on the exact FMA residual; no denormal scaling, no special-case selects).  Both are
// bit-identical to the IEEE sqrtf() / 1.0f/x of the arithmetic contract on their whole domain:
// va_selftest_exact_math() compares them EXHAUSTIVELY (every float in [2^-100, 1e30] resp. [1, 1e30])
// against the compiler's correctly rounded expansions; tests/test_tvl1_gpu.py runs that check.  (The
// raw seeds fail it on 31 % resp. 11 % of the inputs; gfx950's v_rsq_f32 / v_rcp_f32 are accurate
// enough that the second refinement step of the textbook sequences is never needed.)
constexpr float kSqrtReg = 7.888609052210118e-31f;  // 2^-100
__device__ __forceinline__ f2 sqrt_exact_pk(f2 s)  // s in [2^-100, 1e30]
{
    const f2 y = f2{__builtin_amdgcn_rsqf(s.x), __builtin_amdgcn_rsqf(s.y)};
    const f2 g = s * y, h = y * 0.5f;
    const f2 d = pk_fma(-g, g, s);  // exact residual s - g^2
    return pk_fma(d, h, g);
}
__device__ __forceinline__ f2 rcp_exact_pk(f2 d)  // d in [1, 1e30]
{
    const f2 r = f2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    const f2 e = pk_fma(-d, r, splat(1.0f));  // exact residual 1 - d r
    return pk_fma(e, r, r);
}

__global__ void k_selftest_exact_math(unsigned lo, unsigned long long n, unsigned long long* bad)
{
    unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long b0 = 0, b1 = 0;
    for (; i < n; i += stride) {
        const float x = __uint_as_float(lo + (unsigned)i);
        const f2 v = f2{x, x};
        b0 += __float_as_uint(sqrt_exact_pk(v).y) != __float_as_uint(sqrtf(x));
        if (x >= 1.0f) b1 += __float_as_uint(rcp_exact_pk(v).x) != __float_as_uint(1.0f / x);
    }
    if (b0) atomicAdd(&bad[0], b0);
    if (b1) atomicAdd(&bad[1], b1);
}

// RP float2 per row: RP == 1 -> one 8-byte access, RP == 2 -> one 16-byte access.
template <int RP>
__device__ __forceinline__ void load_row(const float* __restrict__ row, int x0, int pitch, bool rowok, f2 (&v)[RP])
{
#pragma unroll
    for (int j = 0; j < RP; ++j) v[j] = f2{0.0f, 0.0f};
    if (!rowok || x0 >= pitch) return;
    if constexpr (RP == 2) {
        const float4 t = *reinterpret_cast<const float4*>(row + x0);
        v[0] = f2{t.x, t.y};
        v[1] = f2{t.z, t.w};
    } else {
        const float2 t = *reinterpret_cast<const float2*>(row + x0);
        v[0] = f2{t.x, t.y};
    }
}

template <int RP>
__device__ __forceinline__ void store_row(float* __restrict__ row, int x0, int pitch, const f2 (&v)[RP])
{
    if (x0 >= pitch) return;
    if constexpr (RP == 2) *reinterpret_cast<float4*>(row + x0) = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
    else *reinterpret_cast<float2*>(row + x0) = make_float2(v[0].x, v[0].y);
}

// S6 (+S7 when EPS).  Tile = (128*RP) x (NW*C) pixels; a thread keeps C rows of 2*RP pixels of all ten
// fields in registers as float2 pairs, so that the bulk of the arithmetic issues as v_pk_fma_f32 /
// v_pk_mul_f32 / v_pk_add_f32 (two pixels per VALU instruction: a wave64 VALU instruction occupies
// its SIMD for 4 cycles on gfx950 whether it is packed or not -- measured, profiles/README.md).
//
// LX = lanes of a wave along x.  A wave is folded into GPW = 64/LX row groups of LX lanes (LX = 64:
// 256x32 tile; 32: 128x64; 21: 84x96, lane 63 idle; 16: 64x128), so that narrow pyramid levels get
// tall tiles; NG = NW*GPW row groups of C rows each.
template <int RP, int C, int NW, int LX, bool EPS, bool FAST>
__global__ void __launch_bounds__(NW * 64) k_iter_tile(IterArgs a)
{
    constexpr int R = 2 * RP, TW = LX * R, GPW = 64 / LX, NG = NW * GPW, TH = NG * C;
    static_assert(RP == 2, "the interleaved pixel layout (pslot) is written for four pixels per thread row");
    // row NG of the exchange arrays is a dummy for idle lanes (64 % LX != 0); row NG + 1 stays zero: it is
    // the "row above" of the first and the "row below" of the last row group
    __shared__ __attribute__((aligned(16))) float sP12[NG + 2][TW], sP22[NG + 2][TW], sU1[NG + 2][TW], sU2[NG + 2][TW];
    __shared__ unsigned long long sErr;

    // XCD-aware workgroup order: the tiles of a pair (which share their halos) on one XCD's L2
    unsigned lid = blockIdx.y * gridDim.x + blockIdx.x;
    {
        const unsigned nb = gridDim.x * gridDim.y, q = nb / 8, r = nb % 8, xcd = lid % 8, kk = lid / 8;
        lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + kk;
        if (a.rev) lid = nb - 1 - lid;
    }
    const int pair = a.pair0 + (int)(lid / gridDim.x), bx = (int)(lid % gridDim.x);
    int inbuf = a.cur;
    if constexpr (EPS) {
        // S7: a pair that met the stopping rule at iteration it-1 (or earlier: its later
        // counters stay 0 < qthr) does nothing more in this warp.
        if (a.it > 0 && a.err[(size_t)pair * a.iters + a.it - 1] < a.qthr) return;
        inbuf = a.base[pair] ^ (a.it & 1);
        if (bx == 0 && threadIdx.x == 0) a.sel[pair] = inbuf ^ 1;
        if (threadIdx.x == 0) sErr = 0ull;
    }
    const int l64 = threadIdx.x & 63;
    const bool idle = l64 / LX >= GPW;                                     // lanes beyond the last whole row group
    const int lane = idle ? 0 : l64 % LX;                                  // position along x
    const int wave = idle ? NG : (int)(threadIdx.x >> 6) * GPW + l64 / LX;  // row group
    const int tx = bx % a.ntx, ty = bx / a.ntx;
    const int w = a.w, h = a.h, pitch = a.pitch, K = a.K;
    const int ox = tx * (TW - 2 * a.HX), oy = ty * (TH - 2 * K);
    const int vx0 = ox + (tx > 0 ? a.HX : 0), vx1 = (tx == a.ntx - 1) ? w : ox + TW - a.HX;
    const int vy0 = oy + (ty > 0 ? K : 0), vy1 = (ty == a.nty - 1) ? h : oy + TH - K;
    const int x0 = idle ? (1 << 28) : ox + lane * R, y0 = oy + wave * C;  // idle lanes: outside every image
    // folded waves: the DPP "left neighbour" of a row group's first lane belongs to another row group
    const float lfix = (LX == 64 || lane > 0) ? 1.0f : 0.0f;

    const float* __restrict__ ro = a.ro + (size_t)pair * kNF_RO * a.plane;
    const float* __restrict__ sin = (inbuf ? a.stB : a.stA) + (size_t)pair * kNF_STATE * a.plane;
    float* __restrict__ sout = (inbuf ? a.outA : a.outB) + (size_t)pair * kNF_STATE * a.plane;

    // columns a run may touch: up to the last 4-pixel run holding a valid pixel
    const int xlim = (w + 3) & ~3;
    f2 u1[C][RP], u2[C][RP], p11[C][RP], p12[C][RP], p21[C][RP], p22[C][RP];
    f2 wx[C][RP], wy[C][RP], rc[C][RP], ig[C][RP];
#pragma clang loop unroll(full)
    for (int c = 0; c < C; ++c) {
        const int y = y0 + c;
        const bool rowok = y < h;
        const size_t ro_ = (size_t)y * pitch;
        load_row<RP>(sin + ro_, x0, xlim, rowok, u1[c]);
        load_row<RP>(sin + a.plane + ro_, x0, xlim, rowok, u2[c]);
        load_row<RP>(sin + 2 * a.plane + ro_, x0, xlim, rowok, p11[c]);
        load_row<RP>(sin + 3 * a.plane + ro_, x0, xlim, rowok, p12[c]);
        load_row<RP>(sin + 4 * a.plane + ro_, x0, xlim, rowok, p21[c]);
        load_row<RP>(sin + 5 * a.plane + ro_, x0, xlim, rowok, p22[c]);
        load_row<RP>(ro + ro_, x0, xlim, rowok, wx[c]);
        load_row<RP>(ro + a.plane + ro_, x0, xlim, rowok, wy[c]);
        load_row<RP>(ro + 2 * a.plane + ro_, x0, xlim, rowok, rc[c]);
        load_row<RP>(ro + 3 * a.plane + ro_, x0, xlim, rowok, ig[c]);
    }

    // Forward-difference border rule as 0/1 multipliers (x < w-1, y < h-1): exact (d*1 = d, d*0 = 0).
    f2 mx[RP];
    float my[C];
#pragma clang loop unroll(full)
    for (int j = 0; j < RP; ++j) mx[j] = f2{x0 + j < w - 1 ? 1.0f : 0.0f, x0 + j + 2 < w - 1 ? 1.0f : 0.0f};  // pack j = pixels x0+j, x0+j+2
#pragma clang loop unroll(full)
    for (int c = 0; c < C; ++c) my[c] = y0 + c < h - 1 ? 1.0f : 0.0f;

    const float l_t = a.l_t;
    const f2 taut = splat(a.taut), theta = splat(a.theta), one = splat(1.0f);
    unsigned long long qsum = 0ull;

    f2* const rowP12 = reinterpret_cast<f2*>(&sP12[wave][lane * R]);
    f2* const rowP22 = reinterpret_cast<f2*>(&sP22[wave][lane * R]);
    f2* const rowU1 = reinterpret_cast<f2*>(&sU1[wave][lane * R]);
    f2* const rowU2 = reinterpret_cast<f2*>(&sU2[wave][lane * R]);
    const int upRow = wave > 0 ? wave - 1 : NG + 1, dnRow = wave < NG - 1 ? wave + 1 : NG + 1;
    const f2* const upP12 = reinterpret_cast<const f2*>(&sP12[upRow][lane * R]);
    const f2* const upP22 = reinterpret_cast<const f2*>(&sP22[upRow][lane * R]);
    const f2* const dnU1 = reinterpret_cast<const f2*>(&sU1[dnRow][lane * R]);
    const f2* const dnU2 = reinterpret_cast<const f2*>(&sU2[dnRow][lane * R]);

    for (int i = threadIdx.x; i < TW; i += NW * 64) sP12[NG + 1][i] = sP22[NG + 1][i] = sU1[NG + 1][i] = sU2[NG + 1][i] = 0.0f;
#pragma clang loop unroll(full)
    for (int j = 0; j < RP; ++j) {
        rowP12[j] = p12[C - 1][j];
        rowP22[j] = p22[C - 1][j];
    }
    __syncthreads();

    for (int k = 0; k < K; ++k) {
        // ---- phase A: u <- TH(u) + theta * div p   (p of the left and upper neighbours)
        // The IPOL border rules of the divergence need no selects: the left neighbour of x = 0 and
        // the upper neighbour of y = 0 arrive as 0 (DPP bound_ctrl / wave 0), and p11 at x = w-1,
        // p12 at y = h-1 are identically 0 (their forward differences are masked in phase B), so
        // p - neighbour reproduces {p, -neighbour, p - neighbour} exactly.
        f2 A12[RP], A22[RP];
#pragma clang loop unroll(full)
        for (int j = 0; j < RP; ++j) {
            A12[j] = upP12[j];
            A22[j] = upP22[j];
        }
        // Row order: row 0 needs the neighbour row fetched from LDS just above (its latency hides behind
        // row 1) and produces the row the group above waits for (stored right after it, so that the
        // store's latency hides behind rows 2.. before the barrier).
#pragma clang loop unroll(full)
        for (int cc = 0; cc < C; ++cc) {
            const int c = (C > 1 && cc < 2) ? 1 - cc : cc;
            // backward difference across the lane boundary: a plain subtraction, so that the compiler folds the lane shift
            // into it (one v_subrev_f32_dpp); in folded waves the first lane of a row group has no left neighbour in its
            // row: it keeps p itself (= p - 0, what the 0/1 multiplier lfix used to produce)
            float e11 = p11[c][0].x - dpp_from_left(p11[c][RP - 1].y), e21 = p21[c][0].x - dpp_from_left(p21[c][RP - 1].y);
            if constexpr (LX != 64) {
                e11 = lfix != 0.0f ? e11 : p11[c][0].x;
                e21 = lfix != 0.0f ? e21 : p21[c][0].x;
            }
#pragma clang loop unroll(full)
            for (int j = 0; j < RP; ++j) {
                // backward x differences in the interleaved layout (pack 0 = E = pixels x0, x0+2; pack 1 = O = x0+1,
                // x0+3): O - E is one packed subtract; E needs the left lane's last pixel and O.x: two v_sub_f32
                const f2 dx11 = j == 0 ? f2{e11, sub_s(p11[c][0].y, p11[c][1].x)} : p11[c][1] - p11[c][0];
                const f2 dx21 = j == 0 ? f2{e21, sub_s(p21[c][0].y, p21[c][1].x)} : p21[c][1] - p21[c][0];
                const f2 a12 = c > 0 ? p12[c > 0 ? c - 1 : 0][j] : A12[j];
                const f2 a22 = c > 0 ? p22[c > 0 ? c - 1 : 0][j] : A22[j];
                const f2 div1 = dx11 + (p12[c][j] - a12);
                const f2 div2 = dx21 + (p22[c][j] - a22);
                const f2 rho = pk_fma(wy[c][j], u2[c][j], pk_fma(wx[c][j], u1[c][j], rc[c][j]));
                const f2 t = -rho * ig[c][j];
                const f2 fi = f2{__builtin_amdgcn_fmed3f(t.x, -l_t, l_t), __builtin_amdgcn_fmed3f(t.y, -l_t, l_t)};
                const f2 v1 = pk_fma(fi, wx[c][j], u1[c][j]);
                const f2 v2 = pk_fma(fi, wy[c][j], u2[c][j]);
                const f2 n1 = pk_fma(theta, div1, v1);
                const f2 n2 = pk_fma(theta, div2, v2);
                if constexpr (EPS) {
                    const int y = y0 + c, x = x0 + j;  // pack j holds pixels x and x + 2
                    const f2 e1 = n1 - u1[c][j], e2 = n2 - u2[c][j];
                    const f2 e = pk_fma(e2, e2, e1 * e1);
                    if (y >= vy0 && y < vy1) {
                        if (x >= vx0 && x < vx1) qsum += (unsigned long long)(fminf(e.x, 1024.0f) * 4294967296.0f);
                        if (x + 2 >= vx0 && x + 2 < vx1) qsum += (unsigned long long)(fminf(e.y, 1024.0f) * 4294967296.0f);
                    }
                }
                u1[c][j] = n1;
                u2[c][j] = n2;
            }
            if (c == 0) {
#pragma clang loop unroll(full)
                for (int j = 0; j < RP; ++j) {
                    rowU1[j] = u1[0][j];
                    rowU2[j] = u2[0][j];
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // keep rows in program order: bounds register pressure
        }
        __syncthreads();

        // ---- phase B: p <- (p + taut * grad u) / (1 + taut * |grad u|)   (right and lower neighbours)
        f2 B1[RP], B2[RP];
#pragma clang loop unroll(full)
        for (int j = 0; j < RP; ++j) {
            B1[j] = dnU1[j];
            B2[j] = dnU2[j];
        }
        // Row order 0 .. C-3, C-1, C-2: the last row needs the LDS fetch and produces the exchanged row
#pragma clang loop unroll(full)
        for (int cc = 0; cc < C; ++cc) {
            const int c = (C > 1 && cc >= C - 2) ? 2 * C - 3 - cc : cc;
            const float r1 = dpp_from_right(u1[c][0].x), r2 = dpp_from_right(u2[c][0].x);
#pragma clang loop unroll(full)
            for (int j = 0; j < RP; ++j) {
                // forward x differences: E's are O - E (packed); O's need E.y and the right lane's first pixel
                const f2 d1x = j == 0 ? u1[c][1] - u1[c][0] : f2{sub_s(u1[c][0].y, u1[c][1].x), r1 - u1[c][1].y};
                const f2 d2x = j == 0 ? u2[c][1] - u2[c][0] : f2{sub_s(u2[c][0].y, u2[c][1].x), r2 - u2[c][1].y};
                const f2 b1 = c < C - 1 ? u1[c < C - 1 ? c + 1 : 0][j] : B1[j];
                const f2 b2 = c < C - 1 ? u2[c < C - 1 ? c + 1 : 0][j] : B2[j];
                const f2 u1x = d1x * mx[j], u1y = (b1 - u1[c][j]) * my[c];
                const f2 u2x = d2x * mx[j], u2y = (b2 - u2[c][j]) * my[c];
                // |grad u|^2 + 2^-100 (S6): the regulariser rides in the first FMA
                const f2 s1 = pk_fma(u1y, u1y, pk_fma(u1x, u1x, splat(kSqrtReg)));
                const f2 s2 = pk_fma(u2y, u2y, pk_fma(u2x, u2x, splat(kSqrtReg)));
                f2 q1, q2;
                if constexpr (FAST) {  // 1-ulp hardware sqrt / rcp (va_tvl1_params.fast_math)
                    const f2 g1 = f2{__builtin_amdgcn_sqrtf(s1.x), __builtin_amdgcn_sqrtf(s1.y)};
                    const f2 g2 = f2{__builtin_amdgcn_sqrtf(s2.x), __builtin_amdgcn_sqrtf(s2.y)};
                    const f2 d1 = pk_fma(taut, g1, one), d2 = pk_fma(taut, g2, one);
                    q1 = f2{__builtin_amdgcn_rcpf(d1.x), __builtin_amdgcn_rcpf(d1.y)};
                    q2 = f2{__builtin_amdgcn_rcpf(d2.x), __builtin_amdgcn_rcpf(d2.y)};
                } else {
                    // exact contract: correctly rounded sqrt, ONE correctly rounded division per pixel
                    // (s >= 2^-100: inside sqrt_exact_pk's domain).
                    const f2 g1 = sqrt_exact_pk(s1), g2 = sqrt_exact_pk(s2);
                    const f2 d1 = pk_fma(taut, g1, one), d2 = pk_fma(taut, g2, one);
                    const f2 rinv = rcp_exact_pk(d1 * d2);
                    q1 = d2 * rinv;
                    q2 = d1 * rinv;
                }
                p11[c][j] = pk_fma(taut, u1x, p11[c][j]) * q1;
                p12[c][j] = pk_fma(taut, u1y, p12[c][j]) * q1;
                p21[c][j] = pk_fma(taut, u2x, p21[c][j]) * q2;
                p22[c][j] = pk_fma(taut, u2y, p22[c][j]) * q2;
            }
            if (c == C - 1) {
#pragma clang loop unroll(full)
                for (int j = 0; j < RP; ++j) {
                    rowP12[j] = p12[C - 1][j];
                    rowP22[j] = p22[C - 1][j];
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    }

    // ---- write back the tile's valid interior (the valid regions partition the image)
    const bool runok = x0 >= vx0 && x0 < vx1;
#pragma clang loop unroll(full)
    for (int c = 0; c < C; ++c) {
        const int y = y0 + c;
        if (runok && y >= vy0 && y < vy1 && y < h) {
            const size_t ro_ = (size_t)y * pitch;
            store_row<RP>(sout + ro_, x0, xlim, u1[c]);
            store_row<RP>(sout + a.plane + ro_, x0, xlim, u2[c]);
            store_row<RP>(sout + 2 * a.plane + ro_, x0, xlim, p11[c]);
            store_row<RP>(sout + 3 * a.plane + ro_, x0, xlim, p12[c]);
            store_row<RP>(sout + 4 * a.plane + ro_, x0, xlim, p21[c]);
            store_row<RP>(sout + 5 * a.plane + ro_, x0, xlim, p22[c]);
        }
    }
    if constexpr (EPS) {
        if (qsum) atomicAdd(&sErr, qsum);
        __syncthreads();
        if (threadIdx.x == 0 && sErr) atomicAdd(&a.err[(size_t)pair * a.iters + a.it], sErr);
    }
}

// ---------------------------------------------------------------- rows of N pixels per lane ---
// A lane's N consecutive pixels of one field as N/2 packed pairs + a scalar tail: the arithmetic of the row pipeline
// (k_iter_stream, N = 2) is written once over these; pairs issue as v_pk_*_f32, the tail as plain VALU -- element by
// element the same IEEE operations, so results do not depend on N.
template <int N>
struct Row {
    static constexpr int NP = N / 2, NT = N & 1;
    f2 p[NP > 0 ? NP : 1];
    float t;
};
template <int N>
__device__ __forceinline__ Row<N> row_splat(float v)
{
    Row<N> r;
#pragma clang loop unroll(full)
    for (int j = 0; j < Row<N>::NP; ++j) r.p[j] = splat(v);
    r.t = v;
    return r;
}
template <int N>
__device__ __forceinline__ float row_get(const Row<N>& r, int i)
{
    return i < 2 * Row<N>::NP ? ((i & 1) ? r.p[i >> 1].y : r.p[i >> 1].x) : r.t;
}
template <int N>
__device__ __forceinline__ void row_set(Row<N>& r, int i, float v)
{
    if (i < 2 * Row<N>::NP) {
        if (i & 1) r.p[i >> 1].y = v;
        else r.p[i >> 1].x = v;
    } else {
        r.t = v;
    }
}
#define VA_ROW_OP(NAME, ARGS, PK, SC)                                   \
    template <int N>                                                    \
    __device__ __forceinline__ Row<N> NAME ARGS                         \
    {                                                                   \
        Row<N> r;                                                       \
        _Pragma("clang loop unroll(full)") for (int j = 0; j < Row<N>::NP; ++j) r.p[j] = PK; \
        r.t = 0.0f;                                                     \
        if constexpr (Row<N>::NT) r.t = SC;                             \
        return r;                                                       \
    }
VA_ROW_OP(r_fma, (const Row<N>& a, const Row<N>& b, const Row<N>& c), pk_fma(a.p[j], b.p[j], c.p[j]), fmaf(a.t, b.t, c.t))
VA_ROW_OP(r_fma_s, (float s, const Row<N>& b, const Row<N>& c), pk_fma(splat(s), b.p[j], c.p[j]), fmaf(s, b.t, c.t))
VA_ROW_OP(r_fma_c, (const Row<N>& a, const Row<N>& b, float c), pk_fma(a.p[j], b.p[j], splat(c)), fmaf(a.t, b.t, c))
VA_ROW_OP(r_mul, (const Row<N>& a, const Row<N>& b), a.p[j] * b.p[j], a.t * b.t)
VA_ROW_OP(r_mul_s, (const Row<N>& a, float s), a.p[j] * splat(s), a.t * s)
VA_ROW_OP(r_negmul, (const Row<N>& a, const Row<N>& b), -a.p[j] * b.p[j], -a.t * b.t)
VA_ROW_OP(r_add, (const Row<N>& a, const Row<N>& b), a.p[j] + b.p[j], a.t + b.t)
VA_ROW_OP(r_sub, (const Row<N>& a, const Row<N>& b), a.p[j] - b.p[j], a.t - b.t)
VA_ROW_OP(r_med3, (const Row<N>& a, float lo, float hi),
          (f2{__builtin_amdgcn_fmed3f(a.p[j].x, lo, hi), __builtin_amdgcn_fmed3f(a.p[j].y, lo, hi)}), __builtin_amdgcn_fmed3f(a.t, lo, hi))
#undef VA_ROW_OP
// scalar twins of sqrt_exact_pk / rcp_exact_pk (the same operations on one element: bit-identical)
__device__ __forceinline__ float sqrt_exact_s(float s)
{
    const float y = __builtin_amdgcn_rsqf(s);
    const float g = s * y, h = y * 0.5f;
    const float d = fmaf(-g, g, s);
    return fmaf(d, h, g);
}
__device__ __forceinline__ float rcp_exact_s(float d)
{
    const float r = __builtin_amdgcn_rcpf(d);
    const float e = fmaf(-d, r, 1.0f);
    return fmaf(e, r, r);
}
template <int N, bool FAST>
__device__ __forceinline__ Row<N> r_sqrt(const Row<N>& s)
{
    Row<N> r;
#pragma clang loop unroll(full)
    for (int j = 0; j < Row<N>::NP; ++j)
        r.p[j] = FAST ? f2{__builtin_amdgcn_sqrtf(s.p[j].x), __builtin_amdgcn_sqrtf(s.p[j].y)} : sqrt_exact_pk(s.p[j]);
    r.t = 0.0f;
    if constexpr (Row<N>::NT) r.t = FAST ? __builtin_amdgcn_sqrtf(s.t) : sqrt_exact_s(s.t);
    return r;
}
template <int N, bool FAST>
__device__ __forceinline__ Row<N> r_rcp(const Row<N>& d)
{
    Row<N> r;
#pragma clang loop unroll(full)
    for (int j = 0; j < Row<N>::NP; ++j)
        r.p[j] = FAST ? f2{__builtin_amdgcn_rcpf(d.p[j].x), __builtin_amdgcn_rcpf(d.p[j].y)} : rcp_exact_pk(d.p[j]);
    r.t = 0.0f;
    if constexpr (Row<N>::NT) r.t = FAST ? __builtin_amdgcn_rcpf(d.t) : rcp_exact_s(d.t);
    return r;
}
// backward / forward x differences of a lane's N consecutive pixels; the neighbour lane supplies the pixel across the
// lane boundary (0 beyond the wave's ends: the divergence's border rule on the left, masked by mx on the right)
template <int N>
__device__ __forceinline__ Row<N> r_diff_back(const Row<N>& a)
{
    Row<N> d;
    d.t = 0.0f;
    float prev = dpp_from_left(row_get(a, N - 1));
#pragma clang loop unroll(full)
    for (int i = 0; i < N; ++i) {
        const float cur = row_get(a, i);
        row_set(d, i, i == 0 ? cur - prev : sub_s(cur, prev));  // plain across the lane boundary: folds into v_subrev_f32_dpp
        prev = cur;
    }
    return d;
}
template <int N>
__device__ __forceinline__ Row<N> r_diff_fwd(const Row<N>& a)
{
    Row<N> d;
    d.t = 0.0f;
    const float right = dpp_from_right(row_get(a, 0));
#pragma clang loop unroll(full)
    for (int i = 0; i < N; ++i)
        row_set(d, i, i < N - 1 ? sub_s(row_get(a, i + 1 < N ? i + 1 : 0), row_get(a, i)) : right - row_get(a, i));
    return d;
}

template <int PPL> struct RowIo;
template <> struct RowIo<2> {
    typedef unsigned V __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ V ld(__amdgpu_buffer_rsrc_t r, int vo, int so) { return __builtin_amdgcn_raw_buffer_load_b64(r, vo, so, 0); }
    static __device__ __forceinline__ void st(V v, __amdgpu_buffer_rsrc_t r, int vo, int so) { __builtin_amdgcn_raw_buffer_store_b64(v, r, vo, so, 0); }
};
template <int N>
__device__ __forceinline__ Row<N> row_load(__amdgpu_buffer_rsrc_t r, int vo, int so)
{
    const typename RowIo<N>::V v = RowIo<N>::ld(r, vo, so);
    Row<N> o;
    o.t = 0.0f;
#pragma clang loop unroll(full)
    for (int i = 0; i < N; ++i) row_set(o, i, __uint_as_float(v[i]));
    return o;
}
template <int N>
__device__ __forceinline__ void row_store(const Row<N>& o, __amdgpu_buffer_rsrc_t r, int vo, int so)
{
    typename RowIo<N>::V v;
#pragma clang loop unroll(full)
    for (int i = 0; i < N; ++i) v[i] = __float_as_uint(row_get(o, i));
    RowIo<N>::st(v, r, vo, so);
}


// ---------------------------------------------------------------- streaming inner iterations ---
//
// k_iter_stream: the same S6 arithmetic organised as a time-skewed pipeline along y ("3.5-D blocking").  One WAVE owns a
// strip of 128 columns (2 pixels per lane, plain row order) and a chunk of rows [a0, b0); it streams the rows of the
// strip top to bottom ONCE per launch and carries every row through K iterations on the way: level t (t = 0 .. K-1)
// turns the time-t values of its incoming row into time-(t+1) values one row behind, so level t works on row
// (s - t) at step s.  A level keeps only ONE row of p (its row above) and one row of the new u (waiting for its row
// below) in registers: 12 VGPRs per level, 120 for K = 10.  The per-warp constants of the K rows in flight sit in a
// private LDS ring (each lane reads back only what it wrote: no barrier anywhere in the kernel).
// Against k_iter_tile's overlapped tiles (halo K on four sides: 2.0x redundant work on the 224^2 level) a strip pays
// the halo only in x where the level is wider than 128 columns and a triangular K(K+1) level-rows per chunk in y.
struct StreamArgs {
    const float* ro;
    const float* sin;
    float* sout;
    size_t plane;
    int w, h, pitch;
    int nsx, nch, R, HX;  // strips per row, chunks per column, rows per chunk, x halo of interior strip edges
    int K;                // iterations in this launch (<= KS)
    int pair0, rev;
    float l_t, taut, theta;
    // narrow = 1: the last strip of a row needs at most 64 columns (32 lanes), so that ONE wave carries the last strips of TWO
    // consecutive pairs, pair 2c in its lanes 0..31 and pair 2c + 1 in its lanes 32..63 (the 143^2 level: 128 + 64 lane-columns
    // per row instead of 2 x 128).  What crosses the lane 31 | 32 boundary is the left halo of the one and columns beyond the
    // image of the other.  The grid then is ((2 nsx - 1) x nch, couples of pairs); npairs: pairs of this launch.
    int narrow, npairs;
};

// KH levels per wave, NWV waves per workgroup.  NWV = 1: the wave is the whole pipeline (K <= KH iterations per pass).
// NWV = 2: the second wave continues where the first stops -- it takes the rows that leave the first wave's level
// KH-1 out of a double-buffered LDS row instead of HBM and carries them through levels KH .. 2KH-1, so that one pass
// over the strip is worth K <= 2 KH iterations of HBM traffic; both waves share the ring of per-warp constants; one
// workgroup barrier per step keeps them a step apart.
// PPL pixels per lane: a strip is 64 * PPL columns wide.  Only PPL = 2 (128 columns) is instantiated.
// NCH chains per wave: the KH levels of a wave cut into NCH chains of KC = KH / NCH consecutive levels; inside a chain
// level t + 1 consumes what level t emits in the SAME step, from one chain to the next the row waits in registers for one
// step (a latch), so that every chain end costs one step of pipeline depth: global level g works at pipeline position
// pos(g) = g + (chain ends before g).  Only NCH = 1 is instantiated (one chain: no latch, pos(g) = g + waves before g).
// These two parameters served kernel forms that measured slower and were removed.  They stay in
// stream_job because taking either out changes the register allocation of the one-wave form (234 -> 203 registers, more
// moves), which then measures 1-3 % slower; the parameters of the several-jobs-per-workgroup form went without that cost.
template <int KH, int NCH>
struct StreamShape {
    static_assert(KH % NCH == 0, "the levels of a wave are cut into chains of equal length");
    static constexpr int KC = KH / NCH;      // levels per chain
    static constexpr int SPAN = KH + NCH;    // pipeline positions a wave occupies (its levels + its chain ends)
    static constexpr int lpos(int t) { return t + t / KC; }  // position of the wave's level t behind the wave's first level
};
// rows of per-warp constants the LDS ring holds: the oldest row a level reads at step s is s - (its pipeline position)
// (three and four waves: the LAST level of the last wave takes the constants its neighbour level read one step earlier --
// the same row -- out of registers, so that the ring's oldest row is never read: one row less, which is what lets three
// 4 x 4 workgroups share a CU's 160 KB)
template <int KH, int NWV, int NCH>
constexpr bool stream_keep_last() { return NWV >= 3 && NCH == 1 && KH >= 2; }
template <int KH, int NWV, int NCH>
constexpr int stream_ring_rows() { return NWV == 1 ? KH + NCH - 2 : NWV * (KH + NCH) - 2 - (stream_keep_last<KH, NWV, NCH>() ? 1 : 0); }

// Forms that have a second copy of the pipeline without the right-border multiplier (stream_job, MX1): 4 x 4 and 4 x 3.
// The copy doubles a form's code and leaves its registers as they are.  4 x 5 measured no gain from it (179^2 equal,
// 143^2 1 % slower: both copies of its 22 KB of steady loops run side by side on a CU); the one- and two-wave fallback
// forms stay on one body.
template <int KH, int NWV>
constexpr bool kStreamMx1 = NWV >= 3 && KH <= 4;

template <int PPL>
struct StreamRow {  // the six state fields of one row of a strip
    Row<PPL> u1, u2, p11, p12, p21, p22;
};

template <int PPL, int KH, int NWV, bool FAST, int NCH = 1>
__device__ __forceinline__ void stream_job(const StreamArgs& a, const int pair, const int job, const int K,
                                           const float* __restrict__ sin_all, float* __restrict__ sout_all, const int half = 0)
{   // half: 0 = a whole-wave strip of `pair`; 1 = the shared last strip of `pair` (lanes 0..31) and `pair + 1` (lanes 32..63);
    // 2 = the same without a second pair (lanes 32..63 idle)
    typedef Row<PPL> R;
    typedef StreamRow<PPL> SR;
    typedef StreamShape<KH, NCH> SH;
    constexpr int NP = R::NP, NT = R::NT, SW = 64 * PPL, KC = SH::KC;
    // ring rows: NWV = 1: level t >= 1 reads row s - lpos(t), row s is written at the end of step s.  NWV = 2: the first
    // wave writes row s - 1 at the start of step s (after the barrier), the oldest row read in step s is
    // s - (NWV * SPAN - 2), whose slot is that of row s (written in step s + 1).
    constexpr int NRING = stream_ring_rows<KH, NWV, NCH>() > 0 ? stream_ring_rows<KH, NWV, NCH>() : 1;
    // A lane's fields sit side by side in 16-byte units -- ring: (wx, wy), (rc, ig); hand-over: (u1, u2), (p11, p12),
    // (p21, p22) -- so that every access is one ds_read_b128 / ds_write_b128; consecutive lanes lie 16 bytes apart
    // (no bank conflicts), the sizes are those of field-by-field arrays
    typedef float f4 __attribute__((ext_vector_type(4)));
    static_assert(kNF_RO % 2 == 0 && kNF_STATE % 2 == 0, "fields pair up into 16-byte units");
    __shared__ f4 ringP[NRING][kNF_RO / 2][NP][64];
    __shared__ float ringT[NRING][kNF_RO][NT ? 64 : 1];
    __shared__ f4 ifaceP[NWV > 1 ? NWV - 1 : 1][2][kNF_STATE / 2][NP][64];
    __shared__ float ifaceT[NWV > 1 ? NWV - 1 : 1][2][kNF_STATE][NT ? 64 : 1];

    const int sx = job % a.nsx, ch = job / a.nsx;
    const int w = a.w, h = a.h, pitch = a.pitch;
    const int lane = threadIdx.x & 63;
    const int wv = NWV == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ox = sx * (SW - 2 * a.HX);
    const int vx0 = ox + (sx > 0 ? a.HX : 0), vx1 = (sx == a.nsx - 1) ? pitch : ox + SW - a.HX;
    const int x0 = ox + PPL * (half ? (lane & 31) : lane);  // (the pitch, the halo and so every strip origin are multiples of PPL)
    const bool colok = x0 < pitch && !(half == 2 && lane >= 32);
    const bool stok = colok && x0 >= vx0 && x0 < vx1;
    const int a0 = ch * a.R, b0 = d_min(h, a0 + a.R);
    const int ys = d_max(0, a0 - K), ye = d_min(h, b0 + K);

    // buffer addressing: resource (scalar) + per-lane byte offset (one VGPR) + scalar plane/row offset.  Lanes beyond the
    // pitch read column 0 (finite values that no valid pixel can see: their differences are multiplied by mx = 0) and
    // never store.
    const int planeb = (int)(a.plane * sizeof(float)), pitchb = pitch * (int)sizeof(float);
    const int npr = half == 1 ? 2 : 1;  // pairs the resources span (the planes of consecutive pairs follow each other)
    const __amdgpu_buffer_rsrc_t rs_ro = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.ro + (size_t)pair * kNF_RO * a.plane), 0, npr * kNF_RO * planeb, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(sin_all + (size_t)pair * kNF_STATE * a.plane), 0, npr * kNF_STATE * planeb, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(sout_all + (size_t)pair * kNF_STATE * a.plane, 0,
                                                                           npr * kNF_STATE * planeb, 0x00020000);
    const bool second = half == 1 && lane >= 32;  // this lane works on pair + 1
    const int loff = colok ? x0 * (int)sizeof(float) + (second ? kNF_STATE * planeb : 0) : 0;     // state planes
    const int loff_ro = colok ? x0 * (int)sizeof(float) + (second ? kNF_RO * planeb : 0) : 0;     // per-warp constants

    R mx;
    mx.t = 0.0f;
#pragma clang loop unroll(full)
    for (int i = 0; i < PPL; ++i) row_set(mx, i, x0 + i < w - 1 ? 1.0f : 0.0f);
    const float l_t = a.l_t, taut = a.taut, theta = a.theta;
    const R zero = row_splat<PPL>(0.0f), one = row_splat<PPL>(1.0f);

    // one 16-byte unit: the fields f and f + 1 (f even) of a lane
    auto unit_put = [&](f4 (*u)[64], float (*t)[NT ? 64 : 1], int f, const R& v0, const R& v1) __attribute__((always_inline)) {
#pragma clang loop unroll(full)
        for (int j = 0; j < NP; ++j) u[j][lane] = f4{v0.p[j].x, v0.p[j].y, v1.p[j].x, v1.p[j].y};
        if constexpr (NT) {
            t[f][lane] = v0.t;
            t[f + 1][lane] = v1.t;
        }
    };
    auto unit_get = [&](const f4 (*u)[64], const float (*t)[NT ? 64 : 1], int f, R& v0, R& v1) __attribute__((always_inline)) {
#pragma clang loop unroll(full)
        for (int j = 0; j < NP; ++j) {
            const f4 q = u[j][lane];
            v0.p[j] = f2{q.x, q.y};
            v1.p[j] = f2{q.z, q.w};
        }
        v0.t = v1.t = 0.0f;
        if constexpr (NT) {
            v0.t = t[f][lane];
            v1.t = t[f + 1][lane];
        }
    };
    auto ring_put = [&](int slot, const R (&v)[kNF_RO]) __attribute__((always_inline)) {
#pragma clang loop unroll(full)
        for (int f = 0; f < kNF_RO; f += 2) unit_put(ringP[slot][f / 2], ringT[slot], f, v[f], v[f + 1]);
    };
    auto ring_get = [&](int slot, R (&v)[kNF_RO]) __attribute__((always_inline)) {
#pragma clang loop unroll(full)
        for (int f = 0; f < kNF_RO; f += 2) unit_get(ringP[slot][f / 2], ringT[slot], f, v[f], v[f + 1]);
    };
    auto if_put = [&](int wb, int b, const SR& v) __attribute__((always_inline)) {
        unit_put(ifaceP[wb][b][0], ifaceT[wb][b], 0, v.u1, v.u2);
        unit_put(ifaceP[wb][b][1], ifaceT[wb][b], 2, v.p11, v.p12);
        unit_put(ifaceP[wb][b][2], ifaceT[wb][b], 4, v.p21, v.p22);
    };
    auto if_get = [&](int wb, int b, SR& v) __attribute__((always_inline)) {
        unit_get(ifaceP[wb][b][0], ifaceT[wb][b], 0, v.u1, v.u2);
        unit_get(ifaceP[wb][b][1], ifaceT[wb][b], 2, v.p11, v.p12);
        unit_get(ifaceP[wb][b][2], ifaceT[wb][b], 4, v.p21, v.p22);
    };

    {
        const R zro[kNF_RO] = {zero, zero, zero, zero};
        for (int r = wv; r < NRING; r += NWV) ring_put(r, zro);
    }
    if constexpr (NWV > 1) {
        if (wv < NWV - 1) {  // wave w zeroes the hand-over rows it will write
            const SR zst{zero, zero, zero, zero, zero, zero};
            if_put(wv, 0, zst);
            if_put(wv, 1, zst);
        }
        __syncthreads();
    }

    auto ld = [&](const __amdgpu_buffer_rsrc_t& r, int f, int y) -> R { return row_load<PPL>(r, loff, f * planeb + y * pitchb); };
    auto ld_ro = [&](int f, int y) -> R { return row_load<PPL>(rs_ro, loff_ro, f * planeb + y * pitchb); };
    auto st = [&](const R& v, int f, int y) { row_store<PPL>(v, rs_out, loff, f * planeb + y * pitchb); };

    // the last valid row b0 - 1 leaves the last ACTIVE level (K - 1) when row b0 (or the dummy row h) comes in, and then
    // waits one step at every chain end on its way to the last wave's output: NWV * NCH - 1 of them
    const int nsteps = b0 - ys + K + (NWV * NCH - 1);

    // MX1: no lane of the strip holds the image's last column or a column beyond it (mx = 1 in every lane): the x
    // differences need no multiplier (x * 1 = x exactly)
    auto run = [&](auto wave_tag, auto mx1_tag) __attribute__((always_inline)) {
        constexpr int W = decltype(wave_tag)::value;
        constexpr bool MX1 = decltype(mx1_tag)::value;
        constexpr bool FIRST = W == 0, LAST = W == NWV - 1;
        constexpr int G0 = W * KH, LAG = W * SH::SPAN;  // first level of this wave; steps it runs behind the first wave

        R P11[KH], P12[KH], P21[KH], P22[KH], U1[KH], U2[KH];
#pragma clang loop unroll(full)
        for (int t = 0; t < KH; ++t) P11[t] = P12[t] = P21[t] = P22[t] = U1[t] = U2[t] = zero;
        SR latch[NCH > 1 ? NCH - 1 : 1];  // what chain c emitted in the previous step: chain c + 1's input of this one
#pragma clang loop unroll(full)
        for (int c = 0; c < (NCH > 1 ? NCH - 1 : 1); ++c) latch[c] = SR{zero, zero, zero, zero, zero, zero};
        R nst[kNF_STATE], nro[kNF_RO], rprev[kNF_RO] = {zero, zero, zero, zero};
        constexpr bool KEEP = LAST && stream_keep_last<KH, NWV, NCH>();
        R keep[kNF_RO] = {zero, zero, zero, zero};  // KEEP: the constants level KH - 2 worked with in the previous step = level KH - 1's of this one
#pragma clang loop unroll(full)
        for (int f = 0; f < kNF_STATE; ++f) nst[f] = FIRST ? ld(rs_in, f, ys) : zero;
#pragma clang loop unroll(full)
        for (int f = 0; f < kNF_RO; ++f) nro[f] = FIRST ? ld_ro(f, ys) : zero;

        // One level: phase A on the incoming row C (k_iter_tile's arithmetic, operation for operation), phase B on the
        // row above it (whose lower neighbour is the row just computed); the level keeps the incoming p and the new u,
        // and passes on (its old u, the new p) = the time-(t+1) values of the row above.
        // MY1: the row the level holds is not the image's last one (my = 1): its y differences need no multiplier
        // (x * 1 = x exactly; the straight-line steady-state steps use this form)
        auto level = [&](int t, SR& c, const R& wx, const R& wy, const R& rc, const R& ig, const float my, auto my1_tag) __attribute__((always_inline)) {
            constexpr bool MY1 = decltype(my1_tag)::value;
            // (the difference across the lane boundary is a plain subtraction inside r_diff_*: the compiler folds the
            // lane shift into it -- one v_subrev_f32_dpp instead of v_mov_b32_dpp + v_sub_f32)
            const R dx11 = r_diff_back(c.p11), dx21 = r_diff_back(c.p21);
            const R div1 = r_add(dx11, r_sub(c.p12, P12[t]));
            const R div2 = r_add(dx21, r_sub(c.p22, P22[t]));
            const R rho = r_fma(wy, c.u2, r_fma(wx, c.u1, rc));
            const R tt = r_negmul(rho, ig);
            const R fi = r_med3(tt, -l_t, l_t);
            const R v1 = r_fma(fi, wx, c.u1);
            const R v2 = r_fma(fi, wy, c.u2);
            const R n1 = r_fma_s(theta, div1, v1);
            const R n2 = r_fma_s(theta, div2, v2);
            const R d1x = r_diff_fwd(U1[t]), d2x = r_diff_fwd(U2[t]);
            const R u1x = MX1 ? d1x : r_mul(d1x, mx), u1y = MY1 ? r_sub(n1, U1[t]) : r_mul_s(r_sub(n1, U1[t]), my);
            const R u2x = MX1 ? d2x : r_mul(d2x, mx), u2y = MY1 ? r_sub(n2, U2[t]) : r_mul_s(r_sub(n2, U2[t]), my);
            const R s1 = r_fma(u1y, u1y, r_fma_c(u1x, u1x, kSqrtReg));
            const R s2 = r_fma(u2y, u2y, r_fma_c(u2x, u2x, kSqrtReg));
            const R d1 = r_fma_s(taut, r_sqrt<PPL, FAST>(s1), one);
            const R d2 = r_fma_s(taut, r_sqrt<PPL, FAST>(s2), one);
            R q1, q2;
            if constexpr (FAST) {
                q1 = r_rcp<PPL, true>(d1);
                q2 = r_rcp<PPL, true>(d2);
            } else {
                const R rinv = r_rcp<PPL, false>(r_mul(d1, d2));
                q1 = r_mul(d2, rinv);
                q2 = r_mul(d1, rinv);
            }
            const R o11 = r_mul(r_fma_s(taut, u1x, P11[t]), q1);
            const R o12 = r_mul(r_fma_s(taut, u1y, P12[t]), q1);
            const R o21 = r_mul(r_fma_s(taut, u2x, P21[t]), q2);
            const R o22 = r_mul(r_fma_s(taut, u2y, P22[t]), q2);
            const R ou1 = U1[t], ou2 = U2[t];
            P11[t] = c.p11;
            P12[t] = c.p12;
            P21[t] = c.p21;
            P22[t] = c.p22;
            U1[t] = n1;
            U2[t] = n2;
            c.u1 = ou1;
            c.u2 = ou2;
            c.p11 = o11;
            c.p12 = o12;
            c.p21 = o21;
            c.p22 = o22;
        };

        auto step = [&](const int s, auto steady_tag) __attribute__((always_inline)) {
            constexpr bool STEADY = decltype(steady_tag)::value;
            const int s0 = s % NRING;  // row s of the strip lives in ring slot s % NRING
            SR cc[NCH];                // the row travelling through chain c in this step
            R r0[kNF_RO] = {zero, zero, zero, zero};
            if constexpr (FIRST) {
                cc[0] = SR{nst[0], nst[1], nst[2], nst[3], nst[4], nst[5]};
#pragma clang loop unroll(full)
                for (int f = 0; f < kNF_RO; ++f) r0[f] = nro[f];
                // next row (beyond the last row of the strip: row ye - 1 again -- finite values nobody uses, or, at the
                // image bottom, the dummy row h whose only consumer multiplies its difference by my = 0)
                const int rn = d_min(ys + s + 1, ye - 1);
#pragma clang loop unroll(full)
                for (int f = 0; f < kNF_STATE; ++f) nst[f] = ld(rs_in, f, rn);
#pragma clang loop unroll(full)
                for (int f = 0; f < kNF_RO; ++f) nro[f] = ld_ro(f, rn);
                if constexpr (NWV > 1) {  // the constants of row s - 1 go into the ring now that the barrier has passed
                    const int sl = s0 == 0 ? NRING - 1 : s0 - 1;
                    ring_put(sl, rprev);
                }
                __builtin_amdgcn_sched_barrier(0);  // the loads stay at the top of the step: a whole step hides their latency
            } else {
                const int bsel = (s + 1) & 1;  // what the wave before wrote in step s - 1
                if_get(W - 1, bsel, cc[0]);
            }
#pragma clang loop unroll(full)
            for (int c = 1; c < NCH; ++c) cc[c] = latch[c - 1];
            // ring slot of the constants of level t's incoming row, s - LAG - lpos(t)
            auto slot_of = [&](int t) {
                const int c = (LAG + SH::lpos(t)) % NRING;
                return s0 - c < 0 ? s0 - c + NRING : s0 - c;
            };
            if constexpr (STEADY) {
                // every level of the wave works and no row is the image's last: straight-line code.  The levels are
                // issued round by round -- round i = level i of every chain, independent of each other -- and the
                // constants of round i + 1 are fetched from the ring while round i computes
                R q[NCH][kNF_RO];
#pragma clang loop unroll(full)
                for (int c = 0; c < NCH; ++c) {
                    if (FIRST && c == 0) {
#pragma clang loop unroll(full)
                        for (int f = 0; f < kNF_RO; ++f) q[c][f] = r0[f];
                    } else {
                        ring_get(slot_of(c * KC), q[c]);
                    }
                }
#pragma clang loop unroll(full)
                for (int i = 0; i < KC; ++i) {
                    R nq[NCH][kNF_RO];
#pragma clang loop unroll(full)
                    for (int c = 0; c < NCH; ++c)
#pragma clang loop unroll(full)
                        for (int f = 0; f < kNF_RO; ++f) nq[c][f] = zero;
                    if (i + 1 < KC) {
#pragma clang loop unroll(full)
                        for (int c = 0; c < NCH; ++c) {
                            if (KEEP && i + 1 == KH - 1) {  // (NCH == 1) the last level: the row level KH - 2 had one step ago
#pragma clang loop unroll(full)
                                for (int f = 0; f < kNF_RO; ++f) nq[c][f] = keep[f];
                            } else {
                                ring_get(slot_of(c * KC + i + 1), nq[c]);
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (KEEP && i == KH - 2) {
#pragma clang loop unroll(full)
                        for (int f = 0; f < kNF_RO; ++f) keep[f] = q[0][f];
                    }
#pragma clang loop unroll(full)
                    for (int c = 0; c < NCH; ++c) level(c * KC + i, cc[c], q[c][0], q[c][1], q[c][2], q[c][3], 1.0f, std::true_type{});
#pragma clang loop unroll(full)
                    for (int c = 0; c < NCH; ++c)
#pragma clang loop unroll(full)
                        for (int f = 0; f < kNF_RO; ++f) q[c][f] = nq[c][f];
                }
            } else {
#pragma clang loop unroll(full)
                for (int t = 0; t < KH; ++t) {
                    // global level g takes the rows [a0 - (K - g), b0 + (K - g)) of the image and, at the image bottom,
                    // the dummy row h
                    const int g = G0 + t, rin = ys + s - LAG - SH::lpos(t);
                    const int lo = d_max(0, a0 - (K - g)), hi = d_min(h, b0 + (K - g) - 1);
                    const bool act = g < K && rin >= lo && rin <= hi;
                    if (act) {
                        const float my = rin - 1 < h - 1 ? 1.0f : 0.0f;
                        if (FIRST && t == 0) {
                            level(0, cc[0], r0[0], r0[1], r0[2], r0[3], my, std::false_type{});
                        } else if (KEEP && t == KH - 1) {
                            level(t, cc[t / KC], keep[0], keep[1], keep[2], keep[3], my, std::false_type{});
                        } else {
                            R q[kNF_RO];
                            ring_get(slot_of(t), q);
                            level(t, cc[t / KC], q[0], q[1], q[2], q[3], my, std::false_type{});
                        }
                    }
                }
                if constexpr (KEEP) {  // whether or not level KH - 2 worked in this step: the row it stands at is level KH - 1's next one
                    ring_get(slot_of(KH - 2), keep);
                }
            }
#pragma clang loop unroll(full)
            for (int c = 0; c + 1 < NCH; ++c) latch[c] = cc[c];
            const SR& co = cc[NCH - 1];
            if constexpr (LAST) {
                // the row that leaves the pipeline in this step: K iterations on, one step later per chain end on its way
                const int rout = ys + s - K - (NWV * NCH - 1);
                if (stok && rout >= a0 && rout < b0) {
                    st(co.u1, 0, rout);
                    st(co.u2, 1, rout);
                    st(co.p11, 2, rout);
                    st(co.p12, 3, rout);
                    st(co.p21, 4, rout);
                    st(co.p22, 5, rout);
                }
            } else {
                if_put(W, s & 1, co);
            }
            if constexpr (FIRST) {
                if constexpr (NWV == 1) {
                    ring_put(s0, r0);
                } else {
#pragma clang loop unroll(full)
                    for (int f = 0; f < kNF_RO; ++f) rprev[f] = r0[f];
                }
            }
            // hand-over barrier: LDS traffic only (no wait for the global loads in flight or the stores just issued)
            if constexpr (NWV > 1) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        };
        // steady state of this wave: the steps in which all its KH levels are inside their row windows and below the
        // image's last row -- level t (global g) takes row ys + s - LAG - lpos(t), its window is [lo_g, min(hi_g, h - 1)]
        int s_a = 0, s_b = nsteps;
#pragma clang loop unroll(full)
        for (int t = 0; t < KH; ++t) {
            const int g = G0 + t, p = LAG + SH::lpos(t) - ys;
            s_a = d_max(s_a, d_max(0, a0 - (K - g)) + p);
            s_b = d_min(s_b, d_min(h - 1, d_min(h, b0 + (K - g) - 1)) + p + 1);
        }
        if (K < G0 + KH || s_a > s_b) s_a = s_b = 0;
        int s = 0;
        for (; s < s_a; ++s) step(s, std::false_type{});
        // two steady steps per loop trip: the rows a level hands on and keeps (c_* -> P[t], n -> U[t]) change registers
        // by renaming between the two copies instead of by v_mov (5 per level and step otherwise; measured on the 224^2
        // level: 9.8 -> 9.3 ms per warp step of 320 pairs).  Not in the one-wave form: with ten levels in one wave's 256
        // registers the second copy spills (19-21 registers; 1280x720: 62 instead of 114 pairs/s)
        if constexpr (NWV > 1)
            for (; s + 1 < s_b; s += 2) {
                step(s, std::true_type{});
                step(s + 1, std::true_type{});
            }
        for (; s < s_b; ++s) step(s, std::true_type{});
        for (; s < nsteps; ++s) step(s, std::false_type{});
    };
    auto waves = [&](auto mx1_tag) __attribute__((always_inline)) {
        if constexpr (NWV == 1) {
            run(std::integral_constant<int, 0>{}, mx1_tag);
        } else if constexpr (NWV == 2) {
            if (wv == 0) run(std::integral_constant<int, 0>{}, mx1_tag);
            else run(std::integral_constant<int, NWV - 1>{}, mx1_tag);
        } else if constexpr (NWV == 3) {
            if (wv == 0) run(std::integral_constant<int, 0>{}, mx1_tag);
            else if (wv == 1) run(std::integral_constant<int, 1>{}, mx1_tag);
            else run(std::integral_constant<int, 2>{}, mx1_tag);
        } else {
            static_assert(NWV == 4, "pipelines of one to four waves");
            if (wv == 0) run(std::integral_constant<int, 0>{}, mx1_tag);
            else if (wv == 1) run(std::integral_constant<int, 1>{}, mx1_tag);
            else if (wv == 2) run(std::integral_constant<int, 2>{}, mx1_tag);
            else run(std::integral_constant<int, 3>{}, mx1_tag);
        }
    };
    // a strip that ends before the image's last column (never the last strip of a row, never a shared one) runs the copy
    // without the x multiplier; the choice is uniform over the workgroup and made once per job
    if constexpr (kStreamMx1<KH, NWV>) {
        if (half == 0 && ox + SW < w) waves(std::true_type{});
        else waves(std::false_type{});
    } else {
        waves(std::false_type{});
    }
}

// One launch = one pass (a.K iterations) of every pair of the call: the grid is (strips x chunks, pairs).
template <int PPL, int KH, int NWV, bool FAST, int NCH = 1>
__global__ void __launch_bounds__(NWV * 64)
    __attribute__((amdgpu_waves_per_eu(2, NWV >= 3 ? 4 : 2)))
    k_iter_stream(StreamArgs a)
{
    unsigned lid = blockIdx.y * gridDim.x + blockIdx.x;
    {
        const unsigned nb = gridDim.x * gridDim.y, q = nb / 8, r = nb % 8, xcd = lid % 8, kk = lid / 8;
        lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + kk;
        if (a.rev) lid = nb - 1 - lid;
    }
    if (!a.narrow) {
        stream_job<PPL, KH, NWV, FAST, NCH>(a, a.pair0 + (int)(lid / gridDim.x), (int)(lid % gridDim.x), a.K, a.sin, a.sout);
        return;
    }
    // shared last strips: per couple of pairs and chunk 2 (nsx - 1) whole-wave strips and ONE wave for both last strips
    const int couple = (int)(lid / gridDim.x), jx = (int)(lid % gridDim.x), per = 2 * a.nsx - 1;
    const int ch = jx / per, r = jx % per, first = 2 * couple;
    int which = 0, sx = a.nsx - 1, half = first + 1 < a.npairs ? 1 : 2;
    if (r < 2 * (a.nsx - 1)) {
        which = r / (a.nsx - 1);
        sx = r % (a.nsx - 1);
        half = 0;
        if (first + which >= a.npairs) return;  // an odd number of pairs: the last couple has no second one
    }
    stream_job<PPL, KH, NWV, FAST, NCH>(a, a.pair0 + first + which, ch * a.nsx + sx, a.K, a.sin, a.sout, half);
}

// ---------------------------------------------------------------- median of the flow (S55) ----
// u1 and u2 replaced by their KS x KS median (KS = 3, 5): window centred on the pixel, coordinates clamped to the
// frame, exact selection.  Out of place: k_median writes the filtered planes to scratch, k_median_store copies them
// back over the state, so that every sample is read from the values before the filter.
__device__ __forceinline__ void cswap(float& a, float& b)  // a <- min, b <- max
{
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo;
    b = hi;
}

// Forgetful selection.  Of M = live / 2 + 2 values out of `live` (odd) neither the smallest nor the largest can be
// the median of all: both leave, the median of the rest is the median sought, and one value not yet seen joins the M - 2
// that stay.  25 values: rounds of 14, 13, ..., 4 and a median of three; 9 values: 6, 5, 4.  A round orders pairs
// (w[2i] <= w[2i+1]), then carries the minimum of the lower halves to w[0] and the maximum of the upper ones to w[1]:
// 3M - 4 min/max, 253 for 25 values and 33 for 9.  Every index is a compile-time constant (the recursion is over
// template arguments): the arrays live in registers.
template <int M, int NEXT, int N, int M0>
__device__ __forceinline__ float median_round(float (&w)[M0], const float (&v)[N])
{
    if constexpr (M == 3) {
        static_assert(NEXT == N, "every value has been seen when three are left");
        return __builtin_amdgcn_fmed3f(w[0], w[1], w[2]);
    } else {
#pragma unroll
        for (int i = 0; i + 1 < M; i += 2) cswap(w[i], w[i + 1]);
#pragma unroll
        for (int i = 2; i < M; i += 2) cswap(w[0], w[i]);  // (M odd: the unpaired last value, index M - 1, is among these)
#pragma unroll
        for (int i = 3; i < M; i += 2) cswap(w[i], w[1]);
        if constexpr (M % 2 == 1) cswap(w[M - 1], w[1]);
        w[0] = v[NEXT];
        w[1] = w[M - 1];
        return median_round<M - 1, NEXT + 1, N, M0>(w, v);
    }
}
template <int N>
__device__ __forceinline__ float median_of(const float (&v)[N])
{
    constexpr int M0 = N / 2 + 2;
    float w[M0];
#pragma unroll
    for (int i = 0; i < M0; ++i) w[i] = v[i];
    return median_round<M0, M0, N, M0>(w, v);
}

struct MedianArgs {
    const float* srcA;  // fields to filter, [pair][src_nf][plane]; plane 0 = u1, plane 1 = u2 of a pair
    const float* srcB;  // the other ping-pong buffer (which of the two: `cur`, in epsilon mode base[pair] ^ (it & 1))
    float* dstA;        // [pair][dst_nf][plane]
    float* dstB;
    const int* base;                // epsilon mode (err != nullptr): as IterArgs
    const unsigned long long* err;
    unsigned long long qthr;
    size_t plane;
    int src_nf, dst_nf;
    int cur, it, iters;
    int w, h, pitch, perm, ntx, pair0;
};

constexpr int kMedTX = 64, kMedTY = 16, kMedRows = 4;  // tile of a workgroup of 64 x 4 threads; rows per thread

// The buffer of this launch's pair, or -1: the pair has met the stopping rule in this warp (the test of k_iter_tile<EPS>)
__device__ __forceinline__ int median_buffer(const MedianArgs& a, int pair)
{
    if (!a.err) return a.cur;
    if (a.it > 0 && a.err[(size_t)pair * a.iters + a.it - 1] < a.qthr) return -1;
    return a.base[pair] ^ (a.it & 1);
}

template <int KS>
__global__ void __launch_bounds__(kMedTX * (kMedTY / kMedRows)) k_median(MedianArgs a)
{
    constexpr int R = KS / 2, LW = kMedTX + 2 * R, LH = kMedTY + 2 * R, NT = kMedTX * (kMedTY / kMedRows);
    __shared__ float tile[LH][LW];
    const int pair = a.pair0 + blockIdx.y, f = blockIdx.z;
    const int which = median_buffer(a, pair);
    if (which < 0) return;  // (the same for the whole workgroup)
    const float* __restrict__ src = (which ? a.srcB : a.srcA) + ((size_t)pair * a.src_nf + f) * a.plane;
    float* __restrict__ dst = (which ? a.dstB : a.dstA) + ((size_t)pair * a.dst_nf + f) * a.plane;
    const int w = a.w, h = a.h, pitch = a.pitch, perm = a.perm;
    const int ox = (int)(blockIdx.x % a.ntx) * kMedTX, oy = (int)(blockIdx.x / a.ntx) * kMedTY;
    const int tid = threadIdx.y * kMedTX + threadIdx.x;
    for (int i = tid; i < LW * LH; i += NT) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gx = d_min(d_max(ox + lx - R, 0), w - 1), gy = d_min(d_max(oy + ly - R, 0), h - 1);
        tile[ly][lx] = src[(size_t)gy * pitch + pslot(gx, perm)];
    }
    __syncthreads();
    const int x = ox + threadIdx.x;
    if (x >= w) return;
    for (int j = 0; j < kMedRows; ++j) {
        const int ly = threadIdx.y * kMedRows + j, y = oy + ly;
        if (y >= h) break;
        float v[KS * KS];
#pragma unroll
        for (int dy = 0; dy < KS; ++dy)
#pragma unroll
            for (int dx = 0; dx < KS; ++dx) v[dy * KS + dx] = tile[ly + dy][threadIdx.x + dx];
        dst[(size_t)y * pitch + pslot(x, perm)] = median_of<KS * KS>(v);
    }
}

// scratch [pair][2][plane] -> u1, u2 of the state (columns x < w: the pitch padding of the state stays zero)
__global__ void k_median_store(MedianArgs a)
{
    const int pair = a.pair0 + blockIdx.y, f = blockIdx.z;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.w * a.h) return;
    const int which = median_buffer(a, pair);
    if (which < 0) return;
    const float* __restrict__ src = (which ? a.srcB : a.srcA) + ((size_t)pair * a.src_nf + f) * a.plane;
    float* __restrict__ dst = (which ? a.dstB : a.dstA) + ((size_t)pair * a.dst_nf + f) * a.plane;
    const int y = idx / a.w, x = idx - y * a.w;
    const size_t o = (size_t)y * a.pitch + pslot(x, a.perm);
    dst[o] = src[o];
}

dim3 median_grid(const MedianArgs& a, int npairs) { return dim3(a.ntx * va_cdiv(a.h, kMedTY), npairs, 2); }
void launch_median(int ksize, const MedianArgs& a, int npairs, hipStream_t st)
{
    const dim3 grid = median_grid(a, npairs), block(kMedTX, kMedTY / kMedRows);
    if (ksize == 3) k_median<3><<<grid, block, 0, st>>>(a);
    else k_median<5><<<grid, block, 0, st>>>(a);
}

// ---------------------------------------------------------------- host side -------------------

struct TileCfg {
    int R, C, NW, LX;
};
// Candidate tilings (R, C, NW, LX): 256x32, 128x64, 84x96 and 64x128 tiles, 512 threads, a 4x4 pixel
// patch per thread (the packed-math kernel needs more than the 128 VGPRs a 1024-thread workgroup
// would leave it).  Every candidate costs the same time per workgroup-iteration.
constexpr TileCfg kCfgs[] = {{4, 4, 8, 64}, {4, 4, 8, 32}, {4, 4, 8, 21}, {4, 4, 8, 16},
                             {4, 4, 4, 64}, {4, 4, 4, 32}, {4, 4, 4, 21}, {4, 4, 4, 16}};
constexpr int kNumCfgs = (int)(sizeof(kCfgs) / sizeof(kCfgs[0]));

struct TilePick {
    int cfg, ntx, nty, HX, K;
};

// Cost of a workgroup in CU-microseconds, measured on MI355X (tools/bench_tvl1_levels.py,
// tools/microbench_tvl1_tile.py): exposed HBM round trip per launch + time per inner iteration.
// The 4-wave candidates (half-size tiles) run two workgroups per CU: one's load/store phase hides
// behind the other's arithmetic (a few us exposed per 4096-pixel tile instead of ~15 us per 8192) and
// the 4-wave barriers cost less (1.2 us per iteration instead of ~2.7 / 2).  The constants are fitted to the
// per-level optimum found by brute force with the cache-aware workgroup order in place (tools/sweep_tvl1_tiles.py).
double tile_launch_us(int cfg) { return kCfgs[cfg].NW == 8 ? 17.0 : 4.5; }
double tile_iter_us(int cfg)
{
    const double t = kCfgs[cfg].NW == 8 ? 2.75 : 1.2;
    return kCfgs[cfg].LX >= 32 ? t : 1.03 * t;  // 3- and 4-fold waves: a little slower
}
// A launch cannot beat the HBM stream of its tiles: 4.5 TB/s = 17.6 kB per us per CU (5.2 TB/s is the best this access pattern reaches).
double tile_hbm_us(int TW, int TH, int HX, int K) { return ((double)TW * TH * 40.0 + (double)(TW - 2 * HX) * (TH - 2 * K) * 24.0) / 17600.0; }
double tile_cost_us(int cfg, int HX, int K)
{
    const int TW = kCfgs[cfg].LX * kCfgs[cfg].R, TH = kCfgs[cfg].NW * (64 / kCfgs[cfg].LX) * kCfgs[cfg].C;
    const double c = tile_launch_us(cfg) + tile_iter_us(cfg) * K, m = tile_hbm_us(TW, TH, HX, K < TH / 2 ? K : 0);
    return c > m ? c : m;
}

int tiles_1d(int n, int T, int halo)
{
    if (n <= T) return 1;
    return va_cdiv(n - 2 * halo, T - 2 * halo);
}

// Pick the candidate with the lowest modelled cost per iteration for this level and K.
TilePick pick_tiles(int w, int h, int K, unsigned mask)
{
    if (!mask) mask = (1u << kNumCfgs) - 1;
    TilePick best{};
    double best_cost = 1e300;
    for (int i = 0; i < kNumCfgs; ++i) {
        if (!((mask >> i) & 1)) continue;
        const int R = kCfgs[i].R, TW = kCfgs[i].LX * R, TH = kCfgs[i].NW * (64 / kCfgs[i].LX) * kCfgs[i].C;
        int k = K;
        if (h > TH && 2 * k >= TH) k = (TH - 1) / 2 > 0 ? (TH - 1) / 2 : 1;
        const int align = 4;  // tile origins stay 16-byte aligned
        int HX = 0;
        if (w > TW) {
            HX = va_cdiv(k, align) * align;
            if (2 * HX >= TW) continue;
        }
        const int ntx = tiles_1d(w, TW, HX), nty = tiles_1d(h, TH, k);
        const double cost = (double)ntx * nty * tile_cost_us(i, HX, k) / k;
        if (cost < best_cost) {
            best_cost = cost;
            best = TilePick{i, ntx, nty, HX, k};
        }
    }
    if (best_cost == 1e300) return pick_tiles(w, h, K, 0u);  // no allowed candidate fits this halo: allow all
    return best;
}

// block_iters = 0: the depth K that minimises the modelled time of one warp's `iters` iterations
// (full launches of K plus one shorter launch for the remainder).
TilePick pick_tiles_auto(int w, int h, int iters, unsigned mask)
{
    TilePick best{};
    double best_cost = 1e300;
    for (int K = 1; K <= 31 && K <= iters; ++K) {
        const TilePick tp = pick_tiles(w, h, K, mask);
        if (tp.K != K) continue;
        const int full = iters / K, rem = iters - full * K;
        double cost = (double)full * tp.ntx * tp.nty * tile_cost_us(tp.cfg, tp.HX, K);
        if (rem) {
            const TilePick tr = pick_tiles(w, h, rem, mask);
            cost += (double)tr.ntx * tr.nty * tile_cost_us(tr.cfg, tr.HX, tr.K) * ((double)rem / tr.K);
        }
        if (cost < best_cost) {
            best_cost = cost;
            best = tp;
        }
    }
    return best;
}

dim3 iter_grid(const TilePick& tp, int npairs) { return dim3(tp.ntx * tp.nty, npairs); }
template <bool EPS, bool FAST>
void launch_iter(const TilePick& tp, const IterArgs& a, int npairs, hipStream_t st)
{
    const dim3 grid = iter_grid(tp, npairs);
    switch (tp.cfg) {
        case 0: k_iter_tile<2, 4, 8, 64, EPS, FAST><<<grid, 512, 0, st>>>(a); break;  // 256 x 32 tile
        case 1: k_iter_tile<2, 4, 8, 32, EPS, FAST><<<grid, 512, 0, st>>>(a); break;  // 128 x 64 (2 row groups per wave)
        case 2: k_iter_tile<2, 4, 8, 21, EPS, FAST><<<grid, 512, 0, st>>>(a); break;  // 84 x 96 (3 row groups, lane 63 idle)
        case 3: k_iter_tile<2, 4, 8, 16, EPS, FAST><<<grid, 512, 0, st>>>(a); break;  // 64 x 128 (4 row groups)
        case 4: k_iter_tile<2, 4, 4, 64, EPS, FAST><<<grid, 256, 0, st>>>(a); break;  // 256 x 16, two workgroups per CU
        case 5: k_iter_tile<2, 4, 4, 32, EPS, FAST><<<grid, 256, 0, st>>>(a); break;  // 128 x 32
        case 6: k_iter_tile<2, 4, 4, 21, EPS, FAST><<<grid, 256, 0, st>>>(a); break;  // 84 x 48
        default: k_iter_tile<2, 4, 4, 16, EPS, FAST><<<grid, 256, 0, st>>>(a); break; // 64 x 64
    }
}

// ---- k_iter_stream: strips x chunks of a level
constexpr int kStreamSW = 128;      // columns of a strip: 64 lanes x 2 pixels
constexpr int kStreamK1 = 10;       // one-wave pipeline: iterations per pass
constexpr int kStreamKH2 = 8;       // two-wave pipeline: levels per wave (16 iterations per pass)
constexpr int kStreamBit = 1 << 8;  // va_tvl1_params.tile_mask bit: iterate with k_iter_stream
constexpr int kRetiredRowsBit = 1 << 9;  // va_tvl1_params.tile_mask bit of a retired kernel family: refused (check_params)
constexpr int kNoNarrowBit = 1 << 10;  // va_tvl1_params.tile_mask bit: no shared last strips (StreamArgs.narrow) -- A/B and tests
struct StreamPick {
    int nsx, nch, R, HX;
    int nwv, kh;        // the pipeline of four waves x kh levels for the passes deep enough to end in its last wave; nwv = 0: none
    int fb_nwv, fb_kh;  // the fallback shape of every other pass: 2 x 8, or 1 x 10 (which also takes what is too short for 2 x 8)
    int narrow;         // the last strip of a row fits 32 lanes: two pairs' last strips share a wave (StreamArgs.narrow)
};
// stream_waves 7, 8, 9: pipelines of four waves (waves x levels per wave)
constexpr int kMwShapes[][2] = {{4, 4}, {4, 5}, {4, 3}};
constexpr int kNumMwShapes = (int)(sizeof(kMwShapes) / sizeof(kMwShapes[0]));
constexpr int kMwFirst = 7;
// One pass of the row pipeline in one of the five shapes (waves x levels per wave) that exist
int launch_stream(int nwv, int kh, bool fast, dim3 grid, hipStream_t st, const StreamArgs& sa)
{
    auto go = [&](auto nwv_tag, auto kh_tag) {
        constexpr int NWV = decltype(nwv_tag)::value, KH = decltype(kh_tag)::value;
        if (fast) k_iter_stream<2, KH, NWV, true><<<grid, NWV * 64, 0, st>>>(sa);
        else k_iter_stream<2, KH, NWV, false><<<grid, NWV * 64, 0, st>>>(sa);
        return VA_OK;
    };
    using std::integral_constant;
    if (nwv == 1 && kh == kStreamK1) return go(integral_constant<int, 1>{}, integral_constant<int, kStreamK1>{});
    if (nwv == 2 && kh == kStreamKH2) return go(integral_constant<int, 2>{}, integral_constant<int, kStreamKH2>{});
    if (nwv == 4 && kh == 3) return go(integral_constant<int, 4>{}, integral_constant<int, 3>{});
    if (nwv == 4 && kh == 4) return go(integral_constant<int, 4>{}, integral_constant<int, 4>{});
    if (nwv == 4 && kh == 5) return go(integral_constant<int, 4>{}, integral_constant<int, 5>{});
    va_set_error("va_tvl1: no row pipeline of %d waves x %d levels", nwv, kh);
    return VA_ERR_INVALID;
}
// Strips of a level and the shape of the pipeline that carries them (see the comment on the four-wave forms below).  The
// forms of rounds 1-2 remain as explicit choices and as fallbacks for passes too short for four waves: two waves x 8
// levels (16 iterations per pass) where the 16-column x halo costs no third strip (w <= 224), one wave x 10 levels
// (halo 10) on wider levels.  va_tvl1_params.stream_waves = 1: one wave everywhere; 2: these two.
void stream_strips(const va_tvl1_params* p, int w, StreamPick& sp)
{
    constexpr int SW = kStreamSW;
    const bool two = p->tuning[VA_TUNE_STREAM_WAVES] != 1 && tiles_1d(w, SW, 2 * kStreamKH2) <= 2;
    sp.fb_nwv = two ? 2 : 1;
    sp.fb_kh = two ? kStreamKH2 : kStreamK1;
    // (Also measured, round 2, and removed again: THREE waves of 4 / 5 levels each -- 12 / 15 iterations per pass at 144 /
    // 168 registers, i.e. three resident waves per SIMD instead of two: 45.2 / 43.9 ms on the 224^2 level and 35.3 / 34.8
    // on 179^2 against 41.6 / 32.9 for the two-wave form: more resident waves do not fill the idle issue slots.)
    sp.HX = sp.fb_nwv * sp.fb_kh;  // (16 or 10, even: strip origins stay multiples of the two pixels per lane)
    sp.nsx = tiles_1d(w, SW, sp.HX);
    // Pipelines of FOUR waves (round 3): 4 x 4 levels (16 iterations per pass, 143 registers: three waves per SIMD) or, where
    // a 20-column halo still costs no third strip, 4 x 5 levels (20 per pass, 167 registers).  Measured per level on the
    // benchmark's pyramid (320 pairs on two streams, ms per 5 x 300 iterations, against the two-wave form): 224^2 38.7 / 41.7
    // (4 x 4, whole columns per job), 179^2 28.4 / 33.5 (4 x 5), 114^2 12.4 / 14.4 (4 x 4, two chunks): four shallow waves
    // need a quarter of the strip x chunk jobs to fill the GPU, so that the levels are cut into fewer chunks of rows (each
    // chunk costs its halo rows and the pipeline's fill), and leave room for a third wave per SIMD.
    // Levels with more than two strips (the 1280x720 pyramid): 4 x 3 levels (12 per pass, halo 12, 119 registers: four waves
    // per SIMD, three workgroups per CU) -- 138 against 118 pairs/s for the one-wave form with 10 per pass (16 pairs).
    // stream_waves: 0 = this choice, 2 = two waves where they fit (rounds 1-2), 1 = one wave everywhere, 7 / 8 / 9 = 4 x 4 /
    // 4 x 5 / 4 x 3 wherever a strip keeps valid columns.
    const int sw = p->tuning[VA_TUNE_STREAM_WAVES];
    int shape = -1;
    if (sw >= kMwFirst && sw < kMwFirst + kNumMwShapes) shape = sw - kMwFirst;
    else if (sw == 0) shape = !two ? 2 : (w > SW && tiles_1d(w, SW, 20) <= 2) ? 1 : 0;
    if (shape >= 0) {
        const int nwv = kMwShapes[shape][0], kh = kMwShapes[shape][1], hx = va_cdiv(nwv * kh, 2) * 2;
        // the default choice: like the two-wave form only where the deeper x halo costs no third strip; an explicit
        // stream_waves >= 7 takes the shape wherever a strip keeps valid columns
        if (2 * hx < SW && (sw >= kMwFirst || !two || tiles_1d(w, SW, hx) <= 2)) {
            sp.nwv = nwv;
            sp.kh = kh;
            if (hx > sp.HX) sp.HX = hx;  // (a pass that falls back to the two-wave form runs with this halo too)
            sp.nsx = tiles_1d(w, SW, sp.HX);
            // the last strip starts at (nsx - 1) (SW - 2 HX); if the level (with its pitch padding) ends within 64 columns of
            // that, the strip is narrow (tile_mask bit 10: never)
            const int pitch4 = (w + 3) & ~3;
            sp.narrow = sp.nsx >= 2 && !(p->tile_mask & kNoNarrowBit) && (sp.nsx - 1) * (SW - 2 * sp.HX) + 64 >= pitch4;
        }
    }
}
StreamPick pick_stream(const va_tvl1_params* p, int w, int h, int npairs)
{
    StreamPick sp{};
    stream_strips(p, w, sp);
    // chunks of rows: the number of jobs (strip x chunk x pair) that keeps the GPU busiest was measured with one and
    // with two concurrent calls on different HIP streams: ~1024 one-wave jobs, ~640 two-wave jobs per call (256 CUs x
    // 8 waves); rows per chunk not below 32
    // (four-wave jobs: 320 per call on the levels of at most two strips -- 256 ... 400 measured equal, 480 and more 5 % slower
    // in the whole benchmark --, 1024 on the wide levels: 512 ... 1280 within 2 %, 2048 8 % slower)
    const int slots = p->tuning[VA_TUNE_STREAM_SLOTS] > 0 ? p->tuning[VA_TUNE_STREAM_SLOTS]
                      : sp.nwv ? (sp.nsx <= 2 ? 320 : 1024) : (sp.fb_nwv == 2 ? 640 : 1024);
    int nch = p->tuning[VA_TUNE_STREAM_CHUNKS];
    if (nch <= 0) nch = (int)((double)slots / ((double)npairs * sp.nsx) + 0.5);
    if (nch > h / 32) nch = h / 32;
    if (nch < 1) nch = 1;
    sp.R = va_cdiv(h, nch);
    sp.nch = va_cdiv(h, sp.R);
    return sp;
}
// Level (w, h) of the pyramid iterates with k_iter_stream: wherever its strips are well filled and the level is large
// enough for a GPU-full of strip x chunk jobs (measured, tools/bench_tvl1_levels.py).  tile_mask bit 8 forces it (tests);
// va_tvl1_params.stream_levels >= 0 is the explicit per-level choice (bit s = level s, 0 = never).
bool level_streams(const va_tvl1_params* p, bool eps, int s, int w, int h, size_t plane)
{
    if (eps || (double)plane * kNF_STATE * sizeof(float) >= 2147483648.0) return false;  // 32-bit buffer offsets
    if (p->tile_mask & kStreamBit) return true;
    if ((p->tile_mask & ~kNoNarrowBit) != 0) return false;
    if (p->tuning[VA_TUNE_STREAM_LEVELS] >= 0) return ((p->tuning[VA_TUNE_STREAM_LEVELS] >> s) & 1) != 0;
    if (p->tuning[VA_TUNE_ROWS_LEVELS] >= 0) return false;  // the reserved slot's 0 has always meant "explicit choice": tiles
    StreamPick sp{};
    stream_strips(p, w, sp);
    // measured per level of the 224x224 pyramid (320 pairs, two streams; profiles/README.md): the row pipeline wins on 224^2
    // (two strips 88 % full), 179^2 (70 %) and 114^2 (one strip, 89 %), the register tiles on 143^2 (56 %) and 91^2 (71 %
    // of one strip, too few jobs); every level of the 1280x720 pyramid (80..85 %) streams
    // (round 3: with the last strips of two pairs sharing a wave 143^2 fills 74 % of 1.5 strips: 18.9 ms against 21.6 on tiles)
    const double fill = (double)w / ((double)kStreamSW * (sp.nsx - (sp.narrow ? 0.5 : 0.0))), px = (double)w * h;
    return (fill >= 0.85 && px >= 10000.0) || (fill >= 0.69 && px >= 20000.0);
}

// Pairs per chunk of a level: the iteration launches of a chunk re-read what the previous launch wrote, so a chunk
// whose state (64 B per pixel) stays within ~150 MB (70, 110, 200 MB measured slower) is served largely by the Infinity Cache (measured on the 179^2
// and 143^2 levels of the benchmark: -4 % each).  No chunking where a chunk could not fill the GPU.
constexpr double kChunkMB = 150.0;
int chunk_pairs(int lw, int lh, const TilePick& tp, int NP)
{
    const int tiles = tp.ntx * tp.nty;
    const bool w8 = kCfgs[tp.cfg].NW == 8;
    const int cp_min = (int)std::ceil((w8 ? 2.0 * 256 : 1.25 * 512) / tiles);
    const int cp_mem = (int)(kChunkMB * 1.0e6 / ((double)lw * lh * 64.0));
    if (cp_mem < cp_min || cp_mem >= NP) return NP;
    const int n = va_cdiv(NP, cp_mem);
    return va_cdiv(NP, n);
}

enum { LK_TILE = 0, LK_STREAM = 1 };
// kernel of level s.  Explicit choices first (tests), then the measured default: level_streams.
int level_kind(const va_tvl1_params* p, int s, int w, int h, size_t plane)
{
    return level_streams(p, p->epsilon > 0.0f, s, w, h, plane) ? LK_STREAM : LK_TILE;
}

struct Plan : va_flow_levels {
    int lk[kVaMaxScales];        // LK_TILE / LK_STREAM per level
    size_t off_pyr[kVaMaxScales], off_tmp, off_state[2], off_ro, off_err, off_sel, total;
};

int check_params(const va_tvl1_params* p, int w, int h, int n_seq, int fps)
{
    VA_CHECK_ARG(p != nullptr, "va_tvl1: params is NULL");
    if (int rc = va_flow_check_shape("va_tvl1", w, h, n_seq, fps, false)) return rc;
    VA_CHECK_ARG(p->nscales >= 1 && p->warps >= 1 && p->iters >= 1, "va_tvl1: nscales, warps, iters must be >= 1");
    VA_CHECK_ARG(p->scale_step > 0.0f && p->scale_step < 1.0f, "va_tvl1: scale_step must be in (0,1)");
    VA_CHECK_ARG(p->tau > 0.0f && p->lambda > 0.0f && p->theta > 0.0f, "va_tvl1: tau, lambda, theta must be > 0");
    VA_CHECK_ARG(p->block_iters >= 0 && p->block_iters <= 64, "va_tvl1: block_iters must be in [0,64]");
    VA_CHECK_ARG(p->fast_math == 0 || p->fast_math == 1, "va_tvl1: fast_math must be 0 or 1");
    VA_CHECK_ARG(p->tile_mask >= 0 && p->tile_mask < (1 << (kNumCfgs + 3)), "va_tvl1: tile_mask must be in [0, %d]", (1 << (kNumCfgs + 3)) - 1);
    const int sw = p->tuning[VA_TUNE_STREAM_WAVES];
    VA_CHECK_ARG(!((sw >= 3 && sw <= 6) || (sw >= 10 && sw <= 12)) && p->tuning[VA_TUNE_STREAM_PPL] != 3 && p->tuning[VA_TUNE_STREAM_QUEUE] != 1 &&
                     (p->tuning[VA_TUNE_ROWS_LEVELS] == -1 || p->tuning[VA_TUNE_ROWS_LEVELS] == 0) && p->tuning[VA_TUNE_ROWS_CFG] == 0 &&
                     !(p->tile_mask & kRetiredRowsBit),
                 "va_tvl1: this tuning value selected a retired VA_EXPERIMENTS kernel family (k_iter_rows, k_iter_stream_q, k_iter_stream4, one "
                 "deep wave, two chains per wave, 3 x 5 / 3 x 6 / 4 x 6 waves x levels, 3 pixels per lane): measured slower and removed, see "
                 "DESIGN.md section 7; commit eebd154 is the last one that contains them.  Valid stream_waves: 0, 1, 2, 7, 8, 9");
    VA_CHECK_ARG(p->tuning[VA_TUNE_STREAM_PPL] == 0 || p->tuning[VA_TUNE_STREAM_PPL] == 2, "va_tvl1: stream_ppl must be 0 (default) or 2");
    VA_CHECK_ARG(p->tuning[VA_TUNE_STREAM_QUEUE] == 0 || p->tuning[VA_TUNE_STREAM_QUEUE] == 2, "va_tvl1: stream_queue must be 0 (default) or 2 (a launch per pass)");
    VA_CHECK_ARG(p->tuning[VA_TUNE_STREAM_LEVELS] >= -1 && p->tuning[VA_TUNE_STREAM_LEVELS] < (1 << kVaMaxScales) && (sw >= 0 && sw < kMwFirst + kNumMwShapes) &&
                     p->tuning[VA_TUNE_STREAM_CHUNKS] >= 0 && p->tuning[VA_TUNE_STREAM_SLOTS] >= 0,
                 "va_tvl1: stream_levels must be -1 or a level bit set, stream_waves in [0, 9], stream_chunks and stream_slots >= 0");
    VA_CHECK_ARG(p->tau / p->theta <= 1000.0f && p->lambda * p->theta <= 1000.0f, "va_tvl1: tau/theta and lambda*theta must be <= 1000");
    return VA_OK;
}

// va_tvl1_options (NULL: every option off).  On success *median is 0, 3 or 5 and *every the iterations between two filters.
int check_options(const va_tvl1_options* o, const va_tvl1_params* p, int* median, int* every)
{
    *median = 0;
    *every = p->iters;
    if (!o) return VA_OK;
    VA_CHECK_ARG(o->struct_bytes >= (int)sizeof(va_tvl1_options), "va_tvl1: options.struct_bytes is %d, need at least %d", o->struct_bytes,
                 (int)sizeof(va_tvl1_options));
    VA_CHECK_ARG(o->median == 0 || o->median == 3 || o->median == 5, "va_tvl1: options.median must be 0, 3 or 5 (got %d)", o->median);
    VA_CHECK_ARG(o->median_every >= 0, "va_tvl1: options.median_every must be >= 0 (got %d)", o->median_every);
    *median = o->median;
    if (o->median_every > 0 && o->median_every < p->iters) *every = o->median_every;
    return VA_OK;
}

void make_plan(Plan& P, int w, int h, int n_seq, int fps, const va_tvl1_params* p)
{
    va_flow_levels_fill(&P, w, h, n_seq, fps, p->scale_step, p->nscales);
    size_t off = 0;
    for (int s = 0; s < P.ns; ++s) {
        P.lk[s] = level_kind(p, s, P.ws[s], P.hs[s], P.plane[s]);
        P.off_pyr[s] = off;
        off += va_align_up((size_t)P.NF * 3 * P.plane[s] * sizeof(float), 256);
    }
    P.off_tmp = off;  // (the buffers every level shares are sized for the largest plane of the pyramid)
    off += va_align_up((size_t)P.NF * 2 * P.plane_max * sizeof(float), 256);
    for (int b = 0; b < 2; ++b) {
        P.off_state[b] = off;
        off += va_align_up((size_t)P.NP * kNF_STATE * P.plane_max * sizeof(float), 256);
    }
    P.off_ro = off;
    off += va_align_up((size_t)P.NP * kNF_RO * P.plane_max * sizeof(float), 256);
    P.off_err = off;
    if (p->epsilon > 0.0f) off += va_align_up((size_t)P.NP * p->iters * sizeof(unsigned long long), 256);
    P.off_sel = off;
    off += va_align_up((size_t)P.NP * 2 * sizeof(int), 256);
    // unused tail, kept so that the total callers allocate by does not move: the task counters of a retired kernel
    // (2 + pairs x (iters / 16 + 2) words) were part of it
    off += va_align_up((size_t)(2 + P.NP * (p->iters / 16 + 2)) * sizeof(unsigned), 256);
    P.total = off;
}

va_prof_span prof_get(va_ctx* ctx)
{
    va_prof_span s{};
    if (!ctx->prof_pool.empty()) {
        s = ctx->prof_pool.back();
        ctx->prof_pool.pop_back();
    } else {
        (void)hipEventCreate(&s.beg);
        (void)hipEventCreate(&s.end);
    }
    return s;
}

// The buffers of a call inside its workspace (make_plan's offsets)
struct LevelBufs {
    float* pyr[kVaMaxScales];
    float *tmp1, *state[2], *ro;
    unsigned long long* err;
    int *sel, *base;
};

// va_tvl1_launch_plan's records: run_levels writes one next to every inner-iteration and median launch
struct LaunchLog {
    va_tvl1_launch* out;
    int cap, n;
    void add(const va_tvl1_launch& r)
    {
        if (n < cap) out[n] = r;
        ++n;
    }
};

// S5-S8 over the pyramid: the level, chunk, warp and iteration loop of va_tvl1_flow_opt, from the coarsest level's zero
// state to level 0's result in state[*cur_out].  live: every kernel, memset and event goes to `st`.  Not live
// (va_tvl1_launch_plan): the same decisions are taken and nothing touches a device -- ctx is NULL and B holds null pointers.
// log (NULL: none) receives a record per inner-iteration and per median launch, live or not.
int run_levels(va_ctx* ctx, const bool live, const Plan& P, const va_tvl1_params* p, const int median, const int median_every,
               const LevelBufs& B, hipStream_t st, LaunchLog* log, int* cur_out)
{
    float* const* pyr = B.pyr;
    float* const tmp1 = B.tmp1;
    float* const state[2] = {B.state[0], B.state[1]};
    float* const ro = B.ro;
    unsigned long long* const err = B.err;
    int* const sel = B.sel;
    int* const base = B.base;
    const bool eps = p->epsilon > 0.0f;
    const bool prof = live && ctx->prof_on;
    const int TPB = 256;
    const int sc = P.ns - 1;
    int cur = 0;
    int K0 = p->block_iters;  // 0 = per-level automatic choice (12 on every level of the 224x224 pyramid's top three)
    if (eps) K0 = 1;

    for (int s = sc; s >= 0; --s) {
        const int lw = P.ws[s], lh = P.hs[s], lp = P.pitch[s];
        const size_t plane = P.plane[s];
        const unsigned tmask = (unsigned)p->tile_mask & (unsigned)(kStreamBit - 1);
        // (S55: the block depth is chosen for the run of iterations between two filters)
        const TilePick tp = K0 > 0 ? pick_tiles(lw, lh, K0, tmask) : pick_tiles_auto(lw, lh, median ? median_every : p->iters, tmask);
        const bool strm = P.lk[s] == LK_STREAM;
        const int perm = strm ? 0 : 1;
        if (live && lp != lw) {
            k_zero_pad<<<dim3(va_cdiv((lp - lw) * lh * kNF_RO, TPB), P.NP), TPB, 0, st>>>(ro, kNF_RO, lw, lh, lp, plane, perm);
            VA_LAUNCH_CHECK();
        }
        // the pairs of a level go through its warps x iterations in chunks (cache residency: chunk_pairs); every chunk
        // starts from the level's entry buffer index and ends on the same one
        const int cp = (eps || strm) ? P.NP : chunk_pairs(lw, lh, tp, P.NP);
        const int cur_in = cur;
        for (int c0 = 0; c0 < P.NP; c0 += cp) {
            const int nc = P.NP - c0 < cp ? P.NP - c0 : cp;
            const dim3 gpc(va_cdiv(lw * lh, TPB), nc);
            cur = cur_in;
            for (int wp = 0; wp < p->warps; ++wp) {
                if (live) {
                    k_warp<<<gpc, TPB, 0, st>>>(pyr[s], plane, lw, lh, lp, P.F, state[0], state[1], eps ? sel : nullptr, cur,
                                                 eps ? base : nullptr, ro, c0, perm);
                    VA_LAUNCH_CHECK();
                    if (eps) VA_HIP(hipMemsetAsync(err, 0, (size_t)P.NP * p->iters * sizeof(unsigned long long), st));
                }
                va_prof_span span{};
                if (prof) {
                    span = prof_get(ctx);
                    span.level = s;
                    VA_HIP(hipEventRecord(span.beg, st));
                }
                IterArgs a{};
                a.ro = ro;
                a.stA = state[0];
                a.stB = state[1];
                a.outA = state[0];
                a.outB = state[1];
                a.base = base;
                a.sel = sel;
                a.err = err;
                a.qthr = eps ? (unsigned long long)((double)p->epsilon * (double)p->epsilon * (double)lw * (double)lh * 4294967296.0) : 0ull;
                a.plane = plane;
                a.w = lw;
                a.h = lh;
                a.pitch = lp;
                a.ntx = tp.ntx;
                a.nty = tp.nty;
                a.HX = tp.HX;
                a.iters = p->iters;
                a.l_t = p->lambda * p->theta;
                a.taut = p->tau / p->theta;
                a.theta = p->theta;
                a.pair0 = c0;
                int launches = 0;
                // what every record of this warp and chunk shares
                va_tvl1_launch rec{};
                rec.level = s;
                rec.warp = wp;
                rec.pair0 = c0;
                rec.npairs = nc;
                rec.w = lw;
                rec.h = lh;
                rec.pitch = lp;
                rec.cfg = -1;
                rec.fast = p->fast_math != 0;
                // one pass of the row pipeline in the shape nwv x kh over `grid`
                auto stream_pass = [&](const StreamPick& sp, StreamArgs& sa, int nwv, int kh, const dim3& grid, int it) -> int {
                    sa.sin = state[cur];
                    sa.sout = state[cur ^ 1];
                    sa.rev = launches & 1;
                    if (log) {
                        va_tvl1_launch r = rec;
                        r.family = VA_TVL1_LAUNCH_STREAM;
                        r.waves = nwv;
                        r.levels = kh;
                        r.K = sa.K;
                        r.it0 = it;
                        r.grid_x = (int)grid.x;
                        r.grid_y = (int)grid.y;
                        r.strips = sp.nsx;
                        r.row_chunks = sp.nch;
                        r.rows_per_chunk = sp.R;
                        r.halo_x = sp.HX;
                        r.narrow = sa.narrow;
                        r.rev = sa.rev;
                        log->add(r);
                    }
                    if (live)
                        if (int rc = launch_stream(nwv, kh, p->fast_math != 0, grid, st, sa)) return rc;
                    cur ^= 1;
                    ++launches;
                    return VA_OK;
                };
                // iterations it0 .. it0 + n - 1 of this warp, from state[cur]: the whole warp, or (S55) the segment between two filters
                auto run_iters = [&](const int it0, const int n) -> int {
                    if (strm) {
                        const StreamPick sp = pick_stream(p, lw, lh, nc);
                        StreamArgs sa{};
                        sa.ro = ro;
                        sa.plane = plane;
                        sa.w = lw;
                        sa.h = lh;
                        sa.pitch = lp;
                        sa.nsx = sp.nsx;
                        sa.nch = sp.nch;
                        sa.R = sp.R;
                        sa.HX = sp.HX;
                        sa.pair0 = c0;
                        sa.l_t = a.l_t;
                        sa.taut = a.taut;
                        sa.theta = a.theta;
                        const dim3 grid(sp.nsx * sp.nch, nc);
                        // the four-wave passes of a level whose last strip fits 32 lanes: one wave for the last strips of two pairs
                        const bool narrow = sp.narrow != 0;
                        const dim3 grid_mw = narrow ? dim3((2 * sp.nsx - 1) * sp.nch, va_cdiv(nc, 2)) : grid;
                        sa.npairs = nc;
                        // pipelines of four waves: the passes share the iterations as evenly as possible, so that every pass
                        // is deep enough to end in the last wave (K > (waves - 1) x levels per wave); otherwise the forms below run
                        int mw_n = 0, mw_base = 0, mw_extra = 0;
                        if (sp.nwv) {
                            const int kmax = sp.nwv * sp.kh, kmin = (sp.nwv - 1) * sp.kh + 1;
                            mw_n = va_cdiv(n, kmax);
                            mw_base = n / mw_n;
                            mw_extra = n % mw_n;
                            if (mw_base < kmin) mw_n = 0;
                        }
                        int it = 0;
                        for (int i = 0; i < mw_n; ++i) {
                            sa.K = mw_base + (i < mw_extra ? 1 : 0);
                            sa.narrow = narrow ? 1 : 0;
                            if (int rc = stream_pass(sp, sa, sp.nwv, sp.kh, grid_mw, it0 + it)) return rc;
                            sa.narrow = 0;
                            it += sa.K;
                        }
                        for (it = mw_n ? n : 0; it < n;) {
                            const int rem = n - it;
                            // the two-wave kernel needs its last level in the second wave: a shorter remainder runs in one wave
                            const bool fb = rem > (sp.fb_nwv - 1) * sp.fb_kh;
                            const int nwv = fb ? sp.fb_nwv : 1, kh = fb ? sp.fb_kh : kStreamK1;
                            sa.K = rem < nwv * kh ? rem : nwv * kh;
                            if (int rc = stream_pass(sp, sa, nwv, kh, grid, it0 + it)) return rc;
                            it += sa.K;
                        }
                    }
                    for (int it = strm ? n : 0; it < n;) {
                        // the tile grid depends on the halo depth: a shorter last launch gets its own grid
                        const int k = (n - it) < tp.K ? (n - it) : tp.K;
                        const TilePick tk = (k == tp.K) ? tp : pick_tiles(lw, lh, k, tmask);
                        a.ntx = tk.ntx;
                        a.nty = tk.nty;
                        a.HX = tk.HX;
                        a.cur = cur;
                        a.K = tk.K;
                        a.it = it0 + it;
                        a.rev = launches & 1;
                        if (log) {
                            const TileCfg& c = kCfgs[tk.cfg];
                            const dim3 grid = iter_grid(tk, nc);
                            va_tvl1_launch r = rec;
                            r.family = VA_TVL1_LAUNCH_TILE;
                            r.cfg = tk.cfg;
                            r.waves = c.NW;
                            r.eps = eps;
                            r.K = a.K;
                            r.it0 = a.it;
                            r.grid_x = (int)grid.x;
                            r.grid_y = (int)grid.y;
                            r.strips = tk.ntx;
                            r.row_chunks = tk.nty;
                            r.rows_per_chunk = c.NW * (64 / c.LX) * c.C;
                            r.halo_x = tk.HX;
                            r.rev = a.rev;
                            log->add(r);
                        }
                        if (live) {
                            if (eps) {
                                if (p->fast_math) launch_iter<true, true>(tk, a, nc, st);
                                else launch_iter<true, false>(tk, a, nc, st);
                            } else {
                                if (p->fast_math) launch_iter<false, true>(tk, a, nc, st);
                                else launch_iter<false, false>(tk, a, nc, st);
                            }
                        }
                        cur ^= 1;
                        it += tk.K;
                        ++launches;
                    }
                    return VA_OK;
                };
                if (!median) {
                    if (int rc = run_iters(0, p->iters)) return rc;
                } else {
                    // S55: u1, u2 of every pair still iterating <- their median, at the head of iteration it0; through the
                    // pyramid's scratch planes ([pair][2][plane]: NP x 2 planes fit the NF x 2 of tmp1, tmp2)
                    MedianArgs m{};
                    m.base = base;
                    m.err = eps ? err : nullptr;
                    m.qthr = a.qthr;
                    m.plane = plane;
                    m.iters = p->iters;
                    m.w = lw;
                    m.h = lh;
                    m.pitch = lp;
                    m.perm = perm;
                    m.ntx = va_cdiv(lw, kMedTX);
                    m.pair0 = c0;
                    for (int it0 = 0; it0 < p->iters; it0 += median_every) {
                        m.cur = cur;
                        m.it = it0;
                        m.srcA = state[0];
                        m.srcB = state[1];
                        m.src_nf = kNF_STATE;
                        m.dstA = m.dstB = tmp1;
                        m.dst_nf = 2;
                        if (log) {
                            const dim3 grid = median_grid(m, nc);
                            va_tvl1_launch r = rec;
                            r.family = VA_TVL1_LAUNCH_MEDIAN;
                            r.fast = 0;
                            r.eps = eps;
                            r.median = median;
                            r.it0 = it0;
                            r.grid_x = (int)grid.x;
                            r.grid_y = (int)grid.y;
                            r.strips = m.ntx;
                            r.row_chunks = va_cdiv(lh, kMedTY);
                            r.rows_per_chunk = kMedTY;
                            r.halo_x = median / 2;
                            log->add(r);
                        }
                        if (live) launch_median(median, m, nc, st);
                        m.srcA = m.srcB = tmp1;
                        m.src_nf = 2;
                        m.dstA = state[0];
                        m.dstB = state[1];
                        m.dst_nf = kNF_STATE;
                        if (live) k_median_store<<<dim3(va_cdiv(lw * lh, TPB), nc, 2), TPB, 0, st>>>(m);
                        const int n = p->iters - it0 < median_every ? p->iters - it0 : median_every;
                        if (int rc = run_iters(it0, n)) return rc;
                    }
                }
                if (live) VA_LAUNCH_CHECK();
                if (prof) {
                    VA_HIP(hipEventRecord(span.end, st));
                    ctx->prof_spans.push_back(span);
                    ctx->prof_launches += launches;
                    ctx->prof_pxiters += (double)nc * lw * lh * p->iters;
                    ctx->prof_pxwarps += (double)nc * lw * lh;
                    if (s < kVaProfLevels) {
                        ctx->prof_level_pxiters[s] += (double)nc * lw * lh * p->iters;
                        ctx->prof_level_launches[s] += launches;
                    }
                }
            }
        }
        if (s > 0) {
            if (live) {
                // ro is free between levels: use it as the upsampling target (2 of its 4 planes per pair)
                const dim3 g(va_cdiv(P.ws[s - 1] * P.hs[s - 1], TPB), P.NP);
                k_upsample<<<g, TPB, 0, st>>>(state[0], state[1], eps ? sel : nullptr, cur, lw, lh, lp, plane, ro, P.ws[s - 1],
                                               P.hs[s - 1], P.pitch[s - 1], P.plane[s - 1], 1.0f / p->scale_step, perm);
                const int fperm = P.lk[s - 1] != LK_TILE ? 0 : 1;
                const dim3 gi(va_cdiv(P.pitch[s - 1] * P.hs[s - 1], TPB), P.NP);
                k_level_init<<<gi, TPB, 0, st>>>(ro, state[0], P.ws[s - 1], P.hs[s - 1], P.pitch[s - 1], P.plane[s - 1], fperm);
                VA_LAUNCH_CHECK();
            }
            cur = 0;
            if (live && eps) VA_HIP(hipMemsetAsync(sel, 0, (size_t)P.NP * sizeof(int), st));
        }
    }
    *cur_out = cur;
    return VA_OK;
}

}  // namespace

extern "C" void va_tvl1_default_params(va_tvl1_params* p)
{
    if (!p) return;
    p->tau = 0.25f;
    p->lambda = 0.15f;
    p->theta = 0.3f;
    p->nscales = 5;
    p->warps = 5;
    p->epsilon = 0.01f;
    p->iters = 300;
    p->scale_step = 0.8f;
    p->block_iters = 0;
    p->fast_math = 0;
    p->tile_mask = 0;
    p->tuning[VA_TUNE_STREAM_LEVELS] = -1;
    p->tuning[VA_TUNE_STREAM_WAVES] = 0;
    p->tuning[VA_TUNE_STREAM_CHUNKS] = 0;
    p->tuning[VA_TUNE_STREAM_SLOTS] = 0;
    p->tuning[VA_TUNE_ROWS_LEVELS] = -1;
    p->tuning[VA_TUNE_ROWS_CFG] = 0;
    p->tuning[VA_TUNE_STREAM_PPL] = 0;
    p->tuning[VA_TUNE_STREAM_QUEUE] = 0;
}

extern "C" int va_tvl1_pyramid_sizes(int w, int h, const va_tvl1_params* p, int* ws, int* hs)
{
    if (!p || !ws || !hs || w < 1 || h < 1 || !(p->scale_step > 0.0f && p->scale_step < 1.0f)) return 0;
    return va_flow_pyramid_sizes(w, h, p->scale_step, p->nscales, ws, hs);
}

// The register tiling va_tvl1_flow will use (host logic only; no device needed): for every pyramid level s,
// out[6*s .. 6*s+5] = { tile width, tile height, waves per workgroup, block depth K, tiles in x, tiles in y }.
extern "C" int va_tvl1_tile_plan(int w, int h, const va_tvl1_params* p, int* out)
{
    if (!p || !out || w < 16 || h < 16 || !(p->scale_step > 0.0f && p->scale_step < 1.0f) || p->iters < 1) return 0;
    int ws[kVaMaxScales], hs[kVaMaxScales];
    const int ns = va_flow_pyramid_sizes(w, h, p->scale_step, p->nscales, ws, hs);
    int K0 = p->block_iters;
    if (p->epsilon > 0.0f) K0 = 1;
    for (int s = 0; s < ns; ++s) {
        const unsigned tmask = (unsigned)p->tile_mask & (unsigned)(kStreamBit - 1);
        const TilePick tp = K0 > 0 ? pick_tiles(ws[s], hs[s], K0, tmask) : pick_tiles_auto(ws[s], hs[s], p->iters, tmask);
        const TileCfg& c = kCfgs[tp.cfg];
        int lp;
        size_t lplane;
        va_stage_layout(ws[s], hs[s], &lp, &lplane);
        if (level_kind(p, s, ws[s], hs[s], lplane) == LK_STREAM) {
            StreamPick sp{};
            stream_strips(p, ws[s], sp);
            const int nwv = sp.nwv ? sp.nwv : sp.fb_nwv, kh = sp.nwv ? sp.kh : sp.fb_kh;
            const int plan[6] = {kStreamSW, 0, nwv, nwv * kh, sp.nsx, 0};
            memcpy(out + 6 * s, plan, sizeof(plan));
            continue;
        }
        out[6 * s + 0] = c.LX * c.R;
        out[6 * s + 1] = c.NW * (64 / c.LX) * c.C;
        out[6 * s + 2] = c.NW;
        out[6 * s + 3] = tp.K;
        out[6 * s + 4] = tp.ntx;
        out[6 * s + 5] = tp.nty;
    }
    return ns;
}

extern "C" size_t va_tvl1_workspace_bytes(int w, int h, int n_seq, int frames_per_seq, const va_tvl1_params* p)
{
    return va_tvl1_workspace_bytes_opt(w, h, n_seq, frames_per_seq, p, nullptr);
}

// (the median goes through the pyramid's scratch planes, which are free once the pyramid stands: no option changes the size)
extern "C" size_t va_tvl1_workspace_bytes_opt(int w, int h, int n_seq, int frames_per_seq, const va_tvl1_params* p,
                                              const va_tvl1_options* opt)
{
    if (check_params(p, w, h, n_seq, frames_per_seq) != VA_OK) return 0;
    int median, every;
    if (check_options(opt, p, &median, &every) != VA_OK) return 0;
    Plan P;
    make_plan(P, w, h, n_seq, frames_per_seq, p);
    return P.total;
}

// The launches of a call, from run_levels itself running dry (host only, no device: include/va.h)
extern "C" int va_tvl1_launch_plan(int w, int h, int n_seq, int frames_per_seq, const va_tvl1_params* p, const va_tvl1_options* opt,
                                   va_tvl1_launch* records, int capacity)
{
    if (check_params(p, w, h, n_seq, frames_per_seq) != VA_OK) return -1;
    int median, median_every;
    if (check_options(opt, p, &median, &median_every) != VA_OK) return -1;
    if (capacity < 0 || (capacity > 0 && !records)) {
        va_set_error("va_tvl1_launch_plan: records is NULL or capacity negative");
        return -1;
    }
    Plan P;
    make_plan(P, w, h, n_seq, frames_per_seq, p);
    const LevelBufs B{};
    LaunchLog log{records, capacity, 0};
    int cur = 0;
    if (run_levels(nullptr, false, P, p, median, median_every, B, nullptr, &log, &cur) != VA_OK) return -1;
    return log.n;
}

extern "C" int va_tvl1_flow(va_ctx* ctx, const void* frames, int frames_are_u8, int n_seq, int frames_per_seq, int w,
                            int h, const va_tvl1_params* p, void* flow, void* workspace, size_t workspace_bytes,
                            void* stream)
{
    return va_tvl1_flow_opt(ctx, frames, frames_are_u8, n_seq, frames_per_seq, w, h, p, nullptr, flow, workspace, workspace_bytes, stream);
}

extern "C" int va_tvl1_flow_opt(va_ctx* ctx, const void* frames, int frames_are_u8, int n_seq, int frames_per_seq, int w,
                                int h, const va_tvl1_params* p, const va_tvl1_options* opt, void* flow, void* workspace,
                                size_t workspace_bytes, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_tvl1_flow: ctx is NULL");
    VA_USE_DEVICE(ctx);
    if (int rc = va_flow_check_buffers("va_tvl1_flow", frames, flow, workspace, 0, 0)) return rc;
    if (int rc = check_params(p, w, h, n_seq, frames_per_seq)) return rc;
    int median, median_every;  // S55: median = 0 runs one segment of p->iters iterations, the launch sequence without the option
    if (int rc = check_options(opt, p, &median, &median_every)) return rc;
    Plan P;
    make_plan(P, w, h, n_seq, frames_per_seq, p);
    if (int rc = va_flow_check_buffers("va_tvl1_flow", frames, flow, workspace, workspace_bytes, P.total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* pyr[kVaMaxScales];
    for (int s = 0; s < P.ns; ++s) pyr[s] = (float*)(ws + P.off_pyr[s]);
    float* tmp1 = (float*)(ws + P.off_tmp);
    float* tmp2 = tmp1 + (size_t)P.NF * P.plane_max;
    float* state[2] = {(float*)(ws + P.off_state[0]), (float*)(ws + P.off_state[1])};
    float* ro = (float*)(ws + P.off_ro);
    unsigned long long* err = (unsigned long long*)(ws + P.off_err);
    int* sel = (int*)(ws + P.off_sel);
    int* base = sel + P.NP;
    const bool eps = p->epsilon > 0.0f;
    const int TPB = 256;

    // S0-S2: level 0, then the pyramid of every FRAME (shared by both pairs it belongs to) and its gradient.
    if (int rc = va_stage_frames(frames, frames_are_u8, false, pyr[0], w, h, P.pitch[0], P.plane[0], P.NF, st)) return rc;
    if (int rc = va_stage_pyramid(pyr, P.ws, P.hs, P.pitch, P.plane, P.ns, P.NF, tmp1, tmp2, P.plane_max, p->scale_step, st)) return rc;
    for (int s = 0; s < P.ns; ++s)
        if (int rc = va_stage_gradient(pyr[s], P.ws[s], P.hs[s], P.pitch[s], P.plane[s], P.NF, st)) return rc;

    // S4: u = 0, p = 0 at the coarsest level.
    const int sc = P.ns - 1;
    VA_HIP(hipMemsetAsync(state[0], 0, (size_t)P.NP * kNF_STATE * P.plane[sc] * sizeof(float), st));
    VA_HIP(hipMemsetAsync(sel, 0, (size_t)P.NP * 2 * sizeof(int), st));
    int cur = 0;
    LevelBufs B{};
    for (int s = 0; s < P.ns; ++s) B.pyr[s] = pyr[s];
    B.tmp1 = tmp1;
    B.state[0] = state[0];
    B.state[1] = state[1];
    B.ro = ro;
    B.err = err;
    B.sel = sel;
    B.base = base;
    if (int rc = run_levels(ctx, true, P, p, median, median_every, B, st, nullptr, &cur)) return rc;
    {
        const dim3 g(va_cdiv(w * h, TPB), P.NP);
        k_flow_out<<<g, TPB, 0, st>>>(state[0], state[1], eps ? sel : nullptr, cur, w, h, P.pitch[0], P.plane[0], (float*)flow,
                                       P.lk[0] != LK_TILE ? 0 : 1);
        VA_LAUNCH_CHECK();
    }
    return VA_OK;
}

extern "C" int va_flow_to_stack(va_ctx* ctx, const void* flow, int n_pairs, int w, int h, float bound, float mean,
                                float stdv, void* stack, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_flow_to_stack: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(flow != nullptr && stack != nullptr, "va_flow_to_stack: NULL buffer");
    VA_CHECK_ARG(n_pairs >= 1 && w >= 1 && h >= 1, "va_flow_to_stack: bad shape");
    VA_CHECK_ARG(bound > 0.0f && stdv > 0.0f, "va_flow_to_stack: bound and std must be > 0");
    const size_t n = (size_t)n_pairs * 2 * w * h;
    k_flow_to_stack<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>((const float*)flow, (float*)stack, n, bound, mean, stdv);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

// S55 on stored flow: every plane of flow [n_fields][2][h][w] -> its ksize x ksize median (k_median on dense planes)
extern "C" int va_flow_median(va_ctx* ctx, const void* flow, int n_fields, int w, int h, int ksize, void* out, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_flow_median: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(flow != nullptr && out != nullptr, "va_flow_median: NULL buffer");
    VA_CHECK_ARG(n_fields >= 1 && w >= 1 && h >= 1 && w <= 16384 && h <= 16384, "va_flow_median: bad shape (%d fields of %dx%d)", n_fields, w, h);
    VA_CHECK_ARG(ksize == 3 || ksize == 5, "va_flow_median: ksize must be 3 or 5 (got %d)", ksize);
    const size_t bytes = (size_t)n_fields * 2 * w * h * sizeof(float);
    const uintptr_t f0 = (uintptr_t)flow, o0 = (uintptr_t)out;
    VA_CHECK_ARG(f0 + bytes <= o0 || o0 + bytes <= f0, "va_flow_median: out must not overlap flow");
    MedianArgs m{};
    m.plane = (size_t)w * h;
    m.src_nf = m.dst_nf = 2;
    m.w = w;
    m.h = h;
    m.pitch = w;
    m.ntx = va_cdiv(w, kMedTX);
    for (int f = 0; f < n_fields; f += 32768) {  // (the grid's y extent)
        m.srcA = m.srcB = (const float*)flow + (size_t)f * 2 * m.plane;
        m.dstA = m.dstB = (float*)out + (size_t)f * 2 * m.plane;
        launch_median(ksize, m, n_fields - f < 32768 ? n_fields - f : 32768, (hipStream_t)stream);
    }
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_selftest_exact_math(va_ctx* ctx, float lo, float hi, unsigned long long* mismatches, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr && mismatches != nullptr, "va_selftest_exact_math: NULL argument");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(lo >= kSqrtReg && hi <= 1e30f && lo <= hi, "va_selftest_exact_math: range must lie in [2^-100, 1e30]");
    unsigned ulo, uhi;
    memcpy(&ulo, &lo, 4);
    memcpy(&uhi, &hi, 4);
    VA_HIP(hipMemsetAsync(mismatches, 0, 2 * sizeof(unsigned long long), (hipStream_t)stream));
    k_selftest_exact_math<<<4096, 256, 0, (hipStream_t)stream>>>(ulo, (unsigned long long)uhi - ulo + 1, mismatches);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_tvl1_profile_enable(va_ctx* ctx, int on)
{
    VA_CHECK_ARG(ctx != nullptr, "va_tvl1_profile_enable: ctx is NULL");
    VA_USE_DEVICE(ctx);
    ctx->prof_on = on != 0;
    if (on) {
        // time origin: everything recorded later (on any stream) is measured against it
        if (!ctx->prof_ref) VA_HIP(hipEventCreate(&ctx->prof_ref));
        VA_HIP(hipDeviceSynchronize());
        VA_HIP(hipEventRecord(ctx->prof_ref, nullptr));
        VA_HIP(hipEventSynchronize(ctx->prof_ref));
    }
    return VA_OK;
}

extern "C" int va_tvl1_profile_read(va_ctx* ctx, double* out, int reset)
{
    VA_CHECK_ARG(ctx != nullptr && out != nullptr, "va_tvl1_profile_read: NULL argument");
    VA_USE_DEVICE(ctx);
    std::vector<std::pair<float, float>> iv;
    for (va_prof_span& s : ctx->prof_spans) {
        VA_HIP(hipEventSynchronize(s.end));
        float ms = 0.0f, t0 = 0.0f, t1 = 0.0f;
        VA_HIP(hipEventElapsedTime(&ms, s.beg, s.end));
        ctx->prof_ms += ms;
        if (s.level >= 0 && s.level < kVaProfLevels) ctx->prof_level_ms[s.level] += ms;
        if (ctx->prof_ref) {
            VA_HIP(hipEventElapsedTime(&t0, ctx->prof_ref, s.beg));
            VA_HIP(hipEventElapsedTime(&t1, ctx->prof_ref, s.end));
            iv.emplace_back(t0, t1);
        }
        ctx->prof_pool.push_back(s);
    }
    ctx->prof_spans.clear();
    // union of the spans: with several streams the launches of different calls overlap in time
    std::sort(iv.begin(), iv.end());
    float cur0 = 0.0f, cur1 = -1.0f;
    for (auto& p : iv) {
        if (cur1 < cur0 || p.first > cur1) {
            if (cur1 >= cur0) ctx->prof_union_ms += cur1 - cur0;
            cur0 = p.first;
            cur1 = p.second;
        } else if (p.second > cur1) {
            cur1 = p.second;
        }
    }
    if (cur1 >= cur0) ctx->prof_union_ms += cur1 - cur0;
    out[0] = ctx->prof_ms;
    out[1] = ctx->prof_launches;
    out[2] = ctx->prof_pxiters;
    out[3] = ctx->prof_pxwarps;
    out[4] = ctx->prof_union_ms;
    if (reset) ctx->prof_ms = ctx->prof_union_ms = ctx->prof_launches = ctx->prof_pxiters = ctx->prof_pxwarps = 0.0;
    return VA_OK;
}

// Per pyramid level (0 = full resolution), since the last reset: out[3*s + 0] = summed per-call milliseconds of the
// level's inner-iteration launches, out[3*s + 1] = pixel-iterations, out[3*s + 2] = launches (HOST array of 3*n
// doubles, n <= 16).  Call after va_tvl1_profile_read (which synchronises the events) and before its reset.
extern "C" int va_tvl1_profile_levels(va_ctx* ctx, double* out, int n, int reset)
{
    VA_CHECK_ARG(ctx != nullptr && out != nullptr && n >= 1 && n <= kVaProfLevels, "va_tvl1_profile_levels: bad argument");
    for (int s = 0; s < n; ++s) {
        out[3 * s + 0] = ctx->prof_level_ms[s];
        out[3 * s + 1] = ctx->prof_level_pxiters[s];
        out[3 * s + 2] = ctx->prof_level_launches[s];
    }
    if (reset)
        for (int s = 0; s < kVaProfLevels; ++s) ctx->prof_level_ms[s] = ctx->prof_level_pxiters[s] = ctx->prof_level_launches[s] = 0.0;
    return VA_OK;
}

// ---- S8 and the output copy for the methods whose state is TV-L1's [pair][6][plane] in plain row order (brox.hip,
// farneback.hip): k_upsample, k_level_init and k_flow_out as va_tvl1_flow launches them, without the per-pair buffer select.

// S8: planes 0, 1 of the coarse state -> planes 0, 1 of the fine state (through tmp [pair][2][fplane]); the fine state's
// planes 2..5 and its pitch padding become 0 (k_level_init).  The coarse and the fine state may be the same buffer.
int va_stage_upsample(const float* cstate, int cw, int ch, int cpitch, size_t cplane, float* tmp, float* fstate, int fw, int fh,
                      int fpitch, size_t fplane, float inv_step, int NP, hipStream_t st)
{
    const int TPB = 256;
    k_upsample<<<dim3(va_cdiv(fw * fh, TPB), NP), TPB, 0, st>>>(cstate, cstate, nullptr, 0, cw, ch, cpitch, cplane, tmp, fw, fh, fpitch,
                                                                 fplane, inv_step, 0);
    k_level_init<<<dim3(va_cdiv(fpitch * fh, TPB), NP), TPB, 0, st>>>(tmp, fstate, fw, fh, fpitch, fplane, 0);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

// planes 0, 1 of the state -> flow [pair][2][h][w]
int va_stage_flow_out(const float* state, int w, int h, int pitch, size_t plane, float* flow, int NP, hipStream_t st)
{
    k_flow_out<<<dim3(va_cdiv(w * h, 256), NP), 256, 0, st>>>(state, state, nullptr, 0, w, h, pitch, plane, flow, 0);
    VA_LAUNCH_CHECK();
    return VA_OK;
}
