// Farneback optical flow for gfx950 (MI355X): hand-written HIP, no CPU fallback.
//
// G. Farneback, "Two-frame motion estimation based on polynomial expansion" (SCIA 2003), in the structure of OpenCV's
// calcOpticalFlowFarneback.  DESIGN.md S63-S67 fix every expression and its operation order; this file is compiled with
// -ffp-contract=off and writes no fmaf of its own, so that results are independent of the tiling and comparable bit for bit
// with an independent float32 implementation.
//
// Frames (S0) and pyramid (S1) are the flow methods' shared front end (va_stage_*, flow_common.hip); upsampling (S8) and the
// output copy are TV-L1's kernels (va_stage_*, tvl1.hip).  The layout is the shared one: rows `pitch` = width rounded up to
// 4 floats, planes rounded up to 64 floats.
//   pyramid  [level][frame][3][plane]: plane 0 is the frame (gray values in [0,255]); planes 1, 2 are not used
//   coef     [frame][5][plane]: (b_x, b_y, a_xx, a_yy, a_xy) of the current level (S64)
//   state    [pair][6][plane]: the flow ping-pongs between planes (0, 1) and planes (2, 3)
//
// Two kernels are the whole method.  k_farneback_polyexp runs once per frame and level: a tile and its halo of poly_n in
// LDS, the vertical and the horizontal pass there, five planes out.  k_farneback_pass is one pass of S65-S67 in one launch:
// the five matrix entries of a tile and its halo of winsize/2 into LDS (the halo is recomputed, not exchanged: workgroups
// stay independent), the vertical and the horizontal window sum from LDS, the 2x2 solve, the new flow into the other field.
#include "va_internal.h"
#include <cmath>
#include <cstring>

namespace {

constexpr int kNT = 256;
constexpr int kMaxRadius = 31;       // winsize <= 63
constexpr int kDefTileW = 32, kDefTileH = 16;
constexpr float kDetReg = 1e-3f;     // S67

__device__ __forceinline__ int d_clamp(int v, int hi) { return d_min(d_max(v, 0), hi); }

struct PolyArgs {
    const float* src;  // frame f: src + f * sstride, rows `pitch` floats apart
    size_t sstride;
    float* dst;        // plane k of frame f: dst + f * dstride + k * dplane
    size_t dstride, dplane;
    int w, h, pitch;
    int TW, TH, ntx;
    float g[8], xg[8], xxg[8];  // S64's taps for |k| = 0 .. poly_n
    float ig11, ig03, ig33, ig55;
};

// S64.  grid (tiles, frames); dynamic LDS: (TW + 2N)(TH + 2N) + 3 (TW + 2N) TH floats.
template <int N>
__global__ void __launch_bounds__(kNT) k_farneback_polyexp(PolyArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int f = blockIdx.y;
    const int ty0 = blockIdx.x / a.ntx, tx0 = blockIdx.x - ty0 * a.ntx;
    const int x0 = tx0 * a.TW, y0 = ty0 * a.TH;
    const int RW = a.TW + 2 * N, RH = a.TH + 2 * N;
    float* I = lds;            // [RH][RW]
    float* M = lds + RH * RW;  // [3][TH][RW]
    const int msz = a.TH * RW;
    const float* src = a.src + (size_t)f * a.sstride;
    for (int i = threadIdx.x; i < RW * RH; i += kNT) {
        const int ry = i / RW, rx = i - ry * RW;
        const int gx = d_clamp(x0 - N + rx, a.w - 1), gy = d_clamp(y0 - N + ry, a.h - 1);
        I[i] = src[(size_t)gy * a.pitch + gx];
    }
    __syncthreads();
    // vertical: the three moments of every column of the region, taps from -N to +N
    for (int i = threadIdx.x; i < msz; i += kNT) {
        const int ty = i / RW, rx = i - ty * RW;
        const float* col = I + ty * RW + rx;
        float v = col[0];
        float m0 = a.g[N] * v, m1 = -a.xg[N] * v, m2 = a.xxg[N] * v;
#pragma unroll
        for (int k = -N + 1; k <= N; ++k) {
            const int ak = k < 0 ? -k : k;
            v = col[(k + N) * RW];
            m0 = m0 + a.g[ak] * v;
            m1 = m1 + (k < 0 ? -a.xg[ak] : a.xg[ak]) * v;
            m2 = m2 + a.xxg[ak] * v;
        }
        M[i] = m0, M[msz + i] = m1, M[2 * msz + i] = m2;
    }
    __syncthreads();
    // horizontal: the six products, then the coefficients
    for (int i = threadIdx.x; i < a.TW * a.TH; i += kNT) {
        const int ty = i / a.TW, tx = i - ty * a.TW;
        const int gx = x0 + tx, gy = y0 + ty;
        if (gx >= a.w || gy >= a.h) continue;
        const float* r = M + ty * RW + tx;
        float v0 = r[0], v1 = r[msz], v2 = r[2 * msz];
        float b1 = a.g[N] * v0, b2 = -a.xg[N] * v0, b4 = a.xxg[N] * v0;
        float b3 = a.g[N] * v1, b6 = -a.xg[N] * v1, b5 = a.g[N] * v2;
#pragma unroll
        for (int k = -N + 1; k <= N; ++k) {
            const int ak = k < 0 ? -k : k;
            const float gk = a.g[ak], xk = k < 0 ? -a.xg[ak] : a.xg[ak];
            v0 = r[k + N], v1 = r[msz + k + N], v2 = r[2 * msz + k + N];
            b1 = b1 + gk * v0;
            b2 = b2 + xk * v0;
            b4 = b4 + a.xxg[ak] * v0;
            b3 = b3 + gk * v1;
            b6 = b6 + xk * v1;
            b5 = b5 + gk * v2;
        }
        float* d = a.dst + (size_t)f * a.dstride + (size_t)gy * a.pitch + gx;
        d[0] = b2 * a.ig11;
        d[a.dplane] = b3 * a.ig11;
        d[2 * a.dplane] = b1 * a.ig03 + b4 * a.ig33;
        d[3 * a.dplane] = b1 * a.ig03 + b5 * a.ig33;
        d[4 * a.dplane] = b6 * a.ig55;
    }
}

struct PassArgs {
    const float* r0;  // first frame's coefficients of pair n: r0 + frame(n) * rstride, plane k at + k * cplane
    const float* r1;  // second frame's: r1 + frame(n) * rstride
    size_t rstride, cplane;
    const float* fin;  // flow of pair n coming in: u at fin + n * fstride, v one fplane further
    float* fout;       // and going out
    size_t fstride, fplane;
    int w, h, pitch;
    int fps;  // frames per sequence: frame(n) = n + n / (fps - 1); 0: frame(n) = n
    int TW, TH, ntx, m;
    float kw[kMaxRadius + 1];  // S66's taps for |i| = 0 .. m
};

// S65's border weight of coordinate x in a frame of n: the outermost five pixels on either side
__device__ __forceinline__ float border_weight(int x, int n)
{
    const float lo = x < 2 ? 0.14f : (x < 5 ? 0.4472f : 1.0f);
    const int r = n - 1 - x;
    const float hi = r < 2 ? 0.14f : (r < 5 ? 0.4472f : 1.0f);
    return lo * hi;
}

// S65-S67.  grid (tiles, pairs); dynamic LDS: 5 ((TW + 2m)(TH + 2m) + (TW + 2m) TH) floats.
__global__ void __launch_bounds__(kNT) k_farneback_pass(PassArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int n = blockIdx.y;
    const int ty0 = blockIdx.x / a.ntx, tx0 = blockIdx.x - ty0 * a.ntx;
    const int x0 = tx0 * a.TW, y0 = ty0 * a.TH;
    const int m = a.m, RW = a.TW + 2 * m, RH = a.TH + 2 * m;
    const int esz = RW * RH, vsz = RW * a.TH;
    float* E = lds;            // [5][RH][RW]
    float* V = lds + 5 * esz;  // [5][TH][RW]
    const int frame = a.fps > 1 ? n + n / (a.fps - 1) : n;
    const float* R0 = a.r0 + (size_t)frame * a.rstride;
    const float* R1 = a.r1 + (size_t)frame * a.rstride;
    const float* U = a.fin + (size_t)n * a.fstride;
    const size_t cp = a.cplane;

    // S65: the five entries of every pixel of the region (a cell outside the frame is its clamped pixel's)
    for (int i = threadIdx.x; i < esz; i += kNT) {
        const int ry = i / RW, rx = i - ry * RW;
        const int gx = d_clamp(x0 - m + rx, a.w - 1), gy = d_clamp(y0 - m + ry, a.h - 1);
        const size_t o = (size_t)gy * a.pitch + gx;
        const float u = U[o], v = U[a.fplane + o];
        const float px = (float)gx + u, py = (float)gy + v;
        const bool in = px >= 0.0f && px <= (float)(a.w - 1) && py >= 0.0f && py <= (float)(a.h - 1);  // (a NaN is outside)
        const float x1f = fminf(floorf(px), (float)(a.w - 2)), y1f = fminf(floorf(py), (float)(a.h - 2));
        const float a0xx = R0[2 * cp + o], a0yy = R0[3 * cp + o], a0xy = R0[4 * cp + o];
        float axx, ayy, axy, bx1, by1;
        if (in) {
            const int x1 = (int)x1f, y1 = (int)y1f;
            const float fx = px - x1f, fy = py - y1f;
            const float a00 = (1.0f - fx) * (1.0f - fy), a01 = fx * (1.0f - fy), a10 = (1.0f - fx) * fy, a11 = fx * fy;
            const float* q = R1 + (size_t)y1 * a.pitch + x1;
            float c[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const float* qk = q + k * cp;
                c[k] = ((a00 * qk[0] + a01 * qk[1]) + a10 * qk[a.pitch]) + a11 * qk[a.pitch + 1];
            }
            bx1 = c[0], by1 = c[1];
            axx = (a0xx + c[2]) * 0.5f;
            ayy = (a0yy + c[3]) * 0.5f;
            axy = (a0xy + c[4]) * 0.25f;
        } else {
            bx1 = 0.0f, by1 = 0.0f;
            axx = a0xx, ayy = a0yy, axy = a0xy * 0.5f;
        }
        float dbx = (R0[o] - bx1) * 0.5f, dby = (R0[cp + o] - by1) * 0.5f;
        dbx = dbx + (axx * u + axy * v);
        dby = dby + (axy * u + ayy * v);
        const float s = border_weight(gx, a.w) * border_weight(gy, a.h);
        dbx = dbx * s, dby = dby * s, axx = axx * s, ayy = ayy * s, axy = axy * s;
        E[i] = axx * axx + axy * axy;
        E[esz + i] = (axx + ayy) * axy;
        E[2 * esz + i] = ayy * ayy + axy * axy;
        E[3 * esz + i] = axx * dbx + axy * dby;
        E[4 * esz + i] = axy * dbx + ayy * dby;
    }
    __syncthreads();
    // S66, vertical: taps from -m to +m
    for (int i = threadIdx.x; i < vsz; i += kNT) {
        const int ty = i / RW, rx = i - ty * RW;
        const float* col = E + ty * RW + rx;
        float acc[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[k] = a.kw[m] * col[k * esz];
        for (int j = 1; j <= 2 * m; ++j) {
            const float wj = a.kw[j < m ? m - j : j - m];
#pragma unroll
            for (int k = 0; k < 5; ++k) acc[k] = acc[k] + wj * col[k * esz + j * RW];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) V[k * vsz + i] = acc[k];
    }
    __syncthreads();
    // S66, horizontal, and S67
    float* FO = a.fout + (size_t)n * a.fstride;
    for (int i = threadIdx.x; i < a.TW * a.TH; i += kNT) {
        const int ty = i / a.TW, tx = i - ty * a.TW;
        const int gx = x0 + tx, gy = y0 + ty;
        if (gx >= a.w || gy >= a.h) continue;
        const float* row = V + ty * RW + tx;
        float acc[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[k] = a.kw[m] * row[k * vsz];
        for (int j = 1; j <= 2 * m; ++j) {
            const float wj = a.kw[j < m ? m - j : j - m];
#pragma unroll
            for (int k = 0; k < 5; ++k) acc[k] = acc[k] + wj * row[k * vsz + j];
        }
        const float g11 = acc[0], g12 = acc[1], g22 = acc[2], h1 = acc[3], h2 = acc[4];
        const float idet = 1.0f / ((g11 * g22 - g12 * g12) + kDetReg);
        const size_t o = (size_t)gy * a.pitch + gx;
        FO[o] = (g22 * h1 - g12 * h2) * idet;
        FO[a.fplane + o] = (g11 * h2 - g12 * h1) * idet;
    }
}

// ---------------------------------------------------------------- host side ------------------

struct Tile {
    int TW, TH;
    size_t lds;
};

int check_params(const va_farneback_params* p)
{
    VA_CHECK_ARG(p != nullptr, "va_farneback: params is NULL");
    VA_CHECK_ARG(p->struct_bytes >= (int)sizeof(va_farneback_params), "va_farneback: params.struct_bytes is %d, need at least %d",
                 p->struct_bytes, (int)sizeof(va_farneback_params));
    VA_CHECK_ARG(p->pyr_scale > 0.0f && p->pyr_scale < 1.0f, "va_farneback: pyr_scale must be in (0,1), got %g", (double)p->pyr_scale);
    VA_CHECK_ARG(p->poly_sigma > 0.0f && p->poly_sigma <= 1e3f, "va_farneback: poly_sigma must be > 0 (and <= 1e3), got %g",
                 (double)p->poly_sigma);
    VA_CHECK_ARG(p->levels >= 1, "va_farneback: levels must be >= 1, got %d", p->levels);
    VA_CHECK_ARG(p->winsize >= 3 && (p->winsize & 1) == 1 && p->winsize <= 2 * kMaxRadius + 1,
                 "va_farneback: winsize must be odd and in [3,%d], got %d", 2 * kMaxRadius + 1, p->winsize);
    VA_CHECK_ARG(p->iterations >= 1, "va_farneback: iterations must be >= 1, got %d", p->iterations);
    VA_CHECK_ARG(p->poly_n == 5 || p->poly_n == 7, "va_farneback: poly_n must be 5 or 7, got %d", p->poly_n);
    VA_CHECK_ARG(p->gaussian == 0 || p->gaussian == 1, "va_farneback: gaussian must be 0 or 1, got %d", p->gaussian);
    const int* t = p->tuning;
    for (int k = 0; k < 4; ++k)
        VA_CHECK_ARG(t[k] == 0 || (t[k] >= 1 && t[k] <= 256), "va_farneback: tuning[%d] (a tile side) must be 0 or in [1,256]", k);
    VA_CHECK_ARG(t[4] == 0 && t[5] == 0 && t[6] == 0 && t[7] == 0, "va_farneback: tuning[4..7] are reserved, must be 0");
    return VA_OK;
}

int poly_tile(const va_farneback_params* p, Tile* t)
{
    const int n = p->poly_n;
    t->TW = p->tuning[VA_FARNEBACK_TUNE_POLY_TILE_W] ? p->tuning[VA_FARNEBACK_TUNE_POLY_TILE_W] : kDefTileW;
    t->TH = p->tuning[VA_FARNEBACK_TUNE_POLY_TILE_H] ? p->tuning[VA_FARNEBACK_TUNE_POLY_TILE_H] : kDefTileH;
    const size_t rw = t->TW + 2 * n, rh = t->TH + 2 * n;
    t->lds = (rw * rh + 3 * rw * t->TH) * sizeof(float);
    VA_CHECK_ARG(t->lds <= (size_t)kVaMaxLds,
                 "va_farneback: tuning: a %d x %d tile of the polynomial expansion with poly_n %d needs %zu bytes of LDS, more than one "
                 "workgroup holds (%d)", t->TW, t->TH, n, t->lds, kVaMaxLds);
    return VA_OK;
}

int pass_tile(const va_farneback_params* p, Tile* t)
{
    const int m = p->winsize / 2;
    const bool own = p->tuning[VA_FARNEBACK_TUNE_PASS_TILE_W] || p->tuning[VA_FARNEBACK_TUNE_PASS_TILE_H];
    t->TW = p->tuning[VA_FARNEBACK_TUNE_PASS_TILE_W] ? p->tuning[VA_FARNEBACK_TUNE_PASS_TILE_W] : kDefTileW;
    t->TH = p->tuning[VA_FARNEBACK_TUNE_PASS_TILE_H] ? p->tuning[VA_FARNEBACK_TUNE_PASS_TILE_H] : kDefTileH;
    for (;;) {
        const size_t rw = t->TW + 2 * m, rh = t->TH + 2 * m;
        t->lds = 5 * (rw * rh + rw * t->TH) * sizeof(float);
        if (t->lds <= (size_t)kVaMaxLds) return VA_OK;
        // (the library's own tile halves until the window fits beside it: 16 x 16 holds the largest window; a caller's is refused)
        VA_CHECK_ARG(!own && t->TW * t->TH > 64,
                     "va_farneback: tuning: a %d x %d tile of the pass with winsize %d needs %zu bytes of LDS, more than one workgroup "
                     "holds (%d)", t->TW, t->TH, p->winsize, t->lds, kVaMaxLds);
        if (t->TW > t->TH) t->TW /= 2; else t->TH /= 2;
    }
}

// S64's constants: the taps in float64 rounded to float32, the inverse moment matrix in closed form
void fill_poly(PolyArgs& a, const va_farneback_params* p)
{
    const int n = p->poly_n;
    const double sigma = (double)p->poly_sigma;
    double e[8], s;
    for (int k = 0; k <= n; ++k) e[k] = exp(-(double)(k * k) / (2.0 * sigma * sigma));
    s = e[0];
    for (int k = 1; k <= n; ++k) s = s + 2.0 * e[k];
    double m2 = 0.0, m4 = 0.0;
    for (int k = 0; k < 8; ++k) a.g[k] = a.xg[k] = a.xxg[k] = 0.0f;
    for (int k = 0; k <= n; ++k) {
        const double g = e[k] / s, k2 = (double)(k * k);
        a.g[k] = (float)g;
        a.xg[k] = (float)((double)k * g);
        a.xxg[k] = (float)(k2 * g);
        m2 = m2 + 2.0 * (k2 * g);
        m4 = m4 + 2.0 * ((k2 * k2) * g);
    }
    const double d = m4 - m2 * m2;
    a.ig11 = (float)(1.0 / m2);
    a.ig03 = (float)(-m2 / d);
    a.ig33 = (float)(1.0 / d);
    a.ig55 = (float)(1.0 / (m2 * m2));
}

// S66's taps: 1 / winsize each, or the Gaussian of sigma = 0.3 (winsize / 2) normalised over the window
void fill_window(PassArgs& a, const va_farneback_params* p)
{
    const int m = p->winsize / 2;
    a.m = m;
    for (int i = 0; i <= kMaxRadius; ++i) a.kw[i] = 0.0f;
    if (!p->gaussian) {
        for (int i = 0; i <= m; ++i) a.kw[i] = (float)(1.0 / (double)p->winsize);
        return;
    }
    const double sigma = 0.3 * (double)m;
    double e[kMaxRadius + 1], s;
    for (int i = 0; i <= m; ++i) e[i] = exp(-(double)(i * i) / (2.0 * sigma * sigma));
    s = e[0];
    for (int i = 1; i <= m; ++i) s = s + 2.0 * e[i];
    for (int i = 0; i <= m; ++i) a.kw[i] = (float)(e[i] / s);
}

int launch_poly(PolyArgs a, const Tile& t, int poly_n, int nframes, hipStream_t st)
{
    a.TW = t.TW, a.TH = t.TH, a.ntx = va_cdiv(a.w, t.TW);
    const dim3 grid(a.ntx * va_cdiv(a.h, t.TH), nframes);
    if (poly_n == 5) {
        if (int rc = va_allow_lds(&k_farneback_polyexp<5>, t.lds)) return rc;
        k_farneback_polyexp<5><<<grid, kNT, t.lds, st>>>(a);
    } else {
        if (int rc = va_allow_lds(&k_farneback_polyexp<7>, t.lds)) return rc;
        k_farneback_polyexp<7><<<grid, kNT, t.lds, st>>>(a);
    }
    VA_LAUNCH_CHECK();
    return VA_OK;
}

int launch_pass(PassArgs a, const Tile& t, int npairs, hipStream_t st)
{
    a.TW = t.TW, a.TH = t.TH, a.ntx = va_cdiv(a.w, t.TW);
    const dim3 grid(a.ntx * va_cdiv(a.h, t.TH), npairs);
    if (int rc = va_allow_lds(&k_farneback_pass, t.lds)) return rc;
    k_farneback_pass<<<grid, kNT, t.lds, st>>>(a);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

struct Plan : va_flow_levels {
    Tile poly, pass;
    size_t off_pyr[kVaMaxScales], off_tmp, off_coef, off_state, off_up, total;
};

int make_plan(Plan& P, int w, int h, int n_seq, int fps, const va_farneback_params* p)
{
    if (int rc = check_params(p)) return rc;
    if (int rc = poly_tile(p, &P.poly)) return rc;
    if (int rc = pass_tile(p, &P.pass)) return rc;
    if (int rc = va_flow_check_shape("va_farneback", w, h, n_seq, fps, true)) return rc;
    va_flow_levels_fill(&P, w, h, n_seq, fps, p->pyr_scale, p->levels);
    size_t off = 0;
    for (int s = 0; s < P.ns; ++s) {
        P.off_pyr[s] = off;
        off += va_align_up((size_t)P.NF * 3 * P.plane[s] * sizeof(float), 256);
    }
    P.off_tmp = off;
    off += va_align_up((size_t)P.NF * 2 * P.plane_max * sizeof(float), 256);
    P.off_coef = off;
    off += va_align_up((size_t)P.NF * 5 * P.plane_max * sizeof(float), 256);
    P.off_state = off;
    off += va_align_up((size_t)P.NP * 6 * P.plane_max * sizeof(float), 256);
    P.off_up = off;
    off += va_align_up((size_t)P.NP * 2 * P.plane_max * sizeof(float), 256);
    P.total = off;
    return VA_OK;
}

}  // namespace

extern "C" void va_farneback_default_params(va_farneback_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_bytes = (int)sizeof(va_farneback_params);
    p->pyr_scale = 0.5f;
    p->poly_sigma = 1.2f;
    p->levels = 3;
    p->winsize = 15;
    p->iterations = 3;
    p->poly_n = 5;
    p->gaussian = 0;
}

extern "C" size_t va_farneback_workspace_bytes(int w, int h, int n_seq, int frames_per_seq, const va_farneback_params* p)
{
    Plan P;
    if (make_plan(P, w, h, n_seq, frames_per_seq, p) != VA_OK) return 0;
    return P.total;
}

extern "C" int va_farneback_flow(va_ctx* ctx, const void* frames, int frames_are_u8, int n_seq, int frames_per_seq, int w, int h,
                                 const va_farneback_params* p, void* flow, void* workspace, size_t workspace_bytes, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_farneback_flow: ctx is NULL");
    VA_USE_DEVICE(ctx);
    if (int rc = va_flow_check_buffers("va_farneback_flow", frames, flow, workspace, 0, 0)) return rc;
    Plan P;
    if (int rc = make_plan(P, w, h, n_seq, frames_per_seq, p)) return rc;
    if (int rc = va_flow_check_buffers("va_farneback_flow", frames, flow, workspace, workspace_bytes, P.total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* pyr[kVaMaxScales];
    for (int s = 0; s < P.ns; ++s) pyr[s] = (float*)(ws + P.off_pyr[s]);
    float* tmp1 = (float*)(ws + P.off_tmp);
    float* tmp2 = tmp1 + (size_t)P.NF * P.plane_max;
    float* coef = (float*)(ws + P.off_coef);
    float* state = (float*)(ws + P.off_state);
    float* up = (float*)(ws + P.off_up);

    // S63: the frames as they are, S1's pyramid
    if (int rc = va_stage_frames(frames, frames_are_u8, false, pyr[0], w, h, P.pitch[0], P.plane[0], P.NF, st)) return rc;
    if (int rc = va_stage_pyramid(pyr, P.ws, P.hs, P.pitch, P.plane, P.ns, P.NF, tmp1, tmp2, P.plane_max, p->pyr_scale, st)) return rc;

    PolyArgs pa{};
    fill_poly(pa, p);
    PassArgs qa{};
    fill_window(qa, p);
    // the flow is 0 at the coarsest level (padding included)
    const int sc = P.ns - 1;
    VA_HIP(hipMemsetAsync(state, 0, (size_t)P.NP * 6 * P.plane[sc] * sizeof(float), st));
    int cur = 0;  // the flow is in planes (2 cur, 2 cur + 1) of the state
    for (int s = sc; s >= 0; --s) {
        const int lw = P.ws[s], lh = P.hs[s], lp = P.pitch[s];
        const size_t pl = P.plane[s];
        // S64: every frame once
        pa.src = pyr[s], pa.sstride = 3 * pl;
        pa.dst = coef, pa.dstride = 5 * pl, pa.dplane = pl;
        pa.w = lw, pa.h = lh, pa.pitch = lp;
        if (int rc = launch_poly(pa, P.poly, p->poly_n, P.NF, st)) return rc;
        // S65-S67
        qa.r0 = coef, qa.r1 = coef + 5 * pl, qa.rstride = 5 * pl, qa.cplane = pl;
        qa.fstride = 6 * pl, qa.fplane = pl;
        qa.w = lw, qa.h = lh, qa.pitch = lp, qa.fps = P.F;
        for (int it = 0; it < p->iterations; ++it) {
            qa.fin = state + 2 * cur * pl;
            qa.fout = state + 2 * (cur ^ 1) * pl;
            if (int rc = launch_pass(qa, P.pass, P.NP, st)) return rc;
            cur ^= 1;
        }
        if (s > 0) {  // S8: into planes (0, 1) of the finer state
            if (int rc = va_stage_upsample(state + 2 * cur * pl, lw, lh, lp, pl, up, state, P.ws[s - 1], P.hs[s - 1], P.pitch[s - 1],
                                           P.plane[s - 1], 1.0f / p->pyr_scale, P.NP, st))
                return rc;
            cur = 0;
        }
    }
    return va_stage_flow_out(state + 2 * cur * P.plane[0], w, h, P.pitch[0], P.plane[0], (float*)flow, P.NP, st);
}

extern "C" int va_farneback_polyexp(va_ctx* ctx, const void* fields, int n, int w, int h, const va_farneback_params* p, void* coef,
                                    void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_farneback_polyexp: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(fields != nullptr && coef != nullptr, "va_farneback_polyexp: NULL buffer");
    if (int rc = check_params(p)) return rc;
    if (int rc = va_flow_check_fields("va_farneback_polyexp", n, w, h)) return rc;
    Tile t;
    if (int rc = poly_tile(p, &t)) return rc;
    const size_t fl = (size_t)w * h;
    PolyArgs a{};
    fill_poly(a, p);
    a.src = (const float*)fields, a.sstride = fl;
    a.dst = (float*)coef, a.dstride = 5 * fl, a.dplane = fl;
    a.w = w, a.h = h, a.pitch = w;
    return launch_poly(a, t, p->poly_n, n, (hipStream_t)stream);
}

extern "C" int va_farneback_pass(va_ctx* ctx, const void* coef0, const void* coef1, const void* flow_in, void* flow_out, int n, int w,
                                 int h, const va_farneback_params* p, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_farneback_pass: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(coef0 != nullptr && coef1 != nullptr && flow_in != nullptr && flow_out != nullptr, "va_farneback_pass: NULL buffer");
    VA_CHECK_ARG(flow_in != flow_out, "va_farneback_pass: flow_out must not be flow_in (a pass reads its neighbours' flow)");
    if (int rc = check_params(p)) return rc;
    if (int rc = va_flow_check_fields("va_farneback_pass", n, w, h)) return rc;
    Tile t;
    if (int rc = pass_tile(p, &t)) return rc;
    const size_t fl = (size_t)w * h;
    PassArgs a{};
    fill_window(a, p);
    a.r0 = (const float*)coef0, a.r1 = (const float*)coef1, a.rstride = 5 * fl, a.cplane = fl;
    a.fin = (const float*)flow_in, a.fout = (float*)flow_out, a.fstride = 2 * fl, a.fplane = fl;
    a.w = w, a.h = h, a.pitch = w, a.fps = 0;
    return launch_pass(a, t, n, (hipStream_t)stream);
}
