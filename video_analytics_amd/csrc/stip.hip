// Space-time interest points for gfx950 (MI355X): hand-written HIP, no CPU fallback.
//
// I. Laptev, "On space-time interest points" (IJCV 2005), with the constants of the modelled project's Sheet01 and HOG / HOF
// cuboid descriptors.  DESIGN.md S83-S90 fix every expression and its operation order.  The smoothing passes are float32 in
// one written order per output (centre first, then the tap pairs outwards), so a result never depends on a tile shape; the
// orientation votes are S70's polynomial quantised once to fixed point (S71's functions, va_feature_device.h), and every sum
// behind them is an integer sum.  This file is compiled with -ffp-contract=off and writes no fmaf of its own.
//
//   volumes   f32 [T][h][w]: L, the six products (smoothed in place), two pass buffers, H
//   votes     u32 [T][bins][h][w], integral planes u32 [T][bins][h+1][w+1] (va_integral_planes: S72)
//   counts    i32 [16]: [0] points found so far, [1] the count before the current scale pair
//
// The host makes the same launches whatever the counts are; kernels read the counts from the device.
#include "va_feature_device.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int kNT = 256;
constexpr int kScanNT = 1024;
constexpr int kRowsPerBlock = kNT / 64;  // k_stip_rows: one row per wave
constexpr int kDefRowTW = 256, kDefColTX = 32;
constexpr int kColMinTN = 8;
constexpr int kLdsSmall = 64 * 1024;
constexpr int kTapStride = VA_STIP_MAX_RADIUS + 1;  // floats per tap set
constexpr int kDescRounds = 8;                      // 64 descriptor values per round and wave: 512 at the most

// S88: fixed point.  Both groups clamp to VMAX 2^S = 2^17 per vote; a cell slice of at most 32767 pixels then sums to less
// than 2^32 (check_params refuses the parameters that admit a larger slice).
constexpr float kHogVmax = 512.0f, kHogScale = 256.0f;   // S = 8
constexpr float kFlowVmax = 32.0f, kFlowScale = 4096.0f;  // S = 12
constexpr double kHogUnit = 1.0 / 256.0, kFlowUnit = 1.0 / 4096.0;
constexpr long long kMaxSlice = 32767;

enum { C_FOUND = 0, C_BEGIN = 1, C_WORDS = 16 };

// S83: scipy's `reflect` (d c b a | a b c d | d c b a): period 2n, defined for every i
__device__ __forceinline__ int fold(int i, int n)
{
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// S84 along the contiguous axis.  src [rows][n]; grid (row blocks, strips); one row per wave, its TW outputs and their
// reflected halo of r on either side staged in the wave's LDS segment.  Dynamic LDS: kRowsPerBlock (TW + 2r) floats.
template <bool U8>
__global__ void __launch_bounds__(kNT) k_stip_rows(const void* __restrict__ src, float* __restrict__ dst, const float* __restrict__ g, int r,
                                                   int n, long long rows, int TW)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * kRowsPerBlock + wv;
    const int x0 = blockIdx.y * TW;
    const int SW = TW + 2 * r;
    float* seg = lds + (size_t)wv * SW;
    if (row < rows) {
        const size_t base = (size_t)row * n;
        for (int i = lane; i < SW; i += 64) {
            const size_t o = base + fold(x0 - r + i, n);
            seg[i] = U8 ? (float)((const unsigned char*)src)[o] : ((const float*)src)[o];
        }
    }
    __syncthreads();
    if (row >= rows) return;
    for (int i = lane; i < TW; i += 64) {
        const int x = x0 + i;
        if (x >= n) break;
        const float* c = seg + r + i;
        float acc = g[0] * c[0];
        for (int k = 1; k <= r; ++k) acc = acc + g[k] * (c[-k] + c[k]);
        dst[(size_t)row * n + x] = acc;
    }
}

// S84 along an outer axis.  src [batch][n][m], filtered along n (y: batch T, n h, m w; t: batch 1, n T, m h w).
// grid (tiles along m, tiles along n, batch); a tile of TX columns and TN outputs with its reflected halo.  Dynamic LDS:
// (TN + 2r) TX floats.  Lanes run along m.
__global__ void __launch_bounds__(kNT) k_stip_cols(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ g, int r,
                                                   int n, long long m, int TX, int TN)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const long long m0 = (long long)blockIdx.x * TX;
    const int n0 = blockIdx.y * TN;
    const size_t base = (size_t)blockIdx.z * n * m;
    const int SN = TN + 2 * r;
    for (int i = threadIdx.x; i < SN * TX; i += kNT) {
        const int rr = i / TX, tx = i - rr * TX;
        const long long mm = m0 + tx;
        lds[i] = mm < m ? src[base + (size_t)fold(n0 - r + rr, n) * m + mm] : 0.0f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TN * TX; i += kNT) {
        const int ty = i / TX, tx = i - ty * TX;
        const long long mm = m0 + tx;
        const int nn = n0 + ty;
        if (mm >= m || nn >= n) continue;
        const float* c = lds + (ty + r) * TX + tx;
        float acc = g[0] * c[0];
        for (int k = 1; k <= r; ++k) acc = acc + g[k] * (c[-k * TX] + c[k * TX]);
        dst[base + (size_t)nn * m + mm] = acc;
    }
}

// S85: np.gradient along one axis of stride s and length n at index i
__device__ __forceinline__ float grad1(const float* p, int i, int n, size_t s)
{
    if (n < 2) return 0.0f;
    if (i == 0) return p[s] - p[0];
    if (i == n - 1) return p[0] - *(p - s);
    return (p[s] - *(p - s)) * 0.5f;
}

__global__ void __launch_bounds__(kNT) k_stip_products(const float* __restrict__ L, float* __restrict__ P, int T, int h, int w, size_t vox)
{
    const size_t i = (size_t)blockIdx.x * kNT + threadIdx.x;
    if (i >= vox) return;
    const size_t fl = (size_t)w * h;
    const int t = (int)(i / fl);
    const size_t rem = i - (size_t)t * fl;
    const int y = (int)(rem / w), x = (int)(rem - (size_t)y * w);
    const float* p = L + i;
    const float lx = grad1(p, x, w, 1), ly = grad1(p, y, h, (size_t)w), lt = grad1(p, t, T, fl);
    P[i] = lx * lx;
    P[vox + i] = ly * ly;
    P[2 * vox + i] = lt * lt;
    P[3 * vox + i] = lx * ly;
    P[4 * vox + i] = lx * lt;
    P[5 * vox + i] = ly * lt;
}

// S86
__global__ void __launch_bounds__(kNT) k_stip_response(const float* __restrict__ P, float* __restrict__ H, float k, size_t vox)
{
    const size_t i = (size_t)blockIdx.x * kNT + threadIdx.x;
    if (i >= vox) return;
    const float xx = P[i], yy = P[vox + i], tt = P[2 * vox + i], xy = P[3 * vox + i], xt = P[4 * vox + i], yt = P[5 * vox + i];
    const float a = yy * tt - yt * yt;
    const float b = xy * tt - yt * xt;
    const float c = xy * yt - yy * xt;
    const float det = (xx * a - xy * b) + xt * c;
    const float tr = (xx + yy) + tt;
    H[i] = det - k * ((tr * tr) * tr);
}

struct MaxArgs {
    const float* H;
    int T, h, w;
    float min_response;
    int full;  // 26 neighbours
};

// S87: is voxel (x, y, t) a point?  Faces never qualify; a NaN anywhere in the comparison disqualifies.
__device__ __forceinline__ bool is_point(const MaxArgs& a, int x, int y, int t)
{
    if (x < 1 || y < 1 || t < 1 || x >= a.w - 1 || y >= a.h - 1 || t >= a.T - 1) return false;
    const size_t fl = (size_t)a.w * a.h;
    const float* p = a.H + (size_t)t * fl + (size_t)y * a.w + x;
    const float v = p[0];
    if (!(fabsf(v) <= 3.4028234663852886e38f) || !(v > a.min_response)) return false;
    if (!a.full) {
        const ptrdiff_t sw = a.w, sf = (ptrdiff_t)fl;
        return v > p[-1] && v > p[1] && v > p[-sw] && v > p[sw] && v > p[-sf] && v > p[sf];
    }
    bool ok = true;
    for (int dt = -1; dt <= 1; ++dt)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (dt == 0 && dy == 0 && dx == 0) continue;
                ok = ok && v > p[(ptrdiff_t)dt * (ptrdiff_t)fl + (ptrdiff_t)dy * a.w + dx];
            }
    return ok;
}

// S87, first pass: one wave per row (t, y) counts its points
__global__ void __launch_bounds__(kNT) k_stip_count(MaxArgs a, int* __restrict__ rowcnt, long long rows)
{
    const long long row = (long long)blockIdx.x * (kNT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int t = (int)(row / a.h), y = (int)(row - (long long)t * a.h);
    int n = 0;
    for (int x0 = 0; x0 < a.w; x0 += 64) n += __popcll(__ballot(is_point(a, x0 + lane, y, t)));
    if (lane == 0) rowcnt[row] = n;
}

// S87, second pass: one workgroup turns the row counts into row offsets behind the points found so far, and moves the counts
__global__ void __launch_bounds__(kScanNT) k_stip_scan(const int* __restrict__ rowcnt, int* __restrict__ rowoff, long long rows, int* counts)
{
    __shared__ int sh[kScanNT / 64 + 1];
    const int base = counts[C_FOUND];
    int run = 0;
    __syncthreads();
    for (long long r0 = 0; r0 < rows; r0 += kScanNT) {
        const long long r = r0 + threadIdx.x;
        int total;
        const int before = va_wg_scan_excl<kScanNT>(r < rows ? rowcnt[r] : 0, total, sh);
        if (r < rows) rowoff[r] = base + run + before;
        run += total;
    }
    if (threadIdx.x == 0) {
        counts[C_BEGIN] = base;
        counts[C_FOUND] = base + run;
    }
}

// S87, third pass: the same wave per row writes its points in x order behind its offset; nothing lands past the capacity
__global__ void __launch_bounds__(kNT) k_stip_write(MaxArgs a, const int* __restrict__ rowoff, long long rows, int si, int ti, int* __restrict__ points,
                                                    float* __restrict__ resp, int capacity)
{
    const long long row = (long long)blockIdx.x * (kNT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int t = (int)(row / a.h), y = (int)(row - (long long)t * a.h);
    int off = rowoff[row];
    for (int x0 = 0; x0 < a.w; x0 += 64) {
        const int x = x0 + lane;
        const bool f = is_point(a, x, y, t);
        const unsigned long long mask = __ballot(f);
        const int idx = off + __popcll(mask & ((1ull << lane) - 1ull));
        if (f && idx >= 0 && idx < capacity) {
            int* q = points + (size_t)idx * 5;
            q[0] = x, q[1] = y, q[2] = t, q[3] = si, q[4] = ti;
            resp[idx] = a.H[((size_t)t * a.h + y) * a.w + x];
        }
        off += __popcll(mask);
    }
}

// S88: the votes of (Lx, Ly) of this scale's L -> u32 [T][bins][h][w]
__global__ void __launch_bounds__(kNT) k_stip_votes_hog(const float* __restrict__ L, unsigned* __restrict__ out, int T, int h, int w, int bins, size_t vox)
{
    const size_t i = (size_t)blockIdx.x * kNT + threadIdx.x;
    if (i >= vox) return;
    const size_t fl = (size_t)w * h;
    const int t = (int)(i / fl);
    const size_t rem = i - (size_t)t * fl;
    const int y = (int)(rem / w), x = (int)(rem - (size_t)y * w);
    const float lx = grad1(L + i, x, w, 1), ly = grad1(L + i, y, h, (size_t)w);
    int b0;
    unsigned q0, q1;
    float m;
    va_votes_of(lx, ly, kHogVmax, kHogScale, bins, b0, q0, q1, m);
    va_store_bins(out + (size_t)t * bins * fl + rem, fl, bins, b0, q0, q1);
}

// S88: the votes of the flow; frame t reads the field of pair min(t, T - 2)
__global__ void __launch_bounds__(kNT) k_stip_votes_hof(const float* __restrict__ flow, unsigned* __restrict__ out, int T, int h, int w, int bins, size_t vox)
{
    const size_t i = (size_t)blockIdx.x * kNT + threadIdx.x;
    if (i >= vox) return;
    const size_t fl = (size_t)w * h;
    const int t = (int)(i / fl);
    const size_t rem = i - (size_t)t * fl;
    const int ft = d_min(t, T - 2);
    const float* u = flow + (size_t)ft * 2 * fl + rem;
    int b0;
    unsigned q0, q1;
    float m;
    va_votes_of(u[0], u[fl], kFlowVmax, kFlowScale, bins, b0, q0, q1, m);
    va_store_bins(out + (size_t)t * bins * fl + rem, fl, bins, b0, q0, q1);
}

struct DescArgs {
    const int* points;          // [n][5]
    const int* counts;          // device counts, or NULL: the points are [0, n)
    int n, capacity;
    const unsigned* hogI;       // [T][bins][h+1][w+1]
    const unsigned* hofI;
    float* desc;
    int T, h, w, nx, ny, nt, bins;
    double cuboid;
    double sigmas[VA_STIP_MAX_SIGMAS], taus[VA_STIP_MAX_TAUS];
};

// S89: cell edge j of n cells across a side of delta centred on c, inside [0, size]
__device__ __forceinline__ int cell_edge(int c, double delta, int j, int n, int size)
{
    const double e = rint(((double)c - delta / 2.0) + ((double)j * delta) / (double)n);
    return (int)fmin(fmax(e, 0.0), (double)size);
}

// S89: one wave per point.  Every lane sums its descriptor values over the frames of their cells in 64-bit integers; then all
// lanes add the float64 squares in index order, so all hold the same norm.
__global__ void __launch_bounds__(kNT) k_stip_describe(DescArgs a)
{
    int first = 0, last = a.n;
    if (a.counts) first = a.counts[C_BEGIN], last = d_min(a.counts[C_FOUND], a.capacity);
    const int lane = threadIdx.x & 63;
    const int ncell = a.nx * a.ny * a.nt, half = ncell * a.bins, dim = 2 * half;
    const int W1 = a.w + 1;
    const size_t ipl = (size_t)(a.h + 1) * W1;
    for (int j = first + blockIdx.x * (kNT / 64) + (threadIdx.x >> 6); j < last; j += gridDim.x * (kNT / 64)) {
        const int* q = a.points + (size_t)j * 5;
        const int px = q[0], py = q[1], pt = q[2];
        const int si = d_min(d_max(q[3], 0), VA_STIP_MAX_SIGMAS - 1), ti = d_min(d_max(q[4], 0), VA_STIP_MAX_TAUS - 1);
        const double dxy = (2.0 * a.cuboid) * a.sigmas[si], dt = (2.0 * a.cuboid) * a.taus[ti];
        unsigned long long acc[kDescRounds];
        double ss = 0.0;
#pragma unroll
        for (int r = 0; r < kDescRounds; ++r) {
            acc[r] = 0ull;
            if (r * 64 >= dim) continue;
            const int e = r * 64 + lane;
            if (e < dim) {
                const int grp = e >= half, rem = e - grp * half;
                const int cell = rem / a.bins, bin = rem - cell * a.bins;
                const int ct = cell / (a.nx * a.ny), cyx = cell - ct * (a.nx * a.ny);
                const int cy = cyx / a.nx, cx = cyx - cy * a.nx;
                const int xa = cell_edge(px, dxy, cx, a.nx, a.w), xb = cell_edge(px, dxy, cx + 1, a.nx, a.w);
                const int ya = cell_edge(py, dxy, cy, a.ny, a.h), yb = cell_edge(py, dxy, cy + 1, a.ny, a.h);
                const int ta = cell_edge(pt, dt, ct, a.nt, a.T), tb = cell_edge(pt, dt, ct + 1, a.nt, a.T);
                if (xb > xa && yb > ya) {
                    const unsigned* I = (grp ? a.hofI : a.hogI) + (size_t)bin * ipl;
                    unsigned long long s = 0ull;
                    for (int f = ta; f < tb; ++f) {
                        const unsigned* Ip = I + (size_t)f * a.bins * ipl;
                        const unsigned v = Ip[(size_t)yb * W1 + xb] - Ip[(size_t)ya * W1 + xb] - Ip[(size_t)yb * W1 + xa] + Ip[(size_t)ya * W1 + xa];
                        s += v;
                    }
                    acc[r] = s;
                }
            }
            const double v = e < dim ? (double)acc[r] * (e >= half ? kFlowUnit : kHogUnit) : 0.0;
            const double sq = v * v;
#pragma unroll
            for (int i = 0; i < 64; ++i) ss = ss + __shfl(sq, i);
        }
        const double norm = sqrt(ss);
        float* D = a.desc + (size_t)j * dim;
#pragma unroll
        for (int r = 0; r < kDescRounds; ++r) {
            const int e = r * 64 + lane;
            if (e < dim) {
                const double v = (double)acc[r] * (e >= half ? kFlowUnit : kHogUnit);
                D[e] = norm > 0.0 ? (float)(v / norm) : 0.0f;
            }
        }
    }
}

// ---------------------------------------------------------------- host side ------------------

// S83: r and the float32 taps of sigma; false when sigma admits none
bool make_taps(double sigma, int* r_out, float* g)
{
    if (!(sigma > 0.0) || !(sigma <= 1e6)) return false;
    const int r = (int)(4.0 * sigma + 0.5);
    if (r > VA_STIP_MAX_RADIUS) return false;
    double wgt[VA_STIP_MAX_RADIUS + 1];
    const double d = 2.0 * sigma * sigma;
    for (int k = 0; k <= r; ++k) wgt[k] = exp(-((double)k * (double)k) / d);
    double s = wgt[0];
    for (int k = 1; k <= r; ++k) s = s + (wgt[k] + wgt[k]);
    for (int k = 0; k <= r; ++k) g[k] = (float)(wgt[k] / s);
    *r_out = r;
    return true;
}

struct Tune {
    int row_tw, col_tx, col_tn;
};

int check_tuning(const char* who, const int* t, Tune* tu)
{
    VA_CHECK_ARG(t[VA_STIP_TUNE_ROW_TILE_W] >= 0 && t[VA_STIP_TUNE_ROW_TILE_W] <= 4096, "%s: tuning[0] (strip width of the row pass) must be 0 or in [1,4096], got %d",
                 who, t[VA_STIP_TUNE_ROW_TILE_W]);
    VA_CHECK_ARG(t[VA_STIP_TUNE_COL_TILE_W] >= 0 && t[VA_STIP_TUNE_COL_TILE_W] <= 64, "%s: tuning[1] (tile width of the column pass) must be 0 or in [1,64], got %d",
                 who, t[VA_STIP_TUNE_COL_TILE_W]);
    VA_CHECK_ARG(t[VA_STIP_TUNE_COL_TILE_N] >= 0 && t[VA_STIP_TUNE_COL_TILE_N] <= 1024, "%s: tuning[2] (tile length of the column pass) must be 0 or in [1,1024], got %d",
                 who, t[VA_STIP_TUNE_COL_TILE_N]);
    VA_CHECK_ARG(t[3] == 0 && t[4] == 0 && t[5] == 0 && t[6] == 0 && t[7] == 0, "%s: tuning[3..7] are reserved, must be 0", who);
    tu->row_tw = t[VA_STIP_TUNE_ROW_TILE_W] ? t[VA_STIP_TUNE_ROW_TILE_W] : kDefRowTW;
    tu->col_tx = t[VA_STIP_TUNE_COL_TILE_W] ? t[VA_STIP_TUNE_COL_TILE_W] : kDefColTX;
    tu->col_tn = t[VA_STIP_TUNE_COL_TILE_N];
    return VA_OK;
}

int check_params(const char* who, const va_stip_params* p, Tune* tu)
{
    VA_CHECK_ARG(p != nullptr, "%s: params is NULL", who);
    VA_CHECK_ARG(p->struct_bytes >= (int)sizeof(va_stip_params), "%s: params.struct_bytes is %d, need at least %d", who, p->struct_bytes,
                 (int)sizeof(va_stip_params));
    VA_CHECK_ARG(p->n_sigmas >= 1 && p->n_sigmas <= VA_STIP_MAX_SIGMAS, "%s: n_sigmas must be in [1,%d], got %d", who, VA_STIP_MAX_SIGMAS, p->n_sigmas);
    VA_CHECK_ARG(p->n_taus >= 1 && p->n_taus <= VA_STIP_MAX_TAUS, "%s: n_taus must be in [1,%d], got %d", who, VA_STIP_MAX_TAUS, p->n_taus);
    VA_CHECK_ARG(p->integration >= 1.0f && p->integration <= 16.0f, "%s: integration must be in [1,16], got %g", who, (double)p->integration);
    int r;
    float g[kTapStride];
    double smax = 0.0;
    for (int i = 0; i < p->n_sigmas; ++i) {
        VA_CHECK_ARG(make_taps((double)p->sigmas[i], &r, g) && make_taps((double)p->integration * (double)p->sigmas[i], &r, g),
                     "%s: sigmas[%d] must be > 0 with a radius int(4 integration sigma + 0.5) <= %d, got %g", who, i, VA_STIP_MAX_RADIUS,
                     (double)p->sigmas[i]);
        smax = std::max(smax, (double)p->sigmas[i]);
    }
    for (int i = 0; i < p->n_taus; ++i)
        VA_CHECK_ARG(make_taps((double)p->taus[i], &r, g) && make_taps((double)p->integration * (double)p->taus[i], &r, g),
                     "%s: taus[%d] must be > 0 with a radius int(4 integration tau + 0.5) <= %d, got %g", who, i, VA_STIP_MAX_RADIUS,
                     (double)p->taus[i]);
    VA_CHECK_ARG(p->k >= 0.0f && p->k <= 1.0f, "%s: k must be in [0,1], got %g", who, (double)p->k);
    VA_CHECK_ARG(p->min_response >= 0.0f && p->min_response <= 3e38f, "%s: min_response must be >= 0 and finite, got %g", who, (double)p->min_response);
    VA_CHECK_ARG(p->cuboid > 0.0f && p->cuboid <= 64.0f, "%s: cuboid must be in (0,64], got %g", who, (double)p->cuboid);
    VA_CHECK_ARG(p->neighbours == 6 || p->neighbours == 26, "%s: neighbours must be 6 or 26, got %d", who, p->neighbours);
    VA_CHECK_ARG(p->nx >= 1 && p->nx <= 8, "%s: nx must be in [1,8], got %d", who, p->nx);
    VA_CHECK_ARG(p->ny >= 1 && p->ny <= 8, "%s: ny must be in [1,8], got %d", who, p->ny);
    VA_CHECK_ARG(p->nt >= 1 && p->nt <= 8, "%s: nt must be in [1,8], got %d", who, p->nt);
    VA_CHECK_ARG(p->bins >= 2 && p->bins <= 16, "%s: bins must be in [2,16], got %d", who, p->bins);
    VA_CHECK_ARG(2 * p->nx * p->ny * p->nt * p->bins <= 64 * kDescRounds, "%s: the descriptor length 2 nx ny nt bins is %d, at most %d", who,
                 2 * p->nx * p->ny * p->nt * p->bins, 64 * kDescRounds);
    // S88: rounded edges lie at most delta / n + 1 apart
    const double side = 2.0 * (double)p->cuboid * smax;
    const long long slice = ((long long)std::ceil(side / p->nx) + 1) * ((long long)std::ceil(side / p->ny) + 1);
    VA_CHECK_ARG(slice <= kMaxSlice,
                 "%s: cuboid %g at sigma %g with nx %d, ny %d admits a cell slice of %lld pixels: more than %lld could overflow its 32-bit sum", who,
                 (double)p->cuboid, smax, p->nx, p->ny, slice, kMaxSlice);
    return check_tuning(who, p->tuning, tu);
}

int check_volume(const char* who, int T, int w, int h, int tmin)
{
    VA_CHECK_ARG(w >= 1 && h >= 1 && w <= 16384 && h <= 16384, "%s: frame size %d x %d out of range (w, h in [1,16384])", who, w, h);
    VA_CHECK_ARG(T >= tmin && T <= 65535, "%s: n_frames must be in [%d,65535], got %d", who, tmin, T);
    VA_CHECK_ARG((long long)T * w * h <= 0x7fffffffLL, "%s: a volume of %d x %d x %d is 2^31 voxels or more", who, T, h, w);
    return VA_OK;
}

int launch_rows(const void* src, int u8, float* dst, const float* g, int r, int n, long long rows, const Tune& tu, hipStream_t st)
{
    const int TW = tu.row_tw;
    const size_t lds = (size_t)kRowsPerBlock * (TW + 2 * r) * sizeof(float);
    const long long gx = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
    VA_CHECK_ARG(lds <= (size_t)kLdsSmall && gx <= 0x7fffffffLL, "va_stip: the row pass with strip %d and radius %d needs %zu bytes of LDS", TW, r, lds);
    const dim3 grid((unsigned)gx, va_cdiv(n, TW));
    if (u8)
        k_stip_rows<true><<<grid, kNT, lds, st>>>(src, dst, g, r, n, rows, TW);
    else
        k_stip_rows<false><<<grid, kNT, lds, st>>>(src, dst, g, r, n, rows, TW);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

// the tile length the dispatcher picks: what a 64 KB tile holds behind its halo, at least kColMinTN, no more than the axis
int col_tile_n(int r, int n, int TX, int forced)
{
    if (forced) return forced;
    const int rows_small = kLdsSmall / (TX * (int)sizeof(float));
    return std::max(kColMinTN, std::min(n, rows_small - 2 * r));
}

int launch_cols(const float* src, float* dst, const float* g, int r, int n, long long m, int batch, const Tune& tu, hipStream_t st)
{
    const int TX = tu.col_tx, TN = col_tile_n(r, n, TX, tu.col_tn);
    const size_t lds = (size_t)(TN + 2 * r) * TX * sizeof(float);
    VA_CHECK_ARG(lds <= (size_t)kVaMaxLds, "va_stip: tuning: a column tile of %d x %d with radius %d needs %zu bytes of LDS, more than one workgroup holds (%d)",
                 TX, TN, r, lds, kVaMaxLds);
    const long long gx = (m + TX - 1) / TX;
    VA_CHECK_ARG(gx <= 0x7fffffffLL && va_cdiv(n, TN) <= 65535 && batch <= 65535, "va_stip: the column pass over %d x %lld x %d is more than one launch holds",
                 n, m, batch);
    if (int rc = va_allow_lds(&k_stip_cols, lds)) return rc;
    k_stip_cols<<<dim3((unsigned)gx, va_cdiv(n, TN), batch), kNT, lds, st>>>(src, dst, g, r, n, m, TX, TN);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

// S84: x (src -> A), y (A -> B), t (B -> dst); gxy and gt on the device
int smooth3(const void* src, int u8, float* dst, float* A, float* B, const float* gxy, int rxy, const float* gt, int rt, int T, int h, int w,
            const Tune& tu, hipStream_t st)
{
    if (int rc = launch_rows(src, u8, A, gxy, rxy, w, (long long)T * h, tu, st)) return rc;
    if (int rc = launch_cols(A, B, gxy, rxy, h, w, T, tu, st)) return rc;
    return launch_cols(B, dst, gt, rt, T, (long long)w * h, 1, tu, st);
}

unsigned blocks_of(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

int launch_products(const float* L, float* P, int T, int h, int w, hipStream_t st)
{
    const size_t vox = (size_t)T * h * w;
    k_stip_products<<<blocks_of(vox, kNT), kNT, 0, st>>>(L, P, T, h, w, vox);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

int launch_response(const float* P, float* H, float k, size_t vox, hipStream_t st)
{
    k_stip_response<<<blocks_of(vox, kNT), kNT, 0, st>>>(P, H, k, vox);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

int launch_maxima(const float* H, int T, int h, int w, float min_response, int neighbours, int si, int ti, int* points, float* resp, int capacity,
                  int* counts, int* scratch, hipStream_t st)
{
    MaxArgs a{H, T, h, w, min_response, neighbours == 26};
    const long long rows = (long long)T * h;
    int* rowcnt = scratch;
    int* rowoff = scratch + va_align_up((size_t)rows, 64);
    const unsigned g = blocks_of((size_t)rows, kNT / 64);
    k_stip_count<<<g, kNT, 0, st>>>(a, rowcnt, rows);
    VA_LAUNCH_CHECK();
    k_stip_scan<<<1, kScanNT, 0, st>>>(rowcnt, rowoff, rows, counts);
    VA_LAUNCH_CHECK();
    k_stip_write<<<g, kNT, 0, st>>>(a, rowoff, rows, si, ti, points, resp, capacity);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

int launch_votes(const float* L, const float* flow, int T, int h, int w, int bins, unsigned* hog, unsigned* hof, hipStream_t st)
{
    const size_t vox = (size_t)T * h * w;
    if (hog) {
        k_stip_votes_hog<<<blocks_of(vox, kNT), kNT, 0, st>>>(L, hog, T, h, w, bins, vox);
        VA_LAUNCH_CHECK();
    }
    if (hof) {
        k_stip_votes_hof<<<blocks_of(vox, kNT), kNT, 0, st>>>(flow, hof, T, h, w, bins, vox);
        VA_LAUNCH_CHECK();
    }
    return VA_OK;
}

int launch_describe(const va_stip_params* p, const int* points, const int* counts, int n, int capacity, const unsigned* hogI, const unsigned* hofI,
                    int T, int h, int w, float* desc, hipStream_t st)
{
    DescArgs a{};
    a.points = points, a.counts = counts, a.n = n, a.capacity = capacity, a.hogI = hogI, a.hofI = hofI, a.desc = desc;
    a.T = T, a.h = h, a.w = w, a.nx = p->nx, a.ny = p->ny, a.nt = p->nt, a.bins = p->bins;
    a.cuboid = (double)p->cuboid;
    for (int i = 0; i < VA_STIP_MAX_SIGMAS; ++i) a.sigmas[i] = i < p->n_sigmas ? (double)p->sigmas[i] : 1.0;
    for (int i = 0; i < VA_STIP_MAX_TAUS; ++i) a.taus[i] = i < p->n_taus ? (double)p->taus[i] : 1.0;
    const int want = counts ? 2048 : std::max(1, std::min(va_cdiv(n, kNT / 64), 2048));
    k_stip_describe<<<want, kNT, 0, st>>>(a);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

struct Plan {
    Tune tu;
    size_t vox, total;
    float *taps, *L, *Pr, *A, *B, *H;
    int *counts, *rows;
    unsigned *votes, *hogI, *hofI;
};

// the argument checks, and the workspace cut from `base` (NULL: the size alone)
int make_plan(Plan& P, const char* who, int w, int h, int T, int capacity, const va_stip_params* p, void* base)
{
    if (int rc = check_params(who, p, &P.tu)) return rc;
    if (int rc = check_volume(who, T, w, h, 2)) return rc;
    VA_CHECK_ARG(capacity >= 1, "%s: capacity must be >= 1, got %d", who, capacity);
    const long long bound = (long long)((w + 1) / 2) * h * T * p->n_sigmas * p->n_taus;
    VA_CHECK_ARG(bound <= 0x7fffffffLL, "%s: %d scale pairs of a %d x %d x %d volume could yield 2^31 points or more", who, p->n_sigmas * p->n_taus, T,
                 h, w);
    P.vox = (size_t)T * h * w;
    VA_CHECK_ARG((long long)T * p->bins <= 0x7fffffffLL / 4, "%s: too many vote planes", who);
    const size_t integral = (size_t)T * p->bins * (h + 1) * (w + 1);
    va_carver ws{base};
    P.taps = ws.take<float>((size_t)(VA_STIP_MAX_SIGMAS + VA_STIP_MAX_TAUS) * 2 * kTapStride);
    P.counts = ws.take<int>(C_WORDS);
    P.rows = ws.take<int>(2 * va_align_up((size_t)T * h, 64));
    P.L = ws.take<float>(P.vox);
    P.Pr = ws.take<float>(6 * P.vox);
    P.A = ws.take<float>(P.vox);
    P.B = ws.take<float>(P.vox);
    P.H = ws.take<float>(P.vox);
    P.votes = ws.take<unsigned>(P.vox * p->bins);
    P.hogI = ws.take<unsigned>(integral);
    P.hofI = ws.take<unsigned>(integral);
    P.total = ws.off;
    return VA_OK;
}

}  // namespace

extern "C" void va_stip_default_params(va_stip_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_bytes = (int)sizeof(va_stip_params);
    p->n_sigmas = 6;
    p->n_taus = 2;
    for (int i = 1; i <= 6; ++i) p->sigmas[i - 1] = (float)pow(2.0, (1.0 + i) / 2.0);
    for (int j = 1; j <= 2; ++j) p->taus[j - 1] = (float)pow(2.0, j / 2.0);
    p->integration = 2.0f;
    p->k = 0.005f;
    p->min_response = 0.0f;
    p->cuboid = 9.0f;
    p->neighbours = 6;
    p->nx = 3, p->ny = 3, p->nt = 2;
    p->bins = 4;
}

extern "C" size_t va_stip_workspace_bytes(int w, int h, int n_frames, int capacity, const va_stip_params* p)
{
    Plan P;
    if (make_plan(P, "va_stip_workspace_bytes", w, h, n_frames, capacity, p, nullptr) != VA_OK) return 0;
    return P.total;
}

extern "C" int va_stip_taps(double sigma, float* taps, int capacity)
{
    int r;
    float g[kTapStride];
    if (!taps || !make_taps(sigma, &r, g) || capacity < r + 1) return -1;
    memcpy(taps, g, (size_t)(r + 1) * sizeof(float));
    return r;
}

extern "C" int va_stip_extract(va_ctx* ctx, const void* gray, int gray_is_u8, const void* flow, int n_frames, int w, int h,
                               const va_stip_params* p, void* points, void* response, void* desc, int capacity, int* count,
                               void* workspace, size_t workspace_bytes, void* stream)
{
    const char* who = "va_stip_extract";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_CHECK_ARG(gray != nullptr && flow != nullptr && points != nullptr && response != nullptr && desc != nullptr && count != nullptr &&
                     workspace != nullptr,
                 "%s: NULL buffer", who);
    VA_USE_DEVICE(ctx);
    Plan P;
    if (int rc = make_plan(P, who, w, h, n_frames, capacity, p, workspace)) return rc;
    VA_CHECK_ARG(((size_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    if (workspace_bytes < P.total) {
        va_set_error("%s: workspace of %zu bytes, need %zu", who, workspace_bytes, P.total);
        return VA_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int T = n_frames;
    // tap sets: sigma i at slot 2i, its integration scale at 2i + 1; the taus behind them likewise
    const int nsets = 2 * (VA_STIP_MAX_SIGMAS + VA_STIP_MAX_TAUS);
    std::vector<float> host((size_t)nsets * kTapStride, 0.0f);
    int radius[nsets] = {};
    for (int i = 0; i < p->n_sigmas; ++i) {
        make_taps((double)p->sigmas[i], &radius[2 * i], &host[(size_t)(2 * i) * kTapStride]);
        make_taps((double)p->integration * (double)p->sigmas[i], &radius[2 * i + 1], &host[(size_t)(2 * i + 1) * kTapStride]);
    }
    for (int j = 0; j < p->n_taus; ++j) {
        const int s = 2 * (VA_STIP_MAX_SIGMAS + j);
        make_taps((double)p->taus[j], &radius[s], &host[(size_t)s * kTapStride]);
        make_taps((double)p->integration * (double)p->taus[j], &radius[s + 1], &host[(size_t)(s + 1) * kTapStride]);
    }
    VA_HIP(hipMemcpyAsync(P.taps, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, st));
    VA_HIP(hipStreamSynchronize(st));  // `host` may go once the copy has read it
    VA_HIP(hipMemsetAsync(P.counts, 0, C_WORDS * sizeof(int), st));
    // S88: the flow's votes and their integral planes, once for all scales
    const long long planes = (long long)T * p->bins;
    if (int rc = launch_votes(nullptr, (const float*)flow, T, h, w, p->bins, nullptr, P.votes, st)) return rc;
    if (int rc = va_integral_planes(P.votes, P.hofI, planes, w, h, st)) return rc;
    for (int si = 0; si < p->n_sigmas; ++si)
        for (int ti = 0; ti < p->n_taus; ++ti) {
            const int ss = 2 * si, ts = 2 * (VA_STIP_MAX_SIGMAS + ti);
            const float* gs = P.taps + (size_t)ss * kTapStride;
            const float* gt = P.taps + (size_t)ts * kTapStride;
            if (int rc = smooth3(gray, gray_is_u8, P.L, P.A, P.B, gs, radius[ss], gt, radius[ts], T, h, w, P.tu, st)) return rc;
            if (int rc = launch_products(P.L, P.Pr, T, h, w, st)) return rc;
            for (int c = 0; c < 6; ++c) {
                float* Pc = P.Pr + (size_t)c * P.vox;
                if (int rc = smooth3(Pc, 0, Pc, P.A, P.B, gs + kTapStride, radius[ss + 1], gt + kTapStride, radius[ts + 1], T, h, w, P.tu, st)) return rc;
            }
            if (int rc = launch_response(P.Pr, P.H, p->k, P.vox, st)) return rc;
            if (int rc = launch_maxima(P.H, T, h, w, p->min_response, p->neighbours, si, ti, (int*)points, (float*)response, capacity, P.counts, P.rows, st))
                return rc;
            if (int rc = launch_votes(P.L, nullptr, T, h, w, p->bins, P.votes, nullptr, st)) return rc;
            if (int rc = va_integral_planes(P.votes, P.hogI, planes, w, h, st)) return rc;
            if (int rc = launch_describe(p, (const int*)points, P.counts, 0, capacity, P.hogI, P.hofI, T, h, w, (float*)desc, st)) return rc;
        }
    int found = 0;
    VA_HIP(hipMemcpyAsync(&found, P.counts + C_FOUND, sizeof(int), hipMemcpyDeviceToHost, st));
    VA_HIP(hipStreamSynchronize(st));
    *count = found;
    return VA_OK;
}

extern "C" int va_stip_smooth(va_ctx* ctx, const void* src, int src_is_u8, int n_frames, int w, int h, double sigma, double tau,
                              const va_stip_params* p, void* dst, void* tmp, size_t tmp_floats, void* stream)
{
    const char* who = "va_stip_smooth";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_CHECK_ARG(src != nullptr && dst != nullptr && tmp != nullptr && p != nullptr, "%s: NULL buffer", who);
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(p->struct_bytes >= (int)sizeof(va_stip_params), "%s: params.struct_bytes is %d, need at least %d", who, p->struct_bytes,
                 (int)sizeof(va_stip_params));
    Tune tu;
    if (int rc = check_tuning(who, p->tuning, &tu)) return rc;
    if (int rc = check_volume(who, n_frames, w, h, 1)) return rc;
    float host[2 * kTapStride];
    int rs, rt;
    VA_CHECK_ARG(make_taps(sigma, &rs, host), "%s: sigma must be > 0 with a radius int(4 sigma + 0.5) <= %d, got %g", who, VA_STIP_MAX_RADIUS, sigma);
    VA_CHECK_ARG(make_taps(tau, &rt, host + kTapStride), "%s: tau must be > 0 with a radius int(4 tau + 0.5) <= %d, got %g", who, VA_STIP_MAX_RADIUS, tau);
    const size_t vox = (size_t)n_frames * h * w, vpad = va_align_up(vox, 64);
    VA_CHECK_ARG(((size_t)tmp & 255) == 0, "%s: tmp must be 256-byte aligned", who);
    VA_CHECK_ARG(tmp_floats >= 2 * vox + 2048 && tmp_floats >= 2 * vpad + 2 * kTapStride, "%s: tmp of %zu floats, need %zu", who, tmp_floats,
                 std::max(2 * vox + 2048, 2 * vpad + 2 * kTapStride));
    float* A = (float*)tmp;
    float* B = A + vpad;
    float* taps = B + vpad;
    hipStream_t st = (hipStream_t)stream;
    VA_HIP(hipMemcpyAsync(taps, host, sizeof(host), hipMemcpyHostToDevice, st));
    VA_HIP(hipStreamSynchronize(st));
    return smooth3(src, src_is_u8, (float*)dst, A, B, taps, rs, taps + kTapStride, rt, n_frames, h, w, tu, st);
}

extern "C" int va_stip_gradient_products(va_ctx* ctx, const void* L, int n_frames, int w, int h, void* products, void* stream)
{
    const char* who = "va_stip_gradient_products";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_CHECK_ARG(L != nullptr && products != nullptr, "%s: NULL buffer", who);
    VA_USE_DEVICE(ctx);
    if (int rc = check_volume(who, n_frames, w, h, 1)) return rc;
    return launch_products((const float*)L, (float*)products, n_frames, h, w, (hipStream_t)stream);
}

extern "C" int va_stip_response(va_ctx* ctx, const void* products, int n_frames, int w, int h, float k, void* H, void* stream)
{
    const char* who = "va_stip_response";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_CHECK_ARG(products != nullptr && H != nullptr, "%s: NULL buffer", who);
    VA_USE_DEVICE(ctx);
    if (int rc = check_volume(who, n_frames, w, h, 1)) return rc;
    return launch_response((const float*)products, (float*)H, k, (size_t)n_frames * h * w, (hipStream_t)stream);
}

extern "C" int va_stip_maxima(va_ctx* ctx, const void* H, int n_frames, int w, int h, float min_response, int neighbours, int sigma_index,
                              int tau_index, void* points, void* response, int capacity, void* counts, void* scratch, void* stream)
{
    const char* who = "va_stip_maxima";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_CHECK_ARG(H != nullptr && points != nullptr && response != nullptr && counts != nullptr && scratch != nullptr, "%s: NULL buffer", who);
    VA_USE_DEVICE(ctx);
    if (int rc = check_volume(who, n_frames, w, h, 1)) return rc;
    VA_CHECK_ARG(neighbours == 6 || neighbours == 26, "%s: neighbours must be 6 or 26, got %d", who, neighbours);
    VA_CHECK_ARG(sigma_index >= 0 && sigma_index < VA_STIP_MAX_SIGMAS, "%s: sigma_index must be in [0,%d), got %d", who, VA_STIP_MAX_SIGMAS, sigma_index);
    VA_CHECK_ARG(tau_index >= 0 && tau_index < VA_STIP_MAX_TAUS, "%s: tau_index must be in [0,%d), got %d", who, VA_STIP_MAX_TAUS, tau_index);
    VA_CHECK_ARG(capacity >= 1, "%s: capacity must be >= 1, got %d", who, capacity);
    return launch_maxima((const float*)H, n_frames, h, w, min_response, neighbours, sigma_index, tau_index, (int*)points, (float*)response, capacity,
                         (int*)counts, (int*)scratch, (hipStream_t)stream);
}

extern "C" int va_stip_votes(va_ctx* ctx, const void* L, const void* flow, int n_frames, int w, int h, const va_stip_params* p, void* hog,
                             void* hof, void* stream)
{
    const char* who = "va_stip_votes";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_CHECK_ARG((hog != nullptr || hof != nullptr) && (hog == nullptr || L != nullptr) && (hof == nullptr || flow != nullptr), "%s: NULL buffer", who);
    VA_USE_DEVICE(ctx);
    Tune tu;
    if (int rc = check_params(who, p, &tu)) return rc;
    if (int rc = check_volume(who, n_frames, w, h, 2)) return rc;
    return launch_votes((const float*)L, (const float*)flow, n_frames, h, w, p->bins, (unsigned*)hog, (unsigned*)hof, (hipStream_t)stream);
}

extern "C" int va_stip_describe(va_ctx* ctx, const void* points, int n, const void* hog_integral, const void* hof_integral, int n_frames,
                                int w, int h, const va_stip_params* p, void* desc, void* stream)
{
    const char* who = "va_stip_describe";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_CHECK_ARG(points != nullptr && hog_integral != nullptr && hof_integral != nullptr && desc != nullptr, "%s: NULL buffer", who);
    VA_USE_DEVICE(ctx);
    Tune tu;
    if (int rc = check_params(who, p, &tu)) return rc;
    if (int rc = check_volume(who, n_frames, w, h, 1)) return rc;
    VA_CHECK_ARG(n >= 1, "%s: n must be >= 1, got %d", who, n);
    return launch_describe(p, (const int*)points, nullptr, n, n, (const unsigned*)hog_integral, (const unsigned*)hof_integral, n_frames, h, w,
                           (float*)desc, (hipStream_t)stream);
}
