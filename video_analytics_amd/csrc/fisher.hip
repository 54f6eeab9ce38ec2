// Fisher vectors on the device: PCA moments and projection, the statistics of a diagonal-covariance
// Gaussian mixture (the E-step of fitting it and the first half of encoding with it), its M-step and the Fisher vector
// epilogue -- the modelled project's Sheet02.py:568-617 between the trajectory descriptors and the linear SVM.
//
// Everything is float64 (float32 inputs are widened exactly).  The dense products run on v_mfma_f64_16x16x4_f64 (operand
// layout: v4d in va_feature_device.h).  Every sum has a fixed order that depends on the inputs and the parameters alone, and
// there are no atomics: two calls give the same bits.
#include "va_feature_device.h"

#include <cfloat>
#include <cmath>

namespace {

constexpr int kPcaMaxDim = 2048, kPcaMinChunkRows = 256;
constexpr int kGmmMaxDim = 512, kGmmMaxComp = 256, kGmmMaxSegments = 65536;
constexpr int kGmmMinChunk = 16, kGmmMaxChunk = 65536, kGmmMaxBatch = 65536;
constexpr double kFisherEpsilon = 1e-6;  // Sheet02.py:39

// ---- S77 PCA ----------------------------------------------------------------------------------------------------------

// Element (i, a) of [X, 1]: column d is the ones column that yields the column sums and the row count.
__device__ __forceinline__ double pca_elem(const float* __restrict__ x, size_t i, int d, int a)
{
    return a < d ? (double)x[i * d + a] : (a == d ? 1.0 : 0.0);
}

// part[chunk][a][b] = sum over the chunk's rows of Xh[i][a] Xh[i][b], Xh = [X, 1], i ascending four at a time, for the 64 x 64
// tiles on and above the diagonal.  Wave w holds rows a = 16w .. 16w+15 of the tile (A = Xh^T), all 64 columns b.
__global__ void __launch_bounds__(256) k_pca_xtx(const float* __restrict__ x, int n, int d, int chunk_rows, double* __restrict__ part)
{
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
    const int D = d + 1;
    const int a = ti * 64 + wave * 16 + r16;
    const long long i_beg = (long long)blockIdx.z * chunk_rows;
    const long long i_end = i_beg + chunk_rows < (long long)n ? i_beg + chunk_rows : (long long)n;
    v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (long long i0 = i_beg; i0 < i_end; i0 += 4) {
        const long long i = i0 + q;
        const bool ok = i < i_end;
        const size_t il = (size_t)(ok ? i : i_end - 1);
        const double av = ok ? pca_elem(x, il, d, a) : 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double bv = ok ? pca_elem(x, il, d, tj * 64 + 16 * t + r16) : 0.0;
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
        }
    }
    double* __restrict__ out = part + (size_t)blockIdx.z * D * D;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int ar = ti * 64 + wave * 16 + q + 4 * reg, bc = tj * 64 + 16 * t + r16;
            if (ar < D && bc < D) out[(size_t)ar * D + bc] = acc[t][reg];
        }
}

// sums = [count | column sums [d] | X^T X [d][d], upper triangle]: the chunks added in ascending order, stored or added.
__global__ void __launch_bounds__(256) k_pca_reduce(const double* __restrict__ part, int chunks, int d, int first, double* __restrict__ sums)
{
    const int D = d + 1;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)D * D) return;
    const int a = (int)(idx / D), b = (int)(idx % D);
    size_t at;
    if (a == d && b == d) at = 0;
    else if (b == d) at = 1 + (size_t)a;
    else if (a == d) return;
    else at = 1 + (size_t)d + (size_t)a * d + b;
    if (a > b) {  // below the diagonal: not computed
        if (first) sums[at] = 0.0;
        return;
    }
    double acc = part[idx];
    for (int ch = 1; ch < chunks; ++ch) acc = acc + part[(size_t)ch * D * D + idx];
    sums[at] = first ? acc : sums[at] + acc;
}

// out[i][j] = sum_c (x[i][c] - mean[c]) comp[j][c]: a workgroup computes 64 rows x 64 components, wave w rows 16w .. 16w+15;
// c is walked 16 at a time as in k_svm_fwd.
__global__ void __launch_bounds__(256) k_pca_transform(const float* __restrict__ x, int n, int d, const double* __restrict__ mean,
                                                       const double* __restrict__ comp, int m, float* __restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
    const long long rowbase = (long long)blockIdx.x * 64 + wave * 16;
    if (rowbase >= n) return;
    const int c0 = blockIdx.y * 64;
    const long long rl = rowbase + r16 < n ? rowbase + r16 : (long long)n - 1;
    const float* __restrict__ xr = x + (size_t)rl * d;
    const double* pr[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) pr[t] = comp + (size_t)min(c0 + 16 * t + r16, m - 1) * d;
    v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < d; k0 += 16) {
        const int kb = k0 + 4 * q;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = kb + s;
            const bool in = k < d;
            const int kl = in ? k : d - 1;
            const double a = in ? (double)xr[kl] - mean[kl] : 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double b = in ? pr[t][kl] : 0.0;
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const long long row = rowbase + q + 4 * reg;
            const int col = c0 + 16 * t + r16;
            if (row < n && col < m) out[(size_t)row * m + col] = (float)acc[t][reg];
        }
}

bool pca_sizes_ok(const char* who, int n, int d)
{
    if (n < 1 || d < 1 || d > kPcaMaxDim) {
        va_set_error("%s: need n >= 1 and 1 <= d <= %d (got n %d, d %d)", who, kPcaMaxDim, n, d);
        return false;
    }
    return true;
}

// at most `cap` chunks, where cap keeps cap * (d+1)^2 doubles within 1 GiB, and no chunk below 256 rows
int pca_chunk_rows(int n, int d)
{
    const long long D = d + 1;
    long long cap = ((long long)1 << 27) / (D * D);
    cap = cap < 8 ? 8 : (cap > 64 ? 64 : cap);
    long long rows = ((long long)n + cap - 1) / cap;
    rows = (rows + 3) / 4 * 4;
    return (int)(rows < kPcaMinChunkRows ? kPcaMinChunkRows : rows);
}

int pca_chunks(int n, int d)
{
    const long long cr = pca_chunk_rows(n, d);
    return (int)(((long long)n + cr - 1) / cr);
}

}  // namespace

extern "C" int va_pca_chunk_rows(int n, int d)
{
    if (!pca_sizes_ok("va_pca_chunk_rows", n, d)) return 0;
    return pca_chunk_rows(n, d);
}

extern "C" size_t va_pca_workspace_bytes(int n, int d)
{
    if (!pca_sizes_ok("va_pca_workspace_bytes", n, d)) return 0;
    return (size_t)pca_chunks(n, d) * (d + 1) * (d + 1) * sizeof(double);
}

extern "C" int va_pca_moments(va_ctx* ctx, const void* x, int n, int d, int first, void* sums, void* workspace, size_t workspace_bytes,
                              void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_pca_moments: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x && sums && workspace, "va_pca_moments: NULL pointer");
    VA_CHECK_ARG(first == 0 || first == 1, "va_pca_moments: first must be 0 or 1 (got %d)", first);
    if (!pca_sizes_ok("va_pca_moments", n, d)) return VA_ERR_INVALID;
    const size_t need = va_pca_workspace_bytes(n, d);
    if (workspace_bytes < need) {
        va_set_error("va_pca_moments: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return VA_ERR_WORKSPACE;
    }
    VA_CHECK_ARG(((size_t)workspace & 7) == 0, "va_pca_moments: workspace must be 8-byte aligned");
    const int D = d + 1, tiles = va_cdiv(D, 64), chunks = pca_chunks(n, d);
    hipStream_t st = (hipStream_t)stream;
    k_pca_xtx<<<dim3(tiles, tiles, chunks), 256, 0, st>>>((const float*)x, n, d, pca_chunk_rows(n, d), (double*)workspace);
    k_pca_reduce<<<(unsigned)(((size_t)D * D + 255) / 256), 256, 0, st>>>((const double*)workspace, chunks, d, first, (double*)sums);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_pca_transform(va_ctx* ctx, const void* x, int n, int d, const void* mean, const void* components, int m, void* out,
                                void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_pca_transform: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x && mean && components && out, "va_pca_transform: NULL pointer");
    if (!pca_sizes_ok("va_pca_transform", n, d)) return VA_ERR_INVALID;
    VA_CHECK_ARG(m >= 1 && m <= d, "va_pca_transform: need 1 <= m <= d (got m %d, d %d)", m, d);
    k_pca_transform<<<dim3((unsigned)(((long long)n + 63) / 64), va_cdiv(m, 64)), 256, 0, (hipStream_t)stream>>>(
        (const float*)x, n, d, (const double*)mean, (const double*)components, m, (float*)out);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

// ---- S78-S80 mixture statistics -----------------------------------------------------------------------------------------

namespace {

// The expanded parameters, one workgroup per component row j < kpad: Bm[j][2c] = -1/(2 var_jc), Bm[j][2c+1] = mu_jc / var_jc
// (columns up to DD = 2d rounded up to 16 are 0; rows j >= k are 0), ck[j] = log w_j - 1/2 sum_c log var_jc -
// 1/2 sum_c mu_jc^2 / var_jc - d/2 log 2 pi, both sums over c ascending.
__global__ void __launch_bounds__(256) k_gmm_prep(const double* __restrict__ w, const double* __restrict__ mu, const double* __restrict__ var,
                                                  int k, int d, int DD, double* __restrict__ Bm, double* __restrict__ ck)
{
    const int j = blockIdx.x;
    for (int kk = threadIdx.x; kk < DD; kk += 256) {
        const int c = kk >> 1;
        double v = 0.0;
        if (j < k && c < d) {
            const double s2 = var[(size_t)j * d + c];
            v = (kk & 1) ? mu[(size_t)j * d + c] / s2 : -0.5 / s2;
        }
        Bm[(size_t)j * DD + kk] = v;
    }
    if (threadIdx.x == 0) {
        double c0 = 0.0;
        if (j < k) {
            double ld = 0.0, mm = 0.0;
            for (int c = 0; c < d; ++c) {
                const double s2 = var[(size_t)j * d + c], m = mu[(size_t)j * d + c];
                ld = ld + log(s2);
                mm = mm + m * m / s2;
            }
            c0 = ((log(w[j]) - 0.5 * ld) - 0.5 * mm) - 0.5 * (double)d * 1.8378770664093453;  // log 2 pi
        }
        ck[j] = c0;
    }
}

// The responsibilities of `rows` rows starting at row r0 of x: a wave owns 16 rows and all 16 NT >= k components, 4 NT
// accumulators per lane.  The interleaved operand [x_c^2, x_c] is walked 16 values (8 columns) at a time; lane group q feeds
// columns 2q, 2q+1 of the step.  Then, for each of the lane's four rows: log p = acc + ck, the maximum and the sum of
// exp(log p - max) over the lane's components in ascending order followed by an xor butterfly over the 16 lanes of the row,
// lse = max + log(sum), gamma = exp(log p - lse); HARD: the arg-max, the lowest component on ties, and its one-hot.
// G[row][ldg]: columns below ncols are stored (components >= k as 0).
template <int NT>
__global__ void __launch_bounds__(256) k_gmm_resp(const float* __restrict__ x, long long r0, int rows, int d, int DD, int k,
                                                  const double* __restrict__ Bm, const double* __restrict__ ck, int hard,
                                                  double* __restrict__ G, int ldg, int ncols, double* __restrict__ rowlse)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
    const int rowbase = blockIdx.x * 64 + wave * 16;
    if (rowbase >= rows) return;
    const float* __restrict__ xr = x + (size_t)(r0 + min(rowbase + r16, rows - 1)) * d;
    v4d acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < DD; k0 += 16) {
        const int kb = k0 + 4 * q, c0 = kb >> 1;
        const double x0 = c0 < d ? (double)xr[c0] : 0.0, x1 = c0 + 1 < d ? (double)xr[c0 + 1] : 0.0;
        const double a0 = x0 * x0, a2 = x1 * x1;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double* __restrict__ br = Bm + (size_t)(16 * t + r16) * DD + kb;
            const double b0 = br[0], b1 = br[1], b2 = br[2], b3 = br[3];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, b1, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, b3, acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int row = rowbase + q + 4 * reg;
        double lp[NT];
        double m = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = 16 * t + r16;
            lp[t] = col < k ? acc[t][reg] + ck[col] : -INFINITY;
            if (lp[t] > m) m = lp[t], bi = col;  // ascending components: the lowest wins a tie
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const double om = __shfl_xor(m, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (om > m || (om == m && oi < bi)) m = om, bi = oi;
        }
        double s = 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) s = s + exp(lp[t] - m);
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) s = s + __shfl_xor(s, off, 64);
        const double lse = m + log(s);
        if (row < rows) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int col = 16 * t + r16;
                const double g = hard ? (col == bi ? 1.0 : 0.0) : exp(lp[t] - lse);
                if (col < ncols) G[(size_t)row * ldg + col] = g;
            }
            if (r16 == 0) rowlse[row] = lse;
        }
    }
}

// The chunk sums of one batch.  Workgroup (chunk, component block, column block): the chunk's rows [start, end) are cut at
// the segment boundaries inside it; each piece's sum over its rows, four at a time ascending, of gamma[i][j] xx[i][col],
// xx = [1 | x | x^2] (1 + 2d columns), goes to part[slot][j][col] with slot = chunk + segment, which grows with the rows,
// and the piece's sum of the rows' logsumexp to pll[slot].
// A = gamma^T (16 KT components), B = xx: wave w the columns 16w .. 16w+15 of the block of 64.
template <int KT>
__global__ void __launch_bounds__(256) k_gmm_acc(const float* __restrict__ x, long long r0, int rows, int d, int k, int kpad, int chunk_rows,
                                                 const long long* __restrict__ seg, int n_segments, const double* __restrict__ G,
                                                 const double* __restrict__ rowlse, double* __restrict__ part, int* __restrict__ pseg,
                                                 double* __restrict__ pll)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
    const int C = 1 + 2 * d;
    if (blockIdx.z * 64 + wave * 16 >= C) return;
    const int col = blockIdx.z * 64 + wave * 16 + r16;
    const int xc = col == 0 ? 0 : (col <= d ? col - 1 : min(col - d - 1, d - 1));
    const bool one = col == 0, sq = col > d, live = col < C;
    const int j0 = blockIdx.y * 16 * KT;
    const long long last = r0 + rows;
    long long start = r0 + (long long)blockIdx.x * chunk_rows;
    const long long end = start + chunk_rows < last ? start + chunk_rows : last;
    int lo = 0, hi = n_segments - 1;  // the first segment that ends after `start`
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid + 1] > start) hi = mid;
        else lo = mid + 1;
    }
    int s = lo;
    while (start < end && s < n_segments) {
        const long long pe = seg[s + 1] < end ? seg[s + 1] : end;
        v4d acc[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
        long long i0 = start;
        for (; i0 + 16 <= pe; i0 += 16) {  // four steps' loads first, then their products in the same order as the tail's
            double bb[4], aa[4][KT];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t il = (size_t)(i0 + 4 * u + q);
                double b = 0.0;
                if (live) {
                    b = one ? 1.0 : (double)x[il * d + xc];
                    if (sq) b = b * b;
                }
                bb[u] = b;
                const double* __restrict__ gr = G + (size_t)(il - r0) * kpad + j0 + r16;
#pragma unroll
                for (int t = 0; t < KT; ++t) aa[u][t] = gr[16 * t];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int t = 0; t < KT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[u][t], bb[u], acc[t], 0, 0, 0);
        }
        for (; i0 < pe; i0 += 4) {
            const long long i = i0 + q;
            const bool ok = i < pe;
            const size_t il = (size_t)(ok ? i : pe - 1);
            double b = 0.0;
            if (ok && live) {
                b = one ? 1.0 : (double)x[il * d + xc];
                if (sq) b = b * b;
            }
            const double* __restrict__ gr = G + (size_t)(il - r0) * kpad + j0 + r16;
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                const double a = ok ? gr[16 * t] : 0.0;
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
            }
        }
        const int slot = blockIdx.x + s;
        if (live) {
            double* __restrict__ out = part + (size_t)slot * k * C;
#pragma unroll
            for (int t = 0; t < KT; ++t)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int j = j0 + 16 * t + q + 4 * reg;
                    if (j < k) out[(size_t)j * C + col] = acc[t][reg];
                }
        }
        if (blockIdx.y == 0 && blockIdx.z == 0 && wave == 0) {  // the piece's log-likelihood: lane l rows l, l + 64, ..., then the lanes
            double v = 0.0;
            for (long long i = start + lane; i < pe; i += 64) v = v + rowlse[i - r0];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
            if (lane == 0) {
                pseg[slot] = s;
                pll[slot] = v;
            }
        }
        start = pe;
        ++s;
        while (s < n_segments && seg[s + 1] <= start) ++s;
    }
}

// A batch's chunk sums join the segments' statistics in ascending slot (= row) order; the last workgroup's first thread does
// the same for the pieces' log-likelihoods.
__global__ void __launch_bounds__(256) k_gmm_reduce(const double* __restrict__ part, const int* __restrict__ pseg,
                                                    const double* __restrict__ pll, int slots, int kc, double* __restrict__ stats,
                                                    double* __restrict__ loglik)
{
    if (blockIdx.x == gridDim.x - 1) {
        if (threadIdx.x != 0) return;
        for (int slot = 0; slot < slots; ++slot) {
            const int s = pseg[slot];
            if (s >= 0) loglik[s] = loglik[s] + pll[slot];
        }
        return;
    }
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= kc) return;
    int cur = -1;
    double acc = 0.0;
    for (int slot = 0; slot < slots; ++slot) {
        const int s = pseg[slot];
        if (s < 0) continue;
        if (s != cur) {
            if (cur >= 0) stats[(size_t)cur * kc + idx] = acc;
            cur = s;
            acc = stats[(size_t)s * kc + idx];
        }
        acc = acc + part[(size_t)slot * kc + idx];
    }
    if (cur >= 0) stats[(size_t)cur * kc + idx] = acc;
}

struct GmmPlan {
    int d, k, nt, kpad, DD, C, chunk_rows, batch_rows, chunks_per_batch, slots, n_segments;
    double *Bm, *ck, *G, *rowlse, *part;
    double* pll;
    int* pseg;
    size_t bytes;
};

// The argument checks every mixture entry point shares, and the workspace cut from `base` (NULL: the size alone)
int gmm_plan(const char* who, int n, int d, int k, int n_segments, const va_gmm_params* p, void* base, GmmPlan* out)
{
    va_gmm_params def;
    va_gmm_default_params(&def);
    if (p == nullptr) p = &def;
    VA_CHECK_ARG(p->struct_bytes >= (int)sizeof(va_gmm_params), "%s: struct_bytes %d is smaller than sizeof(va_gmm_params) = %d", who,
                 p->struct_bytes, (int)sizeof(va_gmm_params));
    VA_CHECK_ARG(n >= 1, "%s: n out of range: need n >= 1 (got %d)", who, n);
    VA_CHECK_ARG(d >= 1 && d <= kGmmMaxDim, "%s: d out of range: need 1 <= d <= %d (got %d)", who, kGmmMaxDim, d);
    VA_CHECK_ARG(k >= 1 && k <= kGmmMaxComp, "%s: k out of range: need 1 <= k <= %d (got %d)", who, kGmmMaxComp, k);
    VA_CHECK_ARG(n_segments >= 1 && n_segments <= kGmmMaxSegments, "%s: n_segments out of range: need 1 <= n_segments <= %d (got %d)", who,
                 kGmmMaxSegments, n_segments);
    VA_CHECK_ARG(p->chunk_rows >= kGmmMinChunk && p->chunk_rows <= kGmmMaxChunk,
                 "%s: chunk_rows out of range: need %d <= chunk_rows <= %d (got %d)", who, kGmmMinChunk, kGmmMaxChunk, p->chunk_rows);
    VA_CHECK_ARG(p->batch_rows >= p->chunk_rows && p->batch_rows <= kGmmMaxBatch,
                 "%s: batch_rows out of range: need chunk_rows <= batch_rows <= %d (got %d, chunk_rows %d)", who, kGmmMaxBatch, p->batch_rows,
                 p->chunk_rows);
    GmmPlan g;
    g.d = d, g.k = k, g.n_segments = n_segments;
    g.nt = k <= 16 ? 1 : (k <= 64 ? 4 : 16);
    g.kpad = 16 * g.nt;
    g.DD = (2 * d + 15) / 16 * 16;
    g.C = 1 + 2 * d;
    g.chunk_rows = p->chunk_rows;
    g.chunks_per_batch = p->batch_rows / p->chunk_rows;
    g.batch_rows = g.chunks_per_batch * g.chunk_rows;
    g.slots = g.chunks_per_batch + n_segments;
    va_carver ws{base};
    g.Bm = ws.take<double>((size_t)g.kpad * g.DD);
    g.ck = ws.take<double>((size_t)g.kpad);
    g.G = ws.take<double>((size_t)g.batch_rows * g.kpad);
    g.rowlse = ws.take<double>((size_t)g.batch_rows);
    g.part = ws.take<double>((size_t)g.slots * k * g.C);
    g.pll = ws.take<double>((size_t)g.slots);
    g.pseg = ws.take<int>((size_t)g.slots);
    g.bytes = ws.off;
    *out = g;
    return VA_OK;
}

// the workspace's alignment, the plan and the workspace's size, in that order
int gmm_ready(const char* who, int n, int d, int k, int n_segments, const va_gmm_params* p, void* workspace, size_t workspace_bytes,
              GmmPlan* g)
{
    VA_CHECK_ARG(((size_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    if (int rc = gmm_plan(who, n, d, k, n_segments, p, workspace, g)) return rc;
    if (workspace_bytes < g->bytes) {
        va_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, g->bytes);
        return VA_ERR_WORKSPACE;
    }
    return VA_OK;
}

void gmm_launch_resp(const GmmPlan& g, const float* x, long long r0, int rows, int hard, double* G, int ldg, int ncols, double* rowlse,
                     hipStream_t st)
{
    const dim3 grid(va_cdiv(rows, 64));
    if (g.nt == 1) k_gmm_resp<1><<<grid, 256, 0, st>>>(x, r0, rows, g.d, g.DD, g.k, g.Bm, g.ck, hard, G, ldg, ncols, rowlse);
    else if (g.nt == 4) k_gmm_resp<4><<<grid, 256, 0, st>>>(x, r0, rows, g.d, g.DD, g.k, g.Bm, g.ck, hard, G, ldg, ncols, rowlse);
    else k_gmm_resp<16><<<grid, 256, 0, st>>>(x, r0, rows, g.d, g.DD, g.k, g.Bm, g.ck, hard, G, ldg, ncols, rowlse);
}

}  // namespace

extern "C" void va_gmm_default_params(va_gmm_params* p)
{
    if (p == nullptr) return;
    *p = va_gmm_params{};
    p->struct_bytes = (int)sizeof(va_gmm_params);
    p->chunk_rows = 1024;
    p->batch_rows = 65536;
}

extern "C" size_t va_gmm_workspace_bytes(int n, int d, int k, int n_segments, const va_gmm_params* p)
{
    GmmPlan g;
    if (gmm_plan("va_gmm_workspace_bytes", n, d, k, n_segments, p, nullptr, &g) != VA_OK) return 0;
    return g.bytes;
}

extern "C" int va_gmm_stats(va_ctx* ctx, const void* x, int n, int d, const void* segments, int n_segments, const void* weights,
                            const void* means, const void* variances, int k, int mode, const va_gmm_params* p, void* stats, void* loglik,
                            void* workspace, size_t workspace_bytes, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_gmm_stats: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x && segments && weights && means && variances && stats && loglik && workspace, "va_gmm_stats: NULL pointer");
    VA_CHECK_ARG(mode == VA_GMM_SOFT || mode == VA_GMM_HARD, "va_gmm_stats: mode must be VA_GMM_SOFT or VA_GMM_HARD (got %d)", mode);
    GmmPlan g;
    if (int rc = gmm_ready("va_gmm_stats", n, d, k, n_segments, p, workspace, workspace_bytes, &g)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int kc = k * g.C;
    VA_HIP(hipMemsetAsync(stats, 0, (size_t)n_segments * kc * sizeof(double), st));
    VA_HIP(hipMemsetAsync(loglik, 0, (size_t)n_segments * sizeof(double), st));
    k_gmm_prep<<<g.kpad, 256, 0, st>>>((const double*)weights, (const double*)means, (const double*)variances, k, d, g.DD, g.Bm, g.ck);
    const int kt = g.nt == 1 ? 1 : 4;
    for (long long r0 = 0; r0 < n; r0 += g.batch_rows) {
        const int rows = (int)((long long)n - r0 < g.batch_rows ? (long long)n - r0 : g.batch_rows);
        const int chunks = va_cdiv(rows, g.chunk_rows);
        VA_HIP(hipMemsetAsync(g.pseg, 0xff, (size_t)g.slots * sizeof(int), st));
        gmm_launch_resp(g, (const float*)x, r0, rows, mode == VA_GMM_HARD, g.G, g.kpad, g.kpad, g.rowlse, st);
        const dim3 grid(chunks, g.kpad / (16 * kt), va_cdiv(g.C, 64));
        if (kt == 1)
            k_gmm_acc<1><<<grid, 256, 0, st>>>((const float*)x, r0, rows, d, k, g.kpad, g.chunk_rows, (const long long*)segments, n_segments,
                                               g.G, g.rowlse, g.part, g.pseg, g.pll);
        else
            k_gmm_acc<4><<<grid, 256, 0, st>>>((const float*)x, r0, rows, d, k, g.kpad, g.chunk_rows, (const long long*)segments, n_segments,
                                               g.G, g.rowlse, g.part, g.pseg, g.pll);
        k_gmm_reduce<<<va_cdiv(kc, 256) + 1, 256, 0, st>>>(g.part, g.pseg, g.pll, g.slots, kc, (double*)stats, (double*)loglik);
        VA_LAUNCH_CHECK();
    }
    return VA_OK;
}

extern "C" int va_gmm_posteriors(va_ctx* ctx, const void* x, int n, int d, const void* weights, const void* means, const void* variances,
                                 int k, int mode, void* gamma, void* lse, void* workspace, size_t workspace_bytes, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_gmm_posteriors: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x && weights && means && variances && gamma && lse && workspace, "va_gmm_posteriors: NULL pointer");
    VA_CHECK_ARG(mode == VA_GMM_SOFT || mode == VA_GMM_HARD, "va_gmm_posteriors: mode must be VA_GMM_SOFT or VA_GMM_HARD (got %d)", mode);
    VA_CHECK_ARG(n <= kGmmMaxBatch, "va_gmm_posteriors: n out of range: need n <= %d (got %d)", kGmmMaxBatch, n);
    GmmPlan g;
    if (int rc = gmm_ready("va_gmm_posteriors", n, d, k, 1, nullptr, workspace, workspace_bytes, &g)) return rc;
    hipStream_t st = (hipStream_t)stream;
    k_gmm_prep<<<g.kpad, 256, 0, st>>>((const double*)weights, (const double*)means, (const double*)variances, k, d, g.DD, g.Bm, g.ck);
    gmm_launch_resp(g, (const float*)x, 0, n, mode == VA_GMM_HARD, (double*)gamma, k, k, (double*)lse, st);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

// ---- S81 M-step, S82 Fisher vector ---------------------------------------------------------------------------------------

namespace {

__global__ void __launch_bounds__(256) k_gmm_mstep(const double* __restrict__ stats, int n_segments, int k, int d, double reg,
                                                   double* __restrict__ w, double* __restrict__ mu, double* __restrict__ var)
{
    __shared__ double nk[kGmmMaxComp];
    __shared__ double total;
    const int C = 1 + 2 * d;
    const size_t stride = (size_t)k * C;
    for (int j = threadIdx.x; j < k; j += 256) nk[j] = va_strided_sum(stats, n_segments, stride, (size_t)j * C) + 10.0 * DBL_EPSILON;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int j = 0; j < k; ++j) t = t + nk[j];
        total = t;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += 256) w[j] = nk[j] / total;
    for (int e = threadIdx.x; e < k * d; e += 256) {
        const int j = e / d, c = e % d;
        const double s1 = va_strided_sum(stats, n_segments, stride, (size_t)j * C + 1 + c);
        const double s2 = va_strided_sum(stats, n_segments, stride, (size_t)j * C + 1 + d + c);
        const double m = s1 / nk[j];
        mu[e] = m;
        var[e] = ((s2 / nk[j] - 2.0 * (m * s1 / nk[j])) + m * m) + reg;
    }
}

// Entry e of a segment's Fisher vector before the normalisation.
__device__ __forceinline__ double fisher_value(const double* __restrict__ st, int e, int k, int d, double T, const double* __restrict__ w,
                                               const double* __restrict__ mu, const double* __restrict__ var, double power)
{
    const int C = 1 + 2 * d;
    double v;
    if (e < k) {
        v = (st[(size_t)e * C] - T * w[e]) / sqrt(w[e]);
    } else {
        const int f = (e - k) % (k * d), j = f / d, c = f % d;
        const double s0 = st[(size_t)j * C], s1 = st[(size_t)j * C + 1 + c], s2 = st[(size_t)j * C + 1 + d + c];
        const double m = mu[f], s = var[f];
        if (e < k + k * d) v = (s1 - m * s0) / (sqrt(s) * sqrt(w[j]));
        else v = (((s2 - 2.0 * m * s1) + m * m * s0) / s - s0) / sqrt(2.0 * w[j]);
    }
    v = v / T;
    if (power > 0.0) v = v < 0.0 ? -pow(-v, power) : pow(v, power);
    return v;
}

__global__ void __launch_bounds__(256) k_fisher_encode(const double* __restrict__ stats, const long long* __restrict__ counts, int k, int d,
                                                       const double* __restrict__ w, const double* __restrict__ mu,
                                                       const double* __restrict__ var, double power, float* __restrict__ out)
{
    __shared__ double red[4];
    const int L = k + 2 * k * d;
    const double* __restrict__ st = stats + (size_t)blockIdx.x * k * (1 + 2 * d);
    float* __restrict__ o = out + (size_t)blockIdx.x * L;
    const long long T = counts[blockIdx.x];
    if (T <= 0) {
        for (int e = threadIdx.x; e < L; e += 256) o[e] = 0.0f;
        return;
    }
    double ss = 0.0;
    for (int e = threadIdx.x; e < L; e += 256) {
        const double v = fisher_value(st, e, k, d, (double)T, w, mu, var, power);
        ss = ss + v * v;
    }
    const double norm = sqrt(va_wg_sum256(ss, red));
    for (int e = threadIdx.x; e < L; e += 256) {
        const double v = fisher_value(st, e, k, d, (double)T, w, mu, var, power);
        o[e] = (float)(norm < kFisherEpsilon ? v : v / norm);
    }
}

bool kd_ok(const char* who, int n_segments, int k, int d)
{
    if (n_segments < 1 || n_segments > kGmmMaxSegments || k < 1 || k > kGmmMaxComp || d < 1 || d > kGmmMaxDim) {
        va_set_error("%s: need 1 <= n_segments <= %d, 1 <= k <= %d, 1 <= d <= %d (got %d, %d, %d)", who, kGmmMaxSegments, kGmmMaxComp,
                     kGmmMaxDim, n_segments, k, d);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int va_gmm_mstep(va_ctx* ctx, const void* stats, int n_segments, int k, int d, double reg_covar, void* weights, void* means,
                            void* variances, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_gmm_mstep: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(stats && weights && means && variances, "va_gmm_mstep: NULL pointer");
    if (!kd_ok("va_gmm_mstep", n_segments, k, d)) return VA_ERR_INVALID;
    VA_CHECK_ARG(reg_covar - reg_covar == 0.0 && reg_covar >= 0.0, "va_gmm_mstep: reg_covar must be finite and >= 0 (got %g)", reg_covar);
    k_gmm_mstep<<<1, 256, 0, (hipStream_t)stream>>>((const double*)stats, n_segments, k, d, reg_covar, (double*)weights, (double*)means,
                                                    (double*)variances);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_fisher_encode(va_ctx* ctx, const void* stats, const void* counts, int n_segments, int k, int d, const void* weights,
                                const void* means, const void* variances, double power, void* out, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_fisher_encode: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(stats && counts && weights && means && variances && out, "va_fisher_encode: NULL pointer");
    if (!kd_ok("va_fisher_encode", n_segments, k, d)) return VA_ERR_INVALID;
    VA_CHECK_ARG(power >= 0.0 && power <= 1.0, "va_fisher_encode: power must be in [0, 1] (got %g)", power);
    k_fisher_encode<<<n_segments, 256, 0, (hipStream_t)stream>>>((const double*)stats, (const long long*)counts, k, d, (const double*)weights,
                                                                 (const double*)means, (const double*)variances, power, (float*)out);
    VA_LAUNCH_CHECK();
    return VA_OK;
}
