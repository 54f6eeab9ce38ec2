// Bag of words on the device: k-means++ seeding, the nearest-centre assignment, the centre update as a
// segmented sum, and per-video histograms of the labels -- the modelled project's Sheet01.py:259-277 between the HOG/HOF
// descriptors and the linear SVM.
//
// Everything is float64 (float32 inputs are widened exactly).  The products of the assignment run on v_mfma_f64_16x16x4_f64
// (operand layout: v4d in va_feature_device.h).  Nothing of size n x K exists.  Every floating-point sum has a fixed order that
// depends on the inputs and the parameters alone; the only atomics are integer ones (counts, the lowest and the highest row
// index), whose results do not depend on their order: two calls give the same bits.
#include "va_feature_device.h"

#include <climits>
#include <cmath>

namespace {

constexpr int kKmMaxDim = 512, kKmMaxK = 4096, kKmMaxSegments = 65536;
constexpr int kKmMinChunk = 64, kKmMaxChunk = 1 << 20, kKmMaxChunks = 65536;
constexpr int kTileK = 64;             // centres per LDS tile
constexpr int kTileD = 64;             // columns per LDS tile
constexpr int kTileLd = kTileD + 1;    // row stride in doubles: 130 dwords = 2 mod 64 banks, the 16 centres of a read never collide
constexpr int kRowBlocks = 2;          // 16-row blocks per wave
constexpr int kWgRows = 4 * 16 * kRowBlocks;
constexpr int kSumBlock = 256;         // rows per block sum (inertia, seeding)

// sum_c (x[i][c] - ctr[c])^2 for the 256 rows of a workgroup, row r0 + thread: columns ascending, one rounding per operation.
// The rows' floats pass through LDS 32 columns at a time (loaded along the rows, read down the thread's own row; the stride
// of 33 keeps both free of bank conflicts), so the global reads are whole 128-byte runs.  ctr: the thread's centre row.
constexpr int kDirectCols = 32, kDirectLd = kDirectCols + 1;
template <typename T>
__device__ __forceinline__ double direct_d2(const float* __restrict__ x, long long r0, int n, int d, const T* __restrict__ ctr,
                                            float* __restrict__ xs)
{
    const int lr = threadIdx.x >> 5, lc = threadIdx.x & 31;
    double acc = 0.0;
    for (int c0 = 0; c0 < d; c0 += kDirectCols) {
        __syncthreads();
#pragma unroll 8
        for (int r = lr; r < 256; r += 8) {
            const long long row = r0 + r;
            xs[r * kDirectLd + lc] = (row < n && c0 + lc < d) ? x[(size_t)row * d + c0 + lc] : 0.0f;
        }
        __syncthreads();
        const int cn = d - c0 < kDirectCols ? d - c0 : kDirectCols;
        for (int c = 0; c < cn; ++c) {
            const double t = (double)xs[threadIdx.x * kDirectLd + c] - (double)ctr[c0 + c];
            acc = acc + t * t;
        }
    }
    return acc;
}

// ---- S91 assignment ------------------------------------------------------------------------------------------------------

// hn[j] = 1/2 sum_c centres[j][c]^2, columns ascending
__global__ void __launch_bounds__(256) k_km_halfnorm(const double* __restrict__ centres, int K, int d, double* __restrict__ hn)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K) return;
    const double* __restrict__ c = centres + (size_t)j * d;
    double acc = 0.0;
    for (int a = 0; a < d; ++a) acc = acc + c[a] * c[a];
    hn[j] = 0.5 * acc;
}

// label[i] = the lowest j that attains min_j hn[j] - x_i . c_j.  A workgroup owns 128 rows, a wave two blocks of 16.  The
// centres are walked in tiles of 64 and the columns in tiles of 64; each [64 centres][64 columns] tile is staged in LDS once
// per workgroup (the next one waits in registers meanwhile) and read by all eight row blocks.  Within a column tile lane
// group q feeds columns 16q + s at step s = 0 .. 15, so a lane's sixteen values of x are contiguous.  After the last column
// tile of a centre tile each lane folds its four centres, ascending, into the running (min, index) of its eight rows with
// "strictly smaller"; after the last centre tile an xor butterfly over the 16 lanes of a row merges with "strictly smaller,
// or equal and lower index".  Two waves per SIMD: without the bound the compiler takes 340 registers and the pass is 17 % slower.
__global__ void __launch_bounds__(256, 2) k_km_assign(const float* __restrict__ x, int n, int d, const double* __restrict__ centres, int K,
                                                   const double* __restrict__ hn, int* __restrict__ labels)
{
    __shared__ double cs[kTileK * kTileLd];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
    const long long rowbase = (long long)blockIdx.x * kWgRows + wave * 16 * kRowBlocks;
    const float* xr[kRowBlocks];
#pragma unroll
    for (int rb = 0; rb < kRowBlocks; ++rb) {
        const long long r = rowbase + 16 * rb + r16;
        xr[rb] = x + (size_t)(r < n ? r : (long long)n - 1) * d;
    }
    double best[kRowBlocks][4];
    int bidx[kRowBlocks][4];
#pragma unroll
    for (int rb = 0; rb < kRowBlocks; ++rb)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) best[rb][reg] = INFINITY, bidx[rb][reg] = INT_MAX;
    const int nd = (d + kTileD - 1) / kTileD, steps = ((K + kTileK - 1) / kTileK) * nd;
    const int lj = threadIdx.x >> 6, lc = threadIdx.x & 63;  // the tile elements this thread stages: centres lj + 4u, column lc
    double pre[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int j = lj + 4 * u, c = lc;
        pre[u] = (j < K && c < d) ? centres[(size_t)j * d + c] : 0.0;
    }
    v4d acc[kRowBlocks][4];
    for (int step = 0; step < steps; ++step) {
        const int jt = step / nd, dc = step - jt * nd;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 16; ++u) cs[(lj + 4 * u) * kTileLd + lc] = pre[u];
        __syncthreads();
        if (step + 1 < steps) {
            const int jn = (step + 1) / nd, dn = (step + 1) - jn * nd;
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int j = jn * kTileK + lj + 4 * u, c = dn * kTileD + lc;
                pre[u] = (j < K && c < d) ? centres[(size_t)j * d + c] : 0.0;
            }
        }
        if (dc == 0) {
#pragma unroll
            for (int rb = 0; rb < kRowBlocks; ++rb)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[rb][t] = (v4d){0.0, 0.0, 0.0, 0.0};
        }
        const int cb = dc * kTileD + 16 * q;
        float a[kRowBlocks][16];
#pragma unroll
        for (int rb = 0; rb < kRowBlocks; ++rb)
#pragma unroll
            for (int s = 0; s < 16; ++s) a[rb][s] = cb + s < d ? xr[rb][cb + s] : 0.0f;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            double b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) b[t] = cs[(16 * t + r16) * kTileLd + 16 * q + s];
#pragma unroll
            for (int rb = 0; rb < kRowBlocks; ++rb)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[rb][t] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[rb][s], b[t], acc[rb][t], 0, 0, 0);
        }
        if (dc == nd - 1) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int col = jt * kTileK + 16 * t + r16;
                if (col < K) {
                    const double h = hn[col];
#pragma unroll
                    for (int rb = 0; rb < kRowBlocks; ++rb)
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            const double s = h - acc[rb][t][reg];
                            if (s < best[rb][reg]) best[rb][reg] = s, bidx[rb][reg] = col;  // ascending centres: the lowest wins a tie
                        }
                }
            }
        }
    }
#pragma unroll
    for (int rb = 0; rb < kRowBlocks; ++rb)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            double m = best[rb][reg];
            int bi = bidx[rb][reg];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                const double om = __shfl_xor(m, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (om < m || (om == m && oi < bi)) m = om, bi = oi;
            }
            const long long row = rowbase + 16 * rb + q + 4 * reg;
            if (r16 == 0 && row < n) labels[row] = bi < K ? bi : 0;  // a row of NaNs compares with nothing: centre 0
        }
}

// d2[i] = sum_c (x[i][c] - centres[label_i][c])^2 (stored when d2 is given), the number of rows whose label differs from
// prev's (every row when prev is NULL), and part[block] = the block's sum of d2 (va_wg_sum256) for the inertia.
__global__ void __launch_bounds__(256) k_km_d2(const float* __restrict__ x, int n, int d, const double* __restrict__ centres, int K,
                                               const int* __restrict__ labels, const int* __restrict__ prev, double* __restrict__ d2,
                                               double* __restrict__ part, unsigned long long* __restrict__ changed)
{
    __shared__ double red[4];
    __shared__ float xs[256 * kDirectLd];
    const long long r0 = (long long)blockIdx.x * 256, i = r0 + threadIdx.x;
    int j = i < n ? labels[i] : 0;
    j = j < 0 ? 0 : (j < K ? j : K - 1);
    double v = direct_d2(x, r0, n, d, centres + (size_t)j * d, xs);
    bool moved = false;
    if (i < n) {
        if (d2) d2[i] = v;
        moved = prev == nullptr || prev[i] != j;
    } else {
        v = 0.0;
    }
    const unsigned long long mv = __ballot(moved);
    if ((threadIdx.x & 63) == 0 && mv) atomicAdd(changed, (unsigned long long)__popcll(mv));
    const double s = va_wg_sum256(v, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// out[0] = the sum of part[0 .. count): thread t adds t, t + 256, ... in ascending order, then va_wg_sum256
__global__ void __launch_bounds__(256) k_km_sum_parts(const double* __restrict__ part, long long count, double* __restrict__ out)
{
    __shared__ double red[4];
    double v = 0.0;
    for (long long b = threadIdx.x; b < count; b += 256) v = v + part[b];
    const double s = va_wg_sum256(v, red);
    if (threadIdx.x == 0) out[0] = s;
}

// ---- S92 update: a stable counting sort of the rows by label, then one segmented sum per cluster ---------------------------

// hist[chunk][j] = the rows of the chunk with label j (labels outside 0 .. K-1 are counted nowhere)
__global__ void __launch_bounds__(256) k_km_count(const int* __restrict__ labels, int n, int K, int chunk_rows, int* __restrict__ hist)
{
    __shared__ int h[kKmMaxK];
    for (int j = threadIdx.x; j < K; j += 256) h[j] = 0;
    __syncthreads();
    const long long beg = (long long)blockIdx.x * chunk_rows;
    const long long end = beg + chunk_rows < (long long)n ? beg + chunk_rows : (long long)n;
    for (long long i = beg + threadIdx.x; i < end; i += 256) {
        const int l = labels[i];
        if (l >= 0 && l < K) atomicAdd(&h[l], 1);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < K; j += 256) hist[(size_t)blockIdx.x * K + j] = h[j];
}

// hist[chunk][j] becomes the rows of label j in the chunks before it; counts[j] = all of them
__global__ void __launch_bounds__(256) k_km_scan_chunks(int* __restrict__ hist, int chunks, int K, long long* __restrict__ counts)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K) return;
    int run = 0;
    for (int c = 0; c < chunks; ++c) {
        const int t = hist[(size_t)c * K + j];
        hist[(size_t)c * K + j] = run;
        run += t;
    }
    counts[j] = run;
}

// start[j] = the rows of the labels below j (start[K]: all sorted rows); one workgroup, 16 consecutive labels per thread
__global__ void __launch_bounds__(256) k_km_scan_clusters(const long long* __restrict__ counts, int K, int* __restrict__ start)
{
    __shared__ int s[256];
    int local = 0;
    for (int u = 0; u < 16; ++u) {
        const int j = threadIdx.x * 16 + u;
        if (j < K) local += (int)counts[j];
    }
    s[threadIdx.x] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) {
            const int v = s[t];
            s[t] = run;
            run += v;
        }
    }
    __syncthreads();
    int run = s[threadIdx.x];
    for (int u = 0; u < 16; ++u) {
        const int j = threadIdx.x * 16 + u;
        if (j < K) {
            start[j] = run;
            run += (int)counts[j];
            if (j == K - 1) start[K] = run;
        }
    }
}

// perm[start[j] + rank] = i: the rank of row i among the rows of its label, in ascending row order.  One wave per chunk walks
// its rows 64 at a time; the lanes that share a label take consecutive places after the label's running count in LDS.
__global__ void __launch_bounds__(64) k_km_scatter(const int* __restrict__ labels, int n, int K, int chunk_rows, const int* __restrict__ hist,
                                                   const int* __restrict__ start, int* __restrict__ perm)
{
    __shared__ int run[kKmMaxK];
    const int lane = threadIdx.x;
    for (int j = lane; j < K; j += 64) run[j] = start[j] + hist[(size_t)blockIdx.x * K + j];
    __syncthreads();
    const long long beg = (long long)blockIdx.x * chunk_rows;
    const long long end = beg + chunk_rows < (long long)n ? beg + chunk_rows : (long long)n;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long long i0 = beg; i0 < end; i0 += 64) {
        const long long i = i0 + lane;
        int l = i < end ? labels[i] : -1;
        if (l >= K) l = -1;
        unsigned long long todo = __ballot(l >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int lj = __shfl(l, leader, 64);
            const unsigned long long same = __ballot(l == lj);
            const int base = run[lj];
            if (l == lj) perm[base + __popcll(same & below)] = (int)i;
            __syncthreads();
            if (lane == leader) run[lj] = base + __popcll(same);
            __syncthreads();
            todo &= ~same;
        }
    }
}

// Workgroup (cluster j, block of 16 columns): thread (g, c) adds the rows of ranks g, g + 16, g + 32, ... of the cluster in
// ascending order, then the sixteen partial sums are added in ascending g.  new = sum / count; an empty cluster keeps old.
__global__ void __launch_bounds__(256) k_km_gather(const float* __restrict__ x, int d, const int* __restrict__ perm, const int* __restrict__ start,
                                                   const double* __restrict__ old, double* __restrict__ fresh)
{
    __shared__ double p[16][17];
    const int j = blockIdx.x, g = threadIdx.x >> 4, cc = threadIdx.x & 15, c = blockIdx.y * 16 + cc;
    const int s0 = start[j], m = start[j + 1] - s0;
    double acc = 0.0;
    if (c < d) {
#pragma unroll 4
        for (int t = g; t < m; t += 16) acc = acc + (double)x[(size_t)perm[s0 + t] * d + c];
    }
    p[g][cc] = acc;
    __syncthreads();
    if (g == 0 && c < d) {
        double tot = p[0][cc];
#pragma unroll
        for (int u = 1; u < 16; ++u) tot = tot + p[u][cc];
        fresh[(size_t)j * d + c] = m > 0 ? tot / (double)m : old[(size_t)j * d + c];
    }
}

// sq[j] = sum_c (fresh[j][c] - old[j][c])^2, columns ascending
__global__ void __launch_bounds__(256) k_km_shift(const double* __restrict__ old, const double* __restrict__ fresh, int K, int d,
                                                  double* __restrict__ sq)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K) return;
    double acc = 0.0;
    for (int c = 0; c < d; ++c) {
        const double t = fresh[(size_t)j * d + c] - old[(size_t)j * d + c];
        acc = acc + t * t;
    }
    sq[j] = acc;
}

// out[0] = sq[0] + sq[1] + ... in ascending order
__global__ void __launch_bounds__(256) k_km_serial_sum(const double* __restrict__ sq, int K, double* __restrict__ out)
{
    __shared__ double s[kKmMaxK];
    for (int j = threadIdx.x; j < K; j += 256) s[j] = sq[j];
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int j = 0; j < K; ++j) acc = acc + s[j];
        out[0] = acc;
    }
}

// ---- S93 seeding (k-means++) ---------------------------------------------------------------------------------------------

__device__ __forceinline__ int floor_row(double u, int n)
{
    const double f = floor(u * (double)n);
    return f >= (double)n ? n - 1 : (f >= 0.0 ? (int)f : 0);  // NaN: row 0
}

__global__ void __launch_bounds__(256) k_seed_init(int n, int K, double* __restrict__ m, int* __restrict__ cand, int* __restrict__ last)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) m[i] = INFINITY;
    if (i < K) cand[i] = INT_MAX, last[i] = -1;
}

// m[i] = min(m[i], sum_c (x[i][c] - x[rows[j-1]][c])^2) and bs[block] = the block's sum of m (va_wg_sum256; rows past n add 0)
__global__ void __launch_bounds__(256) k_seed_dist(const float* __restrict__ x, int n, int d, const int* __restrict__ rows, int j,
                                                   double* __restrict__ m, double* __restrict__ bs)
{
    __shared__ double red[4];
    __shared__ float xs[256 * kDirectLd];
    const long long r0 = (long long)blockIdx.x * 256, i = r0 + threadIdx.x;
    const double acc = direct_d2(x, r0, n, d, x + (size_t)rows[j - 1] * d, xs);
    double v = 0.0;
    if (i < n) {
        const double mo = m[i];
        v = acc < mo ? acc : mo;
        m[i] = v;
    }
    const double s = va_wg_sum256(v, red);
    if (threadIdx.x == 0) bs[blockIdx.x] = s;
}

// pre[b] = bs[0] + ... + bs[b-1] in ascending order, tt[0] = the total, tt[1] = u[j] * total.  One workgroup: all threads
// carry 2048 block sums at a time through LDS, thread 0 adds them one after the other.
__global__ void __launch_bounds__(256) k_seed_prefix(const double* __restrict__ bs, long long nb, const double* __restrict__ u, int j,
                                                     double* __restrict__ pre, double* __restrict__ tt)
{
    __shared__ double s[2048];
    __shared__ double carry;
    if (threadIdx.x == 0) carry = 0.0;
    for (long long b0 = 0; b0 < nb; b0 += 2048) {
        const int cnt = (int)(nb - b0 < 2048 ? nb - b0 : 2048);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += 256) s[t] = bs[b0 + t];
        __syncthreads();
        if (threadIdx.x == 0) {
            double run = carry;
#pragma unroll 8
            for (int t = 0; t < cnt; ++t) {
                const double v = s[t];
                s[t] = run;
                run = run + v;
            }
            carry = run;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += 256) pre[b0 + t] = s[t];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        tt[0] = carry;
        tt[1] = u[j] * carry;
    }
}

// One thread per block of 256 rows: the running sum starts at pre[block] and adds the block's rows in ascending order; the
// first row at which it exceeds tt[1] is a candidate (the lowest over all blocks is kept), and so is the last row with m > 0.
__global__ void __launch_bounds__(256) k_seed_search(const double* __restrict__ m, int n, long long nb, const double* __restrict__ pre,
                                                     const double* __restrict__ tt, int* __restrict__ cand, int* __restrict__ last)
{
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const double t = tt[1];
    double run = pre[b];
    const long long beg = b * kSumBlock, end = beg + kSumBlock < (long long)n ? beg + kSumBlock : (long long)n;
    int first = -1, pos = -1;
#pragma unroll 8
    for (long long i = beg; i < end; ++i) {
        const double v = m[i];
        run = run + v;
        if (first < 0 && run > t) first = (int)i;
        if (v > 0.0) pos = (int)i;
    }
    if (first >= 0) atomicMin(cand, first);
    if (pos >= 0) atomicMax(last, pos);
}

// rows[j] and centres[j]: step 0 and a total that is not positive take floor(u[j] n); else the candidate, else the last row
// with m > 0
__global__ void __launch_bounds__(256) k_seed_pick(const float* __restrict__ x, int n, int d, const double* __restrict__ u, int j,
                                                   const double* __restrict__ tt, const int* __restrict__ cand, const int* __restrict__ last,
                                                   int* __restrict__ rows, double* __restrict__ centres)
{
    int pick;
    if (j == 0 || !(tt[0] > 0.0)) pick = floor_row(u[j], n);
    else pick = cand[0] != INT_MAX ? cand[0] : last[0];
    pick = pick < 0 ? 0 : (pick < n ? pick : n - 1);
    if (threadIdx.x == 0) rows[j] = pick;
    for (int c = threadIdx.x; c < d; c += 256) centres[(size_t)j * d + c] = (double)x[(size_t)pick * d + c];
}

// ---- S94 histograms --------------------------------------------------------------------------------------------------------

// One workgroup per segment: integer counts in LDS, then the norm over the words in ascending order, one division each.
__global__ void __launch_bounds__(256) k_bow_hist(const int* __restrict__ labels, int n, const long long* __restrict__ seg, int K, int norm,
                                                  float* __restrict__ out)
{
    __shared__ int h[kKmMaxK];
    __shared__ double scale;
    for (int j = threadIdx.x; j < K; j += 256) h[j] = 0;
    __syncthreads();
    long long beg = seg[blockIdx.x], end = seg[blockIdx.x + 1];  // clamped to the rows there are
    beg = beg < 0 ? 0 : beg;
    end = end > (long long)n ? (long long)n : end;
    for (long long i = beg + threadIdx.x; i < end; i += 256) {
        const int l = labels[i];
        if (l >= 0 && l < K) atomicAdd(&h[l], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        if (norm == VA_BOW_L2) {
            for (int j = 0; j < K; ++j) acc = acc + (double)h[j] * (double)h[j];
            acc = sqrt(acc);
        } else if (norm == VA_BOW_L1) {
            for (int j = 0; j < K; ++j) acc = acc + (double)h[j];
        }
        scale = acc;
    }
    __syncthreads();
    const double s = scale;
    float* __restrict__ o = out + (size_t)blockIdx.x * K;
    for (int j = threadIdx.x; j < K; j += 256) {
        const double v = (double)h[j];
        o[j] = (float)(norm == VA_BOW_NONE ? v : (s > 0.0 ? v / s : 0.0));
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------

struct KmPlan {
    int chunk_rows, chunks;
    long long blocks;  // blocks of kSumBlock rows
    double *hn, *sq, *part, *pre, *tt;
    int *labels, *perm, *hist, *start, *cand, *last;
    size_t bytes;
};

// The argument checks every entry point shares, and the workspace cut from `base` (NULL: the size alone)
int km_plan(const char* who, long long n, int d, int k, int n_segments, const va_kmeans_params* p, void* base, KmPlan* out)
{
    va_kmeans_params def;
    va_kmeans_default_params(&def);
    if (p == nullptr) p = &def;
    VA_CHECK_ARG(p->struct_bytes >= (int)sizeof(va_kmeans_params), "%s: struct_bytes %d is smaller than sizeof(va_kmeans_params) = %d", who,
                 p->struct_bytes, (int)sizeof(va_kmeans_params));
    VA_CHECK_ARG(n >= 1 && n <= INT_MAX, "%s: n out of range: need 1 <= n <= %d (got %lld)", who, INT_MAX, n);
    VA_CHECK_ARG(d >= 1 && d <= kKmMaxDim, "%s: d out of range: need 1 <= d <= %d (got %d)", who, kKmMaxDim, d);
    VA_CHECK_ARG(k >= 1 && k <= kKmMaxK, "%s: k out of range: need 1 <= k <= %d (got %d)", who, kKmMaxK, k);
    VA_CHECK_ARG(n_segments >= 1 && n_segments <= kKmMaxSegments, "%s: n_segments out of range: need 1 <= n_segments <= %d (got %d)", who,
                 kKmMaxSegments, n_segments);
    VA_CHECK_ARG(p->chunk_rows >= kKmMinChunk && p->chunk_rows <= kKmMaxChunk,
                 "%s: chunk_rows out of range: need %d <= chunk_rows <= %d (got %d)", who, kKmMinChunk, kKmMaxChunk, p->chunk_rows);
    KmPlan g;
    long long cr = p->chunk_rows;
    const long long least = (n + kKmMaxChunks - 1) / kKmMaxChunks;  // never more than 65536 chunks: the sort is stable, so the
    if (cr < least) cr = (least + 63) / 64 * 64;                    // chunk size does not reach the result
    g.chunk_rows = (int)cr;
    g.chunks = (int)((n + cr - 1) / cr);
    g.blocks = (n + kSumBlock - 1) / kSumBlock;
    va_carver ws{base};
    g.hn = ws.take<double>((size_t)k);
    g.sq = ws.take<double>((size_t)k);
    g.part = ws.take<double>((size_t)g.blocks);
    g.pre = ws.take<double>((size_t)g.blocks);
    g.tt = ws.take<double>(2);
    g.labels = ws.take<int>((size_t)n);
    g.perm = ws.take<int>((size_t)n);
    g.hist = ws.take<int>((size_t)g.chunks * k);
    g.start = ws.take<int>((size_t)k + 1);
    g.cand = ws.take<int>((size_t)k);
    g.last = ws.take<int>((size_t)k);
    g.bytes = ws.off;
    if (out) *out = g;
    return VA_OK;
}

// the workspace's pointer, the plan and the workspace's size, in that order
int km_ready(const char* who, int n, int d, int k, int n_segments, const va_kmeans_params* p, void* workspace, size_t workspace_bytes,
             KmPlan* g)
{
    VA_CHECK_ARG(workspace != nullptr && ((size_t)workspace & 255) == 0, "%s: workspace must be a 256-byte aligned DEVICE pointer", who);
    if (int rc = km_plan(who, n, d, k, n_segments, p, workspace, g)) return rc;
    if (workspace_bytes < g->bytes) {
        va_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, g->bytes);
        return VA_ERR_WORKSPACE;
    }
    return VA_OK;
}

void km_launch_assign(const KmPlan& g, const float* x, int n, int d, const double* centres, int k, int* labels, hipStream_t st)
{
    k_km_halfnorm<<<va_cdiv(k, 256), 256, 0, st>>>(centres, k, d, g.hn);
    k_km_assign<<<(unsigned)(((long long)n + kWgRows - 1) / kWgRows), 256, 0, st>>>(x, n, d, centres, k, g.hn, labels);
}

bool bow_norm_ok(int norm) { return norm == VA_BOW_NONE || norm == VA_BOW_L1 || norm == VA_BOW_L2; }

}  // namespace

extern "C" void va_kmeans_default_params(va_kmeans_params* p)
{
    if (p == nullptr) return;
    *p = va_kmeans_params{};
    p->struct_bytes = (int)sizeof(va_kmeans_params);
    p->chunk_rows = 8192;
}

extern "C" int va_kmeans_tile_centres(void) { return kTileK; }

extern "C" size_t va_kmeans_workspace_bytes(int n, int d, int k, int n_segments, const va_kmeans_params* p)
{
    KmPlan g;
    if (km_plan("va_kmeans_workspace_bytes", n, d, k, n_segments, p, nullptr, &g) != VA_OK) return 0;
    return g.bytes;
}

extern "C" int va_kmeans_assign(va_ctx* ctx, const void* x, int n, int d, const void* centres, int k, const void* prev_labels, void* labels,
                                void* d2, void* inertia, void* changed, void* workspace, size_t workspace_bytes, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_kmeans_assign: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x && centres && labels && inertia && changed, "va_kmeans_assign: NULL pointer");
    VA_CHECK_ARG(prev_labels != labels, "va_kmeans_assign: prev_labels and labels must not be the same array");
    KmPlan g;
    const int rc = km_ready("va_kmeans_assign", n, d, k, 1, nullptr, workspace, workspace_bytes, &g);
    if (rc != VA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    VA_HIP(hipMemsetAsync(changed, 0, sizeof(unsigned long long), st));
    km_launch_assign(g, (const float*)x, n, d, (const double*)centres, k, (int*)labels, st);
    k_km_d2<<<(unsigned)g.blocks, 256, 0, st>>>((const float*)x, n, d, (const double*)centres, k, (const int*)labels, (const int*)prev_labels,
                                                (double*)d2, g.part, (unsigned long long*)changed);
    k_km_sum_parts<<<1, 256, 0, st>>>(g.part, g.blocks, (double*)inertia);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_kmeans_update(va_ctx* ctx, const void* x, int n, int d, const void* labels, const void* centres, int k,
                                const va_kmeans_params* p, void* counts, void* new_centres, void* shift2, void* workspace,
                                size_t workspace_bytes, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_kmeans_update: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x && labels && centres && counts && new_centres && shift2, "va_kmeans_update: NULL pointer");
    VA_CHECK_ARG(centres != new_centres, "va_kmeans_update: centres and new_centres must not be the same array");
    KmPlan g;
    const int rc = km_ready("va_kmeans_update", n, d, k, 1, p, workspace, workspace_bytes, &g);
    if (rc != VA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    k_km_count<<<g.chunks, 256, 0, st>>>((const int*)labels, n, k, g.chunk_rows, g.hist);
    k_km_scan_chunks<<<va_cdiv(k, 256), 256, 0, st>>>(g.hist, g.chunks, k, (long long*)counts);
    k_km_scan_clusters<<<1, 256, 0, st>>>((const long long*)counts, k, g.start);
    k_km_scatter<<<g.chunks, 64, 0, st>>>((const int*)labels, n, k, g.chunk_rows, g.hist, g.start, g.perm);
    k_km_gather<<<dim3(k, va_cdiv(d, 16)), 256, 0, st>>>((const float*)x, d, g.perm, g.start, (const double*)centres, (double*)new_centres);
    k_km_shift<<<va_cdiv(k, 256), 256, 0, st>>>((const double*)centres, (const double*)new_centres, k, d, g.sq);
    k_km_serial_sum<<<1, 256, 0, st>>>(g.sq, k, (double*)shift2);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_kmeans_seed(va_ctx* ctx, const void* x, int n, int d, const void* u, int k, void* centres, void* rows, void* m,
                              void* workspace, size_t workspace_bytes, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_kmeans_seed: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x && u && centres && rows && m, "va_kmeans_seed: NULL pointer");
    KmPlan g;
    const int rc = km_ready("va_kmeans_seed", n, d, k, 1, nullptr, workspace, workspace_bytes, &g);
    if (rc != VA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const float* xf = (const float*)x;
    const double* uf = (const double*)u;
    const unsigned blocks = (unsigned)g.blocks;
    const long long init = n > k ? n : k;
    k_seed_init<<<(unsigned)((init + 255) / 256), 256, 0, st>>>(n, k, (double*)m, g.cand, g.last);
    k_seed_pick<<<1, 256, 0, st>>>(xf, n, d, uf, 0, g.tt, g.cand, g.last, (int*)rows, (double*)centres);
    for (int j = 1; j < k; ++j) {
        k_seed_dist<<<blocks, 256, 0, st>>>(xf, n, d, (const int*)rows, j, (double*)m, g.part);
        k_seed_prefix<<<1, 256, 0, st>>>(g.part, g.blocks, uf, j, g.pre, g.tt);
        k_seed_search<<<(unsigned)((g.blocks + 255) / 256), 256, 0, st>>>((const double*)m, n, g.blocks, g.pre, g.tt, g.cand + j, g.last + j);
        k_seed_pick<<<1, 256, 0, st>>>(xf, n, d, uf, j, g.tt, g.cand + j, g.last + j, (int*)rows, (double*)centres);
    }
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_bow_histograms(va_ctx* ctx, const void* labels, int n, const void* segments, int n_segments, int k, int norm, void* out,
                                 void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_bow_histograms: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(labels && segments && out, "va_bow_histograms: NULL pointer");
    VA_CHECK_ARG(bow_norm_ok(norm), "va_bow_histograms: norm must be VA_BOW_NONE, VA_BOW_L1 or VA_BOW_L2 (got %d)", norm);
    if (int rc = km_plan("va_bow_histograms", n, 1, k, n_segments, nullptr, nullptr, nullptr)) return rc;
    k_bow_hist<<<n_segments, 256, 0, (hipStream_t)stream>>>((const int*)labels, n, (const long long*)segments, k, norm, (float*)out);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_bow_encode(va_ctx* ctx, const void* x, int n, int d, const void* centres, int k, const void* segments, int n_segments,
                             int norm, void* out, void* workspace, size_t workspace_bytes, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_bow_encode: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x && centres && segments && out, "va_bow_encode: NULL pointer");
    VA_CHECK_ARG(bow_norm_ok(norm), "va_bow_encode: norm must be VA_BOW_NONE, VA_BOW_L1 or VA_BOW_L2 (got %d)", norm);
    KmPlan g;
    const int rc = km_ready("va_bow_encode", n, d, k, n_segments, nullptr, workspace, workspace_bytes, &g);
    if (rc != VA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    km_launch_assign(g, (const float*)x, n, d, (const double*)centres, k, g.labels, st);
    k_bow_hist<<<n_segments, 256, 0, st>>>(g.labels, n, (const long long*)segments, k, norm, (float*)out);
    VA_LAUNCH_CHECK();
    return VA_OK;
}
