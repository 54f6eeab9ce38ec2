// Dense trajectories for gfx950 (MI355X): hand-written HIP, no CPU fallback.
//
// H. Wang, A. Klaeser, C. Schmid, C.-L. Liu, "Action recognition by dense trajectories" (CVPR 2011), with the constants of
// the modelled project's Sheet02.  DESIGN.md S69-S76 fix every expression and its operation order.  Orientation votes are
// float32 (a fixed polynomial instead of a library arctangent: S70), quantised once to fixed point (S71); from there on every
// sum is an integer sum, so that no result depends on a reduction order, a tile shape or a chunk length.  This file is
// compiled with -ffp-contract=off and writes no fmaf of its own.
//
//   votes     u32 [frame][33][h][w]        planes: HOG 0-7, HOF 8-16 (bin 8 of HOF is plane 16), MBHx 17-24, MBHy 25-32
//   integral  u32 [frame][33][h+1][w+1]    S72, sums mod 2^32
//   state     one buffer (va_dtraj_state_layout): counts, the two lists of live slots, and per slot the start frame, the
//             points and the 64-bit accumulators.  A track that starts at frame t in grid cell c owns slot (t mod length) *
//             cells + c for its `length` steps: no allocation, and the table of cells * length slots cannot overflow (S76).
//
// Per frame the host makes the same launches whatever the counts are; kernels read the live count from the state.
#include "va_feature_device.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int kNT = 256;
constexpr int kPlanes = 33;
constexpr int kDefChunk = 8, kDefTileW = 64, kDefTileH = 4;
constexpr int kCornerTW = 32, kCornerTH = 8;
constexpr int kScanNT = 1024;

// S71: fixed point.  (patch / nxy)^2 <= 4096 pixels per cell, so a cell's sum stays below 4096 * VMAX * 2^S = 2^31 < 2^32.
constexpr float kHogVmax = 2048.0f, kHogScale = 256.0f;      // S = 8
constexpr float kFlowVmax = 32.0f, kFlowScale = 16384.0f;    // S = 14
constexpr double kHogUnit = 1.0 / 256.0, kFlowUnit = 1.0 / 16384.0;

// state counts (int32 each)
enum { C_LIVE = 0, C_CUR = 1, C_OUT = 2, C_OUT0 = 3, C_REJ = 4, C_WORDS = 16 };
// what a step leaves for a track
enum { ST_ALIVE = 0, ST_LEFT = 1, ST_DONE = 2 };
// va_dtraj_state_layout's regions
enum { R_COUNTS = 0, R_LIVE, R_STAT, R_START, R_PTS, R_ACC, R_OCC, R_PEND, R_N };

struct Geo {
    int w, h, step, L, patch, nxy, nt;
    int ncx, ncy, cells, slots;
    int cs;    // side of a descriptor cell: patch / nxy
    int tlen;  // steps per temporal cell: L / nt
    int accn;  // accumulators per slot: nt * nxy^2 * 33
    int dim;   // descriptor length: 2 L + accn
    float quality, min_flow;
    double min_std, max_std, max_dis, max_dis_share;
};

struct State {
    int* counts;
    int* live;   // [2][slots]
    int* stat;   // [slots], by list position
    int* start;  // [slots]
    float* pts;  // [slots][L+1][2]
    unsigned long long* acc;  // [slots][nt][nxy^2][33]
    int* occ;    // [cells]
    int* pend;   // [slots]: the slots whose descriptors the current frame writes
};

__device__ __forceinline__ int d_clampi(int v, int lo, int hi) { return d_min(d_max(v, lo), hi); }

// S69: 3x3 Sobel of a tile at (ry, rx); rows RW floats apart
__device__ __forceinline__ void sobel(const float* t, int RW, float& gx, float& gy)
{
    const float tl = t[-RW - 1], tc = t[-RW], tr = t[-RW + 1];
    const float l = t[-1], r = t[1];
    const float bl = t[RW - 1], bc = t[RW], br = t[RW + 1];
    gx = ((tr - tl) + 2.0f * (r - l)) + (br - bl);
    gy = ((bl - tl) + 2.0f * (bc - tc)) + (br - tr);
}

struct VoteArgs {
    const void* gray;   // frame f: [h][w] at gray + f * h * w elements
    const float* flow;  // [frame][2][h][w], unfiltered
    unsigned* out;      // [frame][33][h][w]
    int gray_u8, w, h, TW, TH, ntx;
    float min_flow;
};

// S69-S71 with 8 bins in every group (va_votes_of, va_store_bins).  grid (tiles, frames); dynamic LDS: 3 (TW + 2)(TH + 2) floats.
// Lanes run along x: every plane's stores of a wave are one contiguous run.
__global__ void __launch_bounds__(kNT) k_dtraj_votes(VoteArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int f = blockIdx.y;
    const int ty0 = blockIdx.x / a.ntx, tx0 = blockIdx.x - ty0 * a.ntx;
    const int x0 = tx0 * a.TW, y0 = ty0 * a.TH;
    const int RW = a.TW + 2, RH = a.TH + 2, rsz = RW * RH;
    float* G = lds;
    float* U = lds + rsz;
    float* V = lds + 2 * rsz;
    const size_t fl = (size_t)a.w * a.h;
    const float* u = a.flow + (size_t)f * 2 * fl;
    const float* v = u + fl;
    for (int i = threadIdx.x; i < rsz; i += kNT) {
        const int ry = i / RW, rx = i - ry * RW;
        const int gx = d_clampi(x0 - 1 + rx, 0, a.w - 1), gy = d_clampi(y0 - 1 + ry, 0, a.h - 1);
        const size_t o = (size_t)gy * a.w + gx;
        G[i] = a.gray_u8 ? (float)((const unsigned char*)a.gray)[(size_t)f * fl + o] : ((const float*)a.gray)[(size_t)f * fl + o];
        U[i] = u[o];
        V[i] = v[o];
    }
    __syncthreads();
    unsigned* out = a.out + (size_t)f * kPlanes * fl;
    for (int i = threadIdx.x; i < a.TW * a.TH; i += kNT) {
        const int ty = i / a.TW, tx = i - ty * a.TW;
        const int gx = x0 + tx, gy = y0 + ty;
        if (gx >= a.w || gy >= a.h) continue;
        const int c = (ty + 1) * RW + tx + 1;
        unsigned* o = out + (size_t)gy * a.w + gx;
        float dx, dy, m;
        int b0;
        unsigned q0, q1;
        sobel(G + c, RW, dx, dy);  // HOG
        va_votes_of(dx, dy, kHogVmax, kHogScale, 8, b0, q0, q1, m);
        va_store_bins(o, fl, 8, b0, q0, q1);
        va_votes_of(U[c], V[c], kFlowVmax, kFlowScale, 8, b0, q0, q1, m);  // HOF: the flow itself, and the bin of the still pixels
        const bool still = m <= a.min_flow;
        if (still) q0 = 0u, q1 = 0u;
        va_store_bins(o + 8 * fl, fl, 8, b0, q0, q1);
        o[16 * fl] = still ? (unsigned)kFlowScale : 0u;
        sobel(U + c, RW, dx, dy);  // MBHx
        va_votes_of(dx, dy, kFlowVmax, kFlowScale, 8, b0, q0, q1, m);
        va_store_bins(o + 17 * fl, fl, 8, b0, q0, q1);
        sobel(V + c, RW, dx, dy);  // MBHy
        va_votes_of(dx, dy, kFlowVmax, kFlowScale, 8, b0, q0, q1, m);
        va_store_bins(o + 25 * fl, fl, 8, b0, q0, q1);
    }
}

// S72, first pass: one wave per row, inclusive scans of 64 with a carried prefix; row y of a plane lands in row y + 1 of the
// integral, one column to the right.  Sums are mod 2^32, so the order is free.
__global__ void __launch_bounds__(kNT) k_dtraj_scan_rows(const unsigned* __restrict__ q, unsigned* __restrict__ I, int w, int h,
                                                          long long rows)
{
    const long long row = (long long)blockIdx.x * (kNT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const long long plane = row / h;
    const int y = (int)(row - plane * h);
    const unsigned* src = q + (size_t)row * w;
    unsigned* dst = I + ((size_t)plane * (h + 1) + y + 1) * (size_t)(w + 1);
    if (lane == 0) dst[0] = 0u;
    unsigned carry = 0u;
    for (int x0 = 0; x0 < w; x0 += 64) {
        const int x = x0 + lane;
        const unsigned v = va_wave_scan_incl(x < w ? src[x] : 0u, lane) + carry;
        if (x < w) dst[x + 1] = v;
        carry = __shfl(v, 63);
    }
}

// S72, second pass: one lane per column, running down; row 0 is written here
__global__ void __launch_bounds__(kNT) k_dtraj_scan_cols(unsigned* __restrict__ I, int w, int h, long long cols)
{
    const long long i = (long long)blockIdx.x * kNT + threadIdx.x;
    if (i >= cols) return;
    const long long plane = i / (w + 1);
    const int x = (int)(i - plane * (w + 1));
    unsigned* p = I + (size_t)plane * (h + 1) * (size_t)(w + 1) + x;
    unsigned acc = 0u;
    p[0] = 0u;
    for (int y = 1; y <= h; ++y) {
        acc += p[(size_t)y * (w + 1)];
        p[(size_t)y * (w + 1)] = acc;
    }
}

// S73: the smaller eigenvalue of the 3x3 box sum of the structure tensor, and the frame's maximum as an integer maximum of bit
// patterns (the responses are >= +0).  grid (tiles, frames), one pixel per thread.
__global__ void __launch_bounds__(kNT) k_dtraj_corner(const void* gray, int gray_u8, float* resp, unsigned* maxbits, int w, int h, int ntx)
{
    constexpr int GW = kCornerTW + 4, GH = kCornerTH + 4, PW = kCornerTW + 2, PH = kCornerTH + 2;
    __shared__ float G[GW * GH], XX[PW * PH], XY[PW * PH], YY[PW * PH];
    __shared__ unsigned wgmax;
    const int f = blockIdx.y;
    const int ty0 = blockIdx.x / ntx, tx0 = blockIdx.x - ty0 * ntx;
    const int x0 = tx0 * kCornerTW, y0 = ty0 * kCornerTH;
    const size_t fl = (size_t)w * h;
    for (int i = threadIdx.x; i < GW * GH; i += kNT) {
        const int ry = i / GW, rx = i - ry * GW;
        const int gx = d_clampi(x0 - 2 + rx, 0, w - 1), gy = d_clampi(y0 - 2 + ry, 0, h - 1);
        const size_t o = (size_t)f * fl + (size_t)gy * w + gx;
        G[i] = gray_u8 ? (float)((const unsigned char*)gray)[o] : ((const float*)gray)[o];
    }
    __syncthreads();
    // the gradient products of the tile and its ring: a ring cell outside the frame is its clamped pixel's
    for (int i = threadIdx.x; i < PW * PH; i += kNT) {
        const int ry = i / PW, rx = i - ry * PW;
        const int px = d_clampi(x0 - 1 + rx, 0, w - 1), py = d_clampi(y0 - 1 + ry, 0, h - 1);
        float dx, dy;
        sobel(G + (py - (y0 - 2)) * GW + (px - (x0 - 2)), GW, dx, dy);
        XX[i] = dx * dx, XY[i] = dx * dy, YY[i] = dy * dy;
    }
    __syncthreads();
    const int ty = threadIdx.x / kCornerTW, tx = threadIdx.x - ty * kCornerTW;
    const int gx = x0 + tx, gy = y0 + ty;
    float lam = 0.0f;
    if (gx < w && gy < h) {
        const int c = ty * PW + tx;  // top left of the window
        float sa = XX[c], sb = XY[c], sc = YY[c];
#pragma unroll
        for (int k = 1; k < 9; ++k) {
            const int o = c + (k / 3) * PW + (k % 3);
            sa = sa + XX[o], sb = sb + XY[o], sc = sc + YY[o];
        }
        const float d = sa - sc;
        const float r = sqrtf(d * d + 4.0f * (sb * sb));
        lam = ((sa + sc) - r) * 0.5f;
        lam = lam > 0.0f ? lam : 0.0f;
        resp[(size_t)f * fl + (size_t)gy * w + gx] = lam;
    }
    unsigned bits = __float_as_uint(lam);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = __shfl_xor(bits, d);
        bits = o > bits ? o : bits;
    }
    // one atomic per workgroup: thousands of them on one frame's word would otherwise be the kernel's time
    if (threadIdx.x == 0) wgmax = 0u;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && bits != 0u) atomicMax(&wgmax, bits);
    __syncthreads();
    if (threadIdx.x == 0 && wgmax != 0u) atomicMax(maxbits + f, wgmax);
}

// S74: nearest pixel of a position, inside the frame
__device__ __forceinline__ int nearest(float p, int n) { return d_clampi((int)floorf(p + 0.5f), 0, n - 1); }

// S74: the grid cells that hold a live track
__global__ void __launch_bounds__(kNT) k_dtraj_mark(State s, Geo g, int frame)
{
    const int n = d_min(s.counts[C_LIVE], g.slots);
    const int* live = s.live + (s.counts[C_CUR] & 1) * g.slots;
    for (int i = blockIdx.x * kNT + threadIdx.x; i < n; i += gridDim.x * kNT) {
        const int slot = live[i];
        if (slot < 0 || slot >= g.slots) continue;
        const int k = frame - s.start[slot];
        if (k < 0 || k > g.L) continue;
        const float* P = s.pts + ((size_t)slot * (g.L + 1) + k) * 2;
        const int cx = nearest(P[0], g.w) / g.step, cy = nearest(P[1], g.h) / g.step;
        if (cx < g.ncx && cy < g.ncy) s.occ[cy * g.ncx + cx] = 1;
    }
}

// S74: one workgroup walks the cells in raster order and appends the new tracks behind the live ones
__global__ void __launch_bounds__(kScanNT) k_dtraj_sample(State s, Geo g, const float* resp, const unsigned* maxbits, int frame)
{
    __shared__ int sh[kScanNT / 64 + 1];
    const float tq = g.quality * __uint_as_float(maxbits[0]);
    const int n0 = d_min(s.counts[C_LIVE], g.slots);
    int* live = s.live + (s.counts[C_CUR] & 1) * g.slots;
    const int base = (frame % g.L) * g.cells;
    int run = 0;
    __syncthreads();
    for (int c0 = 0; c0 < g.cells; c0 += kScanNT) {
        const int c = c0 + threadIdx.x;
        int flag = 0, px = 0, py = 0;
        if (c < g.cells) {
            const int cy = c / g.ncx, cx = c - cy * g.ncx;
            px = cx * g.step + g.step / 2, py = cy * g.step + g.step / 2;
            flag = s.occ[c] == 0 && resp[(size_t)py * g.w + px] > tq;
            s.occ[c] = 0;
        }
        int total;
        const int idx = n0 + run + va_wg_scan_excl<kScanNT>(flag, total, sh);
        if (flag && idx < g.slots) {  // (idx < slots always holds for a table this library built: S76)
            const int slot = base + c;
            live[idx] = slot;
            s.start[slot] = frame;
            float* P = s.pts + (size_t)slot * (g.L + 1) * 2;
            P[0] = (float)px, P[1] = (float)py;
        }
        run += total;
    }
    if (threadIdx.x == 0) s.counts[C_LIVE] = d_min(n0 + run, g.slots);
}

// S75: one wave per live track.  Lanes share the nxy^2 * 33 four-corner sums; lane 0 moves the point.
__global__ void __launch_bounds__(kNT) k_dtraj_step(State s, Geo g, const unsigned* __restrict__ I, const float* __restrict__ med, int frame)
{
    const int n = d_min(s.counts[C_LIVE], g.slots);
    const int* live = s.live + (s.counts[C_CUR] & 1) * g.slots;
    const int lane = threadIdx.x & 63;
    const int W1 = g.w + 1;
    const size_t ipl = (size_t)(g.h + 1) * W1;
    const int nitems = g.nxy * g.nxy * kPlanes;
    for (int i = blockIdx.x * (kNT / 64) + (threadIdx.x >> 6); i < n; i += gridDim.x * (kNT / 64)) {
        const int slot = live[i];
        const int k = (slot >= 0 && slot < g.slots) ? frame - s.start[slot] : -1;
        if (k < 0 || k >= g.L) {  // (not a table this library built: the track is dropped as one that left)
            if (lane == 0) s.stat[i] = ST_LEFT;
            continue;
        }
        float* P = s.pts + ((size_t)slot * (g.L + 1) + k) * 2;
        const float px = P[0], py = P[1];
        const int rx = nearest(px, g.w), ry = nearest(py, g.h);
        const int wx0 = rx - g.patch / 2, wy0 = ry - g.patch / 2;
        const int tc = k / g.tlen;
        const bool first = k - tc * g.tlen == 0;
        unsigned long long* acc = s.acc + (size_t)slot * g.accn + (size_t)tc * nitems;
        for (int j = lane; j < nitems; j += 64) {
            const int cell = j / kPlanes, pl = j - cell * kPlanes;
            const int cy = cell / g.nxy, cx = cell - cy * g.nxy;
            const int xa = d_clampi(wx0 + cx * g.cs, 0, g.w), xb = d_clampi(wx0 + (cx + 1) * g.cs, 0, g.w);
            const int ya = d_clampi(wy0 + cy * g.cs, 0, g.h), yb = d_clampi(wy0 + (cy + 1) * g.cs, 0, g.h);
            unsigned sum = 0u;
            if (xb > xa && yb > ya) {
                const unsigned* Ip = I + (size_t)pl * ipl;
                sum = Ip[(size_t)yb * W1 + xb] - Ip[(size_t)ya * W1 + xb] - Ip[(size_t)yb * W1 + xa] + Ip[(size_t)ya * W1 + xa];
            }
            acc[j] = first ? (unsigned long long)sum : acc[j] + sum;
        }
        if (lane == 0) {
            const size_t o = (size_t)ry * g.w + rx;
            const float nx = px + med[o], ny = py + med[(size_t)g.w * g.h + o];
            const bool in = nx >= 0.0f && nx <= (float)(g.w - 1) && ny >= 0.0f && ny <= (float)(g.h - 1);  // (a NaN is outside)
            if (in) P[2] = nx, P[3] = ny;
            s.stat[i] = in ? (k + 1 == g.L ? ST_DONE : ST_ALIVE) : ST_LEFT;
        }
    }
}

// S76's tests on the L + 1 points, float64 in the written order: 0 valid, 1 static, 2 erratic, 3 jump.  *total: the length.
__device__ __forceinline__ int classify(const float* P, const Geo& g, double* total)
{
    const int n = g.L + 1;
    double sx = 0.0, sy = 0.0;
    for (int k = 0; k < n; ++k) sx = sx + (double)P[2 * k], sy = sy + (double)P[2 * k + 1];
    const double mx = sx / (double)n, my = sy / (double)n;
    double vx = 0.0, vy = 0.0;
    for (int k = 0; k < n; ++k) {
        const double dx = (double)P[2 * k] - mx, dy = (double)P[2 * k + 1] - my;
        vx = vx + dx * dx, vy = vy + dy * dy;
    }
    const double sdx = sqrt(vx / (double)n), sdy = sqrt(vy / (double)n);
    double len = 0.0, longest = 0.0;
    for (int k = 0; k < g.L; ++k) {
        const double dx = (double)P[2 * k + 2] - (double)P[2 * k], dy = (double)P[2 * k + 3] - (double)P[2 * k + 1];
        const double seg = sqrt(dx * dx + dy * dy);
        len = len + seg;
        longest = seg > longest ? seg : longest;
    }
    *total = len;
    if (sdx < g.min_std && sdy < g.min_std) return 1;
    if (sdx > g.max_std || sdy > g.max_std) return 2;
    if (longest > g.max_dis) return 3;
    if (longest > g.max_dis_share * len) return 3;
    return 0;
}

// S76: one workgroup walks the live list in order: the survivors go to the other list, the valid finished tracks to `pend`
__global__ void __launch_bounds__(kScanNT) k_dtraj_finish(State s, Geo g)
{
    __shared__ int sh[kScanNT / 64 + 1];
    __shared__ int rej[4];
    if (threadIdx.x < 4) rej[threadIdx.x] = 0;
    const int n = d_min(s.counts[C_LIVE], g.slots);
    const int cur = s.counts[C_CUR] & 1;
    const int out0 = s.counts[C_OUT];
    const int* live = s.live + cur * g.slots;
    int* next = s.live + (cur ^ 1) * g.slots;
    int run_a = 0, run_o = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += kScanNT) {
        const int i = i0 + threadIdx.x;
        int alive = 0, valid = 0, slot = 0;
        if (i < n) {
            slot = live[i];
            const int st = s.stat[i];
            alive = st == ST_ALIVE;
            if (st == ST_LEFT) atomicAdd(&rej[0], 1);
            if (st == ST_DONE && slot >= 0 && slot < g.slots) {
                double len;
                const int code = classify(s.pts + (size_t)slot * (g.L + 1) * 2, g, &len);
                valid = code == 0;
                if (code) atomicAdd(&rej[code], 1);
            }
        }
        int ta, to;
        const int pa = va_wg_scan_excl<kScanNT>(alive, ta, sh);
        const int po = va_wg_scan_excl<kScanNT>(valid, to, sh);
        if (alive) next[run_a + pa] = slot;
        if (valid) s.pend[run_o + po] = slot;
        run_a += ta, run_o += to;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        s.counts[C_LIVE] = run_a;
        s.counts[C_CUR] = cur ^ 1;
        s.counts[C_OUT0] = out0;
        s.counts[C_OUT] = out0 + run_o;
        for (int k = 0; k < 4; ++k) s.counts[C_REJ + k] += rej[k];
    }
}

// S76: the descriptor, one wave per valid track.  Every lane adds the float64 squares in index order, so all hold the same norm.
__global__ void __launch_bounds__(kNT) k_dtraj_desc(State s, Geo g, float* desc, float* points, int* starts, int capacity)
{
    const int out0 = s.counts[C_OUT0], n = s.counts[C_OUT] - out0;
    const int lane = threadIdx.x & 63;
    const int ncell = g.nt * g.nxy * g.nxy;
    for (int j = blockIdx.x * (kNT / 64) + (threadIdx.x >> 6); j < n; j += gridDim.x * (kNT / 64)) {
        const int o = out0 + j;
        if (o >= capacity) continue;  // (counted, not written: the caller reads the count)
        const int slot = s.pend[j];
        const float* P = s.pts + (size_t)slot * (g.L + 1) * 2;
        float* D = desc + (size_t)o * g.dim;
        float* Q = points + (size_t)o * (g.L + 1) * 2;
        if (lane == 0) starts[o] = s.start[slot];
        for (int k = lane; k < 2 * (g.L + 1); k += 64) Q[k] = P[k];
        double len;
        classify(P, g, &len);
        for (int k = lane; k < 2 * g.L; k += 64) D[k] = (float)(((double)P[k + 2] - (double)P[k]) / len);
        const unsigned long long* acc = s.acc + (size_t)slot * g.accn;
        int off = 2 * g.L;
        for (int b = 0; b < 4; ++b) {
            const int p0 = b == 0 ? 0 : (b == 1 ? 8 : (b == 2 ? 17 : 25)), nb = b == 1 ? 9 : 8;
            const double unit = b == 0 ? kHogUnit : kFlowUnit;
            const int cnt = ncell * nb;
            // 64 values at a time: every lane loads and squares one, then all add the 64 squares in lane order (a lane past the
            // block's end holds +0, which changes no sum)
            double ss = 0.0;
            for (int e0 = 0; e0 < cnt; e0 += 64) {
                const int e = e0 + lane, c = e / nb, bin = e - c * nb;
                const double v = e < cnt ? (double)acc[c * kPlanes + p0 + bin] * unit : 0.0;
                const double sq = v * v;
#pragma unroll
                for (int i = 0; i < 64; ++i) ss = ss + __shfl(sq, i);
            }
            const double norm = sqrt(ss);
            for (int e = lane; e < cnt; e += 64) {
                const int c = e / nb, bin = e - c * nb;
                const double v = (double)acc[c * kPlanes + p0 + bin] * unit;
                D[off + e] = norm > 0.0 ? (float)(v / norm) : 0.0f;
            }
            off += cnt;
        }
    }
}

// ---------------------------------------------------------------- host side ------------------

struct Plan {
    Geo g;
    int chunk, TW, TH;
    size_t vote_lds;
    size_t off[R_N], state_bytes;
    size_t off_votes, off_integral, off_resp, off_max, total;
};

int check_params(const va_dtraj_params* p)
{
    VA_CHECK_ARG(p != nullptr, "va_dtraj: params is NULL");
    VA_CHECK_ARG(p->struct_bytes >= (int)sizeof(va_dtraj_params), "va_dtraj: params.struct_bytes is %d, need at least %d", p->struct_bytes,
                 (int)sizeof(va_dtraj_params));
    VA_CHECK_ARG(p->step >= 2 && p->step <= 1024, "va_dtraj: step must be in [2,1024], got %d", p->step);
    VA_CHECK_ARG(p->nt >= 1 && p->nt <= 16, "va_dtraj: nt must be in [1,16], got %d", p->nt);
    VA_CHECK_ARG(p->nxy >= 1 && p->nxy <= 8, "va_dtraj: nxy must be in [1,8], got %d", p->nxy);
    VA_CHECK_ARG(p->length >= 1 && p->length <= 256, "va_dtraj: length must be in [1,256], got %d", p->length);
    VA_CHECK_ARG(p->length % p->nt == 0, "va_dtraj: length (%d) must be a multiple of nt (%d)", p->length, p->nt);
    VA_CHECK_ARG(p->patch >= 1, "va_dtraj: patch must be >= 1, got %d", p->patch);
    VA_CHECK_ARG(p->patch % p->nxy == 0, "va_dtraj: patch (%d) must be a multiple of nxy (%d)", p->patch, p->nxy);
    VA_CHECK_ARG(p->patch / p->nxy <= 64, "va_dtraj: patch / nxy is %d: a cell of more than 4096 pixels could overflow its 32-bit sum",
                 p->patch / p->nxy);
    VA_CHECK_ARG(p->quality > 0.0f && p->quality < 1.0f, "va_dtraj: quality must be in (0,1), got %g", (double)p->quality);
    VA_CHECK_ARG(p->min_flow > 0.0f && p->min_flow <= 3e38f, "va_dtraj: min_flow must be > 0, got %g", (double)p->min_flow);
    VA_CHECK_ARG(p->min_std > 0.0f && p->min_std <= 3e38f, "va_dtraj: min_std must be > 0, got %g", (double)p->min_std);
    VA_CHECK_ARG(p->max_std > 0.0f && p->max_std <= 3e38f, "va_dtraj: max_std must be > 0, got %g", (double)p->max_std);
    VA_CHECK_ARG(p->max_dis > 0.0f && p->max_dis <= 3e38f, "va_dtraj: max_dis must be > 0, got %g", (double)p->max_dis);
    VA_CHECK_ARG(p->max_dis_share > 0.0f && p->max_dis_share <= 3e38f, "va_dtraj: max_dis_share must be > 0, got %g",
                 (double)p->max_dis_share);
    const int* t = p->tuning;
    VA_CHECK_ARG(t[VA_DTRAJ_TUNE_CHUNK] >= 0 && t[VA_DTRAJ_TUNE_CHUNK] <= 4096, "va_dtraj: tuning[0] (frames per chunk) must be 0 or in [1,4096]");
    VA_CHECK_ARG(t[VA_DTRAJ_TUNE_TILE_W] >= 0 && t[VA_DTRAJ_TUNE_TILE_W] <= 256, "va_dtraj: tuning[1] (tile width of the votes) must be 0 or in [1,256]");
    VA_CHECK_ARG(t[VA_DTRAJ_TUNE_TILE_H] >= 0 && t[VA_DTRAJ_TUNE_TILE_H] <= 64, "va_dtraj: tuning[2] (tile height of the votes) must be 0 or in [1,64]");
    VA_CHECK_ARG(t[3] == 0 && t[4] == 0 && t[5] == 0 && t[6] == 0 && t[7] == 0, "va_dtraj: tuning[3..7] are reserved, must be 0");
    return VA_OK;
}

int check_size(const char* who, int w, int h)
{
    VA_CHECK_ARG(w >= 16 && h >= 16 && w <= 16384 && h <= 16384, "%s: frame size %d x %d out of range (w, h in [16,16384])", who, w, h);
    return VA_OK;
}

// parameters and frame size -> geometry, tile and the state's layout
int make_geo(Plan& P, const char* who, int w, int h, const va_dtraj_params* p)
{
    if (int rc = check_params(p)) return rc;
    if (int rc = check_size(who, w, h)) return rc;
    Geo& g = P.g;
    g.w = w, g.h = h, g.step = p->step, g.L = p->length, g.patch = p->patch, g.nxy = p->nxy, g.nt = p->nt;
    g.ncx = w / p->step, g.ncy = h / p->step;
    VA_CHECK_ARG(g.ncx >= 1 && g.ncy >= 1, "%s: step %d leaves no whole grid cell in a %d x %d frame", who, p->step, w, h);
    g.cells = g.ncx * g.ncy;
    VA_CHECK_ARG((long long)g.cells * g.L <= (1LL << 28), "%s: the track table of cells * length = %lld slots is too large (step %d, length %d)",
                 who, (long long)g.cells * g.L, p->step, p->length);
    g.slots = g.cells * g.L;
    g.cs = p->patch / p->nxy, g.tlen = p->length / p->nt;
    g.accn = p->nt * p->nxy * p->nxy * kPlanes;
    g.dim = 2 * g.L + g.accn;
    g.quality = p->quality, g.min_flow = p->min_flow;
    g.min_std = (double)p->min_std, g.max_std = (double)p->max_std, g.max_dis = (double)p->max_dis, g.max_dis_share = (double)p->max_dis_share;
    P.chunk = p->tuning[VA_DTRAJ_TUNE_CHUNK] ? p->tuning[VA_DTRAJ_TUNE_CHUNK] : kDefChunk;
    P.TW = p->tuning[VA_DTRAJ_TUNE_TILE_W] ? p->tuning[VA_DTRAJ_TUNE_TILE_W] : kDefTileW;
    P.TH = p->tuning[VA_DTRAJ_TUNE_TILE_H] ? p->tuning[VA_DTRAJ_TUNE_TILE_H] : kDefTileH;
    P.vote_lds = (size_t)3 * (P.TW + 2) * (P.TH + 2) * sizeof(float);
    VA_CHECK_ARG(P.vote_lds <= (size_t)kVaMaxLds, "%s: tuning: a %d x %d tile of the votes needs %zu bytes of LDS, more than one workgroup holds (%d)",
                 who, P.TW, P.TH, P.vote_lds, kVaMaxLds);
    const size_t slots = (size_t)g.slots;
    const size_t bytes[R_N] = {C_WORDS * sizeof(int), 2 * slots * sizeof(int), slots * sizeof(int), slots * sizeof(int),
                               slots * (g.L + 1) * 2 * sizeof(float), slots * g.accn * sizeof(unsigned long long),
                               (size_t)g.cells * sizeof(int), slots * sizeof(int)};
    va_carver st{nullptr};
    for (int r = 0; r < R_N; ++r) P.off[r] = (size_t)st.take<char>(bytes[r]);
    P.state_bytes = st.off;
    return VA_OK;
}

int make_plan(Plan& P, const char* who, int w, int h, int n_frames, int capacity, const va_dtraj_params* p)
{
    if (int rc = make_geo(P, who, w, h, p)) return rc;
    VA_CHECK_ARG(n_frames >= 2 && n_frames <= 65536, "%s: n_frames must be in [2,65536], got %d", who, n_frames);
    VA_CHECK_ARG(capacity >= 1, "%s: capacity must be >= 1, got %d", who, capacity);
    VA_CHECK_ARG((long long)capacity * P.g.dim <= (1LL << 40), "%s: capacity %d is too large", who, capacity);
    P.chunk = P.chunk < n_frames - 1 ? P.chunk : n_frames - 1;
    const size_t fl = (size_t)w * h, il = (size_t)(w + 1) * (h + 1);
    va_carver ws{nullptr, P.state_bytes};  // the state first, then the chunk's buffers
    P.off_votes = (size_t)ws.take<unsigned>((size_t)P.chunk * kPlanes * fl);
    P.off_integral = (size_t)ws.take<unsigned>((size_t)P.chunk * kPlanes * il);
    P.off_resp = (size_t)ws.take<float>((size_t)P.chunk * fl);
    P.off_max = (size_t)ws.take<unsigned>((size_t)P.chunk);
    P.total = ws.off;
    return VA_OK;
}

State state_of(const Plan& P, void* state)
{
    char* b = (char*)state;
    State s;
    s.counts = (int*)(b + P.off[R_COUNTS]);
    s.live = (int*)(b + P.off[R_LIVE]);
    s.stat = (int*)(b + P.off[R_STAT]);
    s.start = (int*)(b + P.off[R_START]);
    s.pts = (float*)(b + P.off[R_PTS]);
    s.acc = (unsigned long long*)(b + P.off[R_ACC]);
    s.occ = (int*)(b + P.off[R_OCC]);
    s.pend = (int*)(b + P.off[R_PEND]);
    return s;
}

int track_grid(const Geo& g, int per_block) { return std::max(1, std::min(va_cdiv(g.slots, per_block), 2048)); }

int launch_votes(const Plan& P, const void* gray, int gray_u8, const float* flow, unsigned* out, int n, hipStream_t st)
{
    VoteArgs a{};
    a.gray = gray, a.gray_u8 = gray_u8, a.flow = flow, a.out = out;
    a.w = P.g.w, a.h = P.g.h, a.TW = P.TW, a.TH = P.TH, a.ntx = va_cdiv(P.g.w, P.TW);
    a.min_flow = P.g.min_flow;
    if (int rc = va_allow_lds(&k_dtraj_votes, P.vote_lds)) return rc;
    k_dtraj_votes<<<dim3(a.ntx * va_cdiv(P.g.h, P.TH), n), kNT, P.vote_lds, st>>>(a);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

}  // namespace

// S72, both passes (va_internal.h: va_stip_extract sums its votes with it too)
int va_integral_planes(const unsigned* votes, unsigned* out, long long planes, int w, int h, hipStream_t st)
{
    const long long rows = planes * h, cols = planes * (w + 1);
    const long long gr = (rows + kNT / 64 - 1) / (kNT / 64), gc = (cols + kNT - 1) / kNT;
    VA_CHECK_ARG(gr <= 0x7fffffffLL && gc <= 0x7fffffffLL, "va_dtraj: %lld planes of %d x %d are more than one launch scans", planes, w, h);
    k_dtraj_scan_rows<<<(unsigned)gr, kNT, 0, st>>>(votes, out, w, h, rows);
    VA_LAUNCH_CHECK();
    k_dtraj_scan_cols<<<(unsigned)gc, kNT, 0, st>>>(out, w, h, cols);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

namespace {

int launch_corner(const void* gray, int gray_u8, float* resp, unsigned* maxbits, int n, int w, int h, hipStream_t st)
{
    VA_HIP(hipMemsetAsync(maxbits, 0, (size_t)n * sizeof(unsigned), st));
    const int ntx = va_cdiv(w, kCornerTW);
    k_dtraj_corner<<<dim3(ntx * va_cdiv(h, kCornerTH), n), kNT, 0, st>>>(gray, gray_u8, resp, maxbits, w, h, ntx);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

int launch_sample(const Plan& P, const State& s, const float* resp, const unsigned* maxbits, int frame, hipStream_t st)
{
    k_dtraj_mark<<<track_grid(P.g, kNT), kNT, 0, st>>>(s, P.g, frame);
    VA_LAUNCH_CHECK();
    k_dtraj_sample<<<1, kScanNT, 0, st>>>(s, P.g, resp, maxbits, frame);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

int launch_step(const Plan& P, const State& s, const unsigned* integral, const float* med, int frame, hipStream_t st)
{
    k_dtraj_step<<<track_grid(P.g, kNT / 64), kNT, 0, st>>>(s, P.g, integral, med, frame);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

int launch_finish(const Plan& P, const State& s, float* desc, float* points, int* starts, int capacity, hipStream_t st)
{
    k_dtraj_finish<<<1, kScanNT, 0, st>>>(s, P.g);
    VA_LAUNCH_CHECK();
    k_dtraj_desc<<<track_grid(P.g, kNT / 64), kNT, 0, st>>>(s, P.g, desc, points, starts, capacity);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

int check_entry(const char* who, va_ctx* ctx, const void* a, const void* b, const void* c)
{
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_CHECK_ARG(a != nullptr && b != nullptr && c != nullptr, "%s: NULL buffer", who);
    return VA_OK;
}

}  // namespace

extern "C" void va_dtraj_default_params(va_dtraj_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_bytes = (int)sizeof(va_dtraj_params);
    p->step = 5;
    p->length = 15;
    p->patch = 32;
    p->nxy = 2;
    p->nt = 3;
    p->quality = 0.001f;
    p->min_flow = 0.4f;
    p->min_std = 1.7320508f;
    p->max_std = 30.0f;
    p->max_dis = 20.0f;
    p->max_dis_share = 0.7f;
}

extern "C" size_t va_dtraj_workspace_bytes(int w, int h, int n_frames, int capacity, const va_dtraj_params* p)
{
    Plan P;
    if (make_plan(P, "va_dtraj_workspace_bytes", w, h, n_frames, capacity, p) != VA_OK) return 0;
    return P.total;
}

extern "C" size_t va_dtraj_state_layout(int w, int h, const va_dtraj_params* p, size_t* offsets, int capacity)
{
    Plan P;
    if (make_geo(P, "va_dtraj_state_layout", w, h, p) != VA_OK) return 0;
    for (int r = 0; r < R_N && r < capacity; ++r)
        if (offsets) offsets[r] = P.off[r];
    return P.state_bytes;
}

extern "C" int va_dtraj_extract(va_ctx* ctx, const void* gray, int gray_is_u8, const void* flow, const void* flow_median, int n_frames,
                                int w, int h, const va_dtraj_params* p, void* desc, void* points, void* starts, int capacity, int* count,
                                int* rejected, void* workspace, size_t workspace_bytes, void* stream)
{
    if (int rc = check_entry("va_dtraj_extract", ctx, gray, flow, flow_median)) return rc;
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(desc != nullptr && points != nullptr && starts != nullptr && count != nullptr && rejected != nullptr && workspace != nullptr,
                 "va_dtraj_extract: NULL buffer");
    Plan P;
    if (int rc = make_plan(P, "va_dtraj_extract", w, h, n_frames, capacity, p)) return rc;
    VA_CHECK_ARG(((size_t)workspace & 255) == 0, "va_dtraj_extract: workspace must be 256-byte aligned");
    if (workspace_bytes < P.total) {
        va_set_error("va_dtraj_extract: workspace of %zu bytes, need %zu", workspace_bytes, P.total);
        return VA_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const State s = state_of(P, ws);
    unsigned* votes = (unsigned*)(ws + P.off_votes);
    unsigned* integral = (unsigned*)(ws + P.off_integral);
    float* resp = (float*)(ws + P.off_resp);
    unsigned* maxbits = (unsigned*)(ws + P.off_max);
    const Geo& g = P.g;
    const size_t fl = (size_t)w * h, il = (size_t)(w + 1) * (h + 1);
    const size_t gbytes = gray_is_u8 ? 1 : sizeof(float);
    // counts and occupancy start at 0; everything else is written before it is read
    VA_HIP(hipMemsetAsync(s.counts, 0, C_WORDS * sizeof(int), st));
    VA_HIP(hipMemsetAsync(s.occ, 0, (size_t)g.cells * sizeof(int), st));
    const int last_start = n_frames - 1 - g.L;  // S74
    for (int t0 = 0; t0 < n_frames - 1; t0 += P.chunk) {
        const int nc = std::min(P.chunk, n_frames - 1 - t0);
        const char* gr = (const char*)gray + (size_t)t0 * fl * gbytes;
        if (int rc = launch_votes(P, gr, gray_is_u8, (const float*)flow + (size_t)t0 * 2 * fl, votes, nc, st)) return rc;
        if (int rc = va_integral_planes(votes, integral, (long long)nc * kPlanes, w, h, st)) return rc;
        const int ns = std::min(nc, last_start - t0 + 1);
        if (ns > 0)
            if (int rc = launch_corner(gr, gray_is_u8, resp, maxbits, ns, w, h, st)) return rc;
        for (int t = t0; t < t0 + nc; ++t) {
            if (t <= last_start)
                if (int rc = launch_sample(P, s, resp + (size_t)(t - t0) * fl, maxbits + (t - t0), t, st)) return rc;
            if (int rc = launch_step(P, s, integral + (size_t)(t - t0) * kPlanes * il, (const float*)flow_median + (size_t)t * 2 * fl, t, st))
                return rc;
            if (int rc = launch_finish(P, s, (float*)desc, (float*)points, (int*)starts, capacity, st)) return rc;
        }
    }
    int counts[C_WORDS];
    VA_HIP(hipMemcpyAsync(counts, s.counts, sizeof(counts), hipMemcpyDeviceToHost, st));
    VA_HIP(hipStreamSynchronize(st));
    *count = counts[C_OUT];
    for (int k = 0; k < 4; ++k) rejected[k] = counts[C_REJ + k];
    rejected[4] = counts[C_LIVE];  // still live behind the last frame
    return VA_OK;
}

extern "C" int va_dtraj_votes(va_ctx* ctx, const void* gray, int gray_is_u8, const void* flow, int n, int w, int h,
                              const va_dtraj_params* p, void* votes, void* stream)
{
    if (int rc = check_entry("va_dtraj_votes", ctx, gray, flow, votes)) return rc;
    VA_USE_DEVICE(ctx);
    Plan P;
    if (int rc = make_geo(P, "va_dtraj_votes", w, h, p)) return rc;
    VA_CHECK_ARG(n >= 1 && n <= 65535, "va_dtraj_votes: n must be in [1,65535], got %d", n);
    return launch_votes(P, gray, gray_is_u8, (const float*)flow, (unsigned*)votes, n, (hipStream_t)stream);
}

extern "C" int va_dtraj_integral(va_ctx* ctx, const void* votes, int planes, int w, int h, void* integral, void* stream)
{
    if (int rc = check_entry("va_dtraj_integral", ctx, votes, integral, integral)) return rc;
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(planes >= 1 && w >= 1 && h >= 1 && w <= 16384 && h <= 16384, "va_dtraj_integral: planes >= 1 and w, h in [1,16384], got %d, %d x %d",
                 planes, w, h);
    return va_integral_planes((const unsigned*)votes, (unsigned*)integral, planes, w, h, (hipStream_t)stream);
}

extern "C" int va_dtraj_corner(va_ctx* ctx, const void* gray, int gray_is_u8, int n, int w, int h, void* response, void* max_bits,
                               void* stream)
{
    if (int rc = check_entry("va_dtraj_corner", ctx, gray, response, max_bits)) return rc;
    VA_USE_DEVICE(ctx);
    if (int rc = check_size("va_dtraj_corner", w, h)) return rc;
    VA_CHECK_ARG(n >= 1 && n <= 65535, "va_dtraj_corner: n must be in [1,65535], got %d", n);
    return launch_corner(gray, gray_is_u8, (float*)response, (unsigned*)max_bits, n, w, h, (hipStream_t)stream);
}

extern "C" int va_dtraj_sample(va_ctx* ctx, const void* response, const void* max_bits, int w, int h, int frame,
                               const va_dtraj_params* p, void* state, void* stream)
{
    if (int rc = check_entry("va_dtraj_sample", ctx, response, max_bits, state)) return rc;
    VA_USE_DEVICE(ctx);
    Plan P;
    if (int rc = make_geo(P, "va_dtraj_sample", w, h, p)) return rc;
    VA_CHECK_ARG(frame >= 0, "va_dtraj_sample: frame must be >= 0, got %d", frame);
    return launch_sample(P, state_of(P, state), (const float*)response, (const unsigned*)max_bits, frame, (hipStream_t)stream);
}

extern "C" int va_dtraj_step(va_ctx* ctx, const void* integral, const void* flow_median, int w, int h, int frame,
                             const va_dtraj_params* p, void* state, void* stream)
{
    if (int rc = check_entry("va_dtraj_step", ctx, integral, flow_median, state)) return rc;
    VA_USE_DEVICE(ctx);
    Plan P;
    if (int rc = make_geo(P, "va_dtraj_step", w, h, p)) return rc;
    VA_CHECK_ARG(frame >= 0, "va_dtraj_step: frame must be >= 0, got %d", frame);
    return launch_step(P, state_of(P, state), (const unsigned*)integral, (const float*)flow_median, frame, (hipStream_t)stream);
}

extern "C" int va_dtraj_finish(va_ctx* ctx, int w, int h, const va_dtraj_params* p, void* state, void* desc, void* points, void* starts,
                               int capacity, void* stream)
{
    if (int rc = check_entry("va_dtraj_finish", ctx, state, desc, points)) return rc;
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(starts != nullptr, "va_dtraj_finish: NULL buffer");
    Plan P;
    if (int rc = make_geo(P, "va_dtraj_finish", w, h, p)) return rc;
    VA_CHECK_ARG(capacity >= 1, "va_dtraj_finish: capacity must be >= 1, got %d", capacity);
    return launch_finish(P, state_of(P, state), (float*)desc, (float*)points, (int*)starts, capacity, (hipStream_t)stream);
}
