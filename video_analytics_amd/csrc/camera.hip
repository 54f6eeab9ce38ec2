// Warped optical flow, the camera-compensated temporal input of TSN: a robust homography fit over the
// dense TV-L1 field of every pair, and the subtraction of the camera's displacement field from that flow.  Both read the
// TV-L1 buffer [N][2][h][w]; the compensated array has its shape and pair order, so that every S9 - S17 consumer applies to
// it unchanged.  S53 is the first half of TSN's own two-pass form: every pair's second frame warped by H, for a second
// TV-L1 pass that finds the residual motion directly.
#include "va_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// S21: one workgroup per field runs all K iterations of the reweighted least squares in one launch.  Every thread keeps
// the kFitSums distinct sums of the normal equations of its pixels in double registers; they are reduced by a shuffle tree
// per wave and then over the waves in wave order out of LDS, so the summation order is fixed: two runs give the same bits.
// Wave 0 assembles the symmetric 8x8 system in LDS and solves it by Cholesky (all its lanes do the same arithmetic on the
// same LDS words: the control flow around the barriers stays wave-uniform), and g travels back through LDS for the next
// weights.  No atomics, no workspace, no host round trip.
constexpr int kFitThreads = 512;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kFitSums = 27;
constexpr int kFitMaxIters = 1024;

// the sums, with t = omega * (u, v, 1) and u' = u + du, v' = v + dv
enum {
    F_UU, F_UV, F_U, F_VV, F_V, F_1,          // omega * (u, v, 1)(u, v, 1)^T
    F_AUU, F_AUV, F_AVV, F_AU, F_AV,          // ... * u'
    F_BUU, F_BUV, F_BVV, F_BU, F_BV,          // ... * v'
    F_QUU, F_QUV, F_QVV,                      // omega * (u'^2 + v'^2) * (u, v)(u, v)^T
    F_R0, F_R1, F_R2, F_R3, F_R4, F_R5,       // omega * (u, v, 1) * du, ... * dv
    F_R6, F_R7                                // omega * (u, v) * (u' du + v' dv)
};

struct fit_lds {
    double part[kFitWaves][kFitSums];
    double m[8][8];   // the system, then its Cholesky factor in the lower triangle
    double r[8];      // right-hand side, then y, then g
    double g[8];
    double share;
    int status;
};

__global__ void __launch_bounds__(kFitThreads) k_flow_homography(const float* __restrict__ flow, double* __restrict__ Hout,
                                                                 double* __restrict__ stats, int w, int h, int iters,
                                                                 double c0_sq, double cmin_sq)
{
    __shared__ fit_lds L;
    const int n = w * h;
    const float* __restrict__ fx = flow + (size_t)blockIdx.x * 2 * n;
    const float* __restrict__ fy = fx + n;
    const double s = 2.0 / (double)max(w, h), cx = (double)(w - 1) / 2.0, cy = (double)(h - 1) / 2.0;
    const double s2 = s * s;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int step_y = kFitThreads / w, step_x = kFitThreads - step_y * w;
    const int y_first = (int)threadIdx.x / w, x_first = (int)threadIdx.x - y_first * w;

    double g0 = 0, g1 = 0, g2 = 0, g3 = 0, g4 = 0, g5 = 0, g6 = 0, g7 = 0;
    int status = 0;
    for (int k = 0; k < iters; ++k) {
        const double c2 = k > 0 ? fmax(cmin_sq, ldexp(c0_sq, -(k - 1))) : 1.0;
        double a[kFitSums];
#pragma unroll
        for (int j = 0; j < kFitSums; ++j) a[j] = 0.0;
        int x = x_first, y = y_first;
        for (int i = threadIdx.x; i < n; i += kFitThreads) {
            const float dxf = fx[i], dyf = fy[i];
            const bool valid = isfinite(dxf) && isfinite(dyf);
            const double u = ((double)x - cx) * s, v = ((double)y - cy) * s;
            const double du = valid ? (double)dxf * s : 0.0, dv = valid ? (double)dyf * s : 0.0;
            const double up = u + du, vp = v + dv;
            double om = valid ? 1.0 : 0.0;
            if (k > 0) {  // Tukey's biweight of the transfer error of the last solution, in pixels
                const double X = u + ((g0 * u + g1 * v) + g2), Y = v + ((g3 * u + g4 * v) + g5), D = 1.0 + (g6 * u + g7 * v);
                const double ex = X / D - up, ey = Y / D - vp;
                const double e2 = (ex * ex + ey * ey) / s2;
                const double t = 1.0 - e2 / c2;
                om = valid && t > 0.0 ? t * t : 0.0;  // a NaN or infinite e2 fails t > 0
            }
            const double wu = om * u, wv = om * v;
            const double tuu = wu * u, tuv = wu * v, tvv = wv * v;
            const double q = up * up + vp * vp, z = up * du + vp * dv;
            a[F_UU] += tuu, a[F_UV] += tuv, a[F_U] += wu, a[F_VV] += tvv, a[F_V] += wv, a[F_1] += om;
            a[F_AUU] += tuu * up, a[F_AUV] += tuv * up, a[F_AVV] += tvv * up, a[F_AU] += wu * up, a[F_AV] += wv * up;
            a[F_BUU] += tuu * vp, a[F_BUV] += tuv * vp, a[F_BVV] += tvv * vp, a[F_BU] += wu * vp, a[F_BV] += wv * vp;
            a[F_QUU] += tuu * q, a[F_QUV] += tuv * q, a[F_QVV] += tvv * q;
            a[F_R0] += wu * du, a[F_R1] += wv * du, a[F_R2] += om * du;
            a[F_R3] += wu * dv, a[F_R4] += wv * dv, a[F_R5] += om * dv;
            a[F_R6] += wu * z, a[F_R7] += wv * z;
            x += step_x, y += step_y;
            if (x >= w) x -= w, ++y;
        }
#pragma unroll
        for (int j = 0; j < kFitSums; ++j) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) a[j] += __shfl_down(a[j], off, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < kFitSums; ++j) L.part[wave][j] = a[j];
        }
        __syncthreads();
        if (wave == 0) {  // every lane of wave 0 does the same arithmetic on the same LDS words
            double t[kFitSums];
#pragma unroll
            for (int j = 0; j < kFitSums; ++j) {
                t[j] = L.part[0][j];
#pragma unroll
                for (int q = 1; q < kFitWaves; ++q) t[j] += L.part[q][j];
            }
            for (int i = 0; i < 8; ++i)
                for (int j = 0; j < 8; ++j) L.m[i][j] = 0.0;
            for (int b = 0; b < 6; b += 3) {  // the two (u, v, 1) blocks and their couplings to (g6, g7)
                L.m[b][b] = t[F_UU];
                L.m[b + 1][b] = t[F_UV], L.m[b + 1][b + 1] = t[F_VV];
                L.m[b + 2][b] = t[F_U], L.m[b + 2][b + 1] = t[F_V], L.m[b + 2][b + 2] = t[F_1];
            }
            L.m[6][0] = -t[F_AUU], L.m[6][1] = -t[F_AUV], L.m[6][2] = -t[F_AU];
            L.m[7][0] = -t[F_AUV], L.m[7][1] = -t[F_AVV], L.m[7][2] = -t[F_AV];
            L.m[6][3] = -t[F_BUU], L.m[6][4] = -t[F_BUV], L.m[6][5] = -t[F_BU];
            L.m[7][3] = -t[F_BUV], L.m[7][4] = -t[F_BVV], L.m[7][5] = -t[F_BV];
            L.m[6][6] = t[F_QUU], L.m[7][6] = t[F_QUV], L.m[7][7] = t[F_QVV];
            L.r[0] = t[F_R0], L.r[1] = t[F_R1], L.r[2] = t[F_R2], L.r[3] = t[F_R3], L.r[4] = t[F_R4], L.r[5] = t[F_R5];
            L.r[6] = -t[F_R6], L.r[7] = -t[F_R7];
            L.share = t[F_1] / ((double)w * (double)h);
            double top = L.m[0][0];
            for (int i = 1; i < 8; ++i) top = fmax(top, L.m[i][i]);
            const double floor_ = top * 0x1p-40;
            int bad = 0;  // degenerate: a pivot that is not finite or not above the floor (a NaN anywhere ends in one)
            for (int j = 0; j < 8; ++j) {  // Cholesky, column by column; only the lower triangle is read
                double d = L.m[j][j];
                for (int q = 0; q < j; ++q) d -= L.m[j][q] * L.m[j][q];
                if (!(isfinite(d) && d > floor_)) bad = 1;
                const double p = sqrt(bad ? 1.0 : d);
                L.m[j][j] = p;
                for (int i = j + 1; i < 8; ++i) {
                    double e = L.m[i][j];
                    for (int q = 0; q < j; ++q) e -= L.m[i][q] * L.m[j][q];
                    L.m[i][j] = e / p;
                }
            }
            for (int i = 0; i < 8; ++i) {  // L y = r
                double e = L.r[i];
                for (int q = 0; q < i; ++q) e -= L.m[i][q] * L.r[q];
                L.r[i] = e / L.m[i][i];
            }
            for (int i = 7; i >= 0; --i) {  // L^T g = y
                double e = L.r[i];
                for (int q = i + 1; q < 8; ++q) e -= L.m[q][i] * L.r[q];
                L.r[i] = e / L.m[i][i];
            }
            for (int i = 0; i < 8; ++i) L.g[i] = bad ? 0.0 : L.r[i];
            L.status = bad;
        }
        __syncthreads();
        g0 = L.g[0], g1 = L.g[1], g2 = L.g[2], g3 = L.g[3], g4 = L.g[4], g5 = L.g[5], g6 = L.g[6], g7 = L.g[7];
        status = __builtin_amdgcn_readfirstlane(L.status);
        if (status) break;  // degenerate: H = I (a wave-uniform exit: every wave reads the same LDS word)
    }
    if (threadIdx.x == 0) {
        // H = T^-1 (I + G) T, T = (s 0 -cx s; 0 s -cy s; 0 0 1), divided by its [2][2] entry
        const double a00 = 1.0 + g0, a01 = g1, a02 = g2, a10 = g3, a11 = 1.0 + g4, a12 = g5, a20 = g6, a21 = g7, a22 = 1.0;
        const double b00 = a00 * s, b01 = a01 * s, b02 = a02 - (a00 * cx + a01 * cy) * s;
        const double b10 = a10 * s, b11 = a11 * s, b12 = a12 - (a10 * cx + a11 * cy) * s;
        const double b20 = a20 * s, b21 = a21 * s, b22 = a22 - (a20 * cx + a21 * cy) * s;
        const double h00 = b00 / s + cx * b20, h01 = b01 / s + cx * b21, h02 = b02 / s + cx * b22;
        const double h10 = b10 / s + cy * b20, h11 = b11 / s + cy * b21, h12 = b12 / s + cy * b22;
        double* __restrict__ H = Hout + (size_t)blockIdx.x * 9;
        if (status) {
            H[0] = 1.0, H[1] = 0.0, H[2] = 0.0, H[3] = 0.0, H[4] = 1.0, H[5] = 0.0, H[6] = 0.0, H[7] = 0.0, H[8] = 1.0;
        } else {
            H[0] = h00 / b22, H[1] = h01 / b22, H[2] = h02 / b22;
            H[3] = h10 / b22, H[4] = h11 / b22, H[5] = h12 / b22;
            H[6] = b20 / b22, H[7] = b21 / b22, H[8] = b22 / b22;
        }
        stats[2 * (size_t)blockIdx.x] = L.share;
        stats[2 * (size_t)blockIdx.x + 1] = (double)status;
    }
}

// S22: flow f32 [N][2][h][w] -> out of the same shape (out == flow: in place).  Block (blockIdx.x, blockIdx.y = field);
// each thread owns kCompPx consecutive pixels.  The camera's displacement of pixel (x, y) under H is evaluated in double,
// left to right and without fused multiply-adds, rounded to float once and subtracted in float32.
// vec4 bit 0: 16-byte aligned out and planes of a multiple of 4 floats (one 16-byte store per component); bit 1: the same
// for flow (one 16-byte load).
constexpr int kCompThreads = 256;
constexpr int kCompPx = 4;

__global__ void __launch_bounds__(kCompThreads) k_flow_compensate(const float* flow, const double* __restrict__ Hin, float* out,
                                                                  int w, int h, int vec4)
{
    const int n = w * h;
    const int i0 = (blockIdx.x * kCompThreads + threadIdx.x) * kCompPx;
    if (i0 >= n) return;
    const double* __restrict__ H = Hin + (size_t)blockIdx.y * 9;
    const double h00 = H[0], h01 = H[1], h02 = H[2], h10 = H[3], h11 = H[4], h12 = H[5], h20 = H[6], h21 = H[7], h22 = H[8];
    const float* fx = flow + (size_t)blockIdx.y * 2 * n;
    const float* fy = fx + n;
    float dx[kCompPx], dy[kCompPx];
    if (vec4 & 2) {
        const f32x4 vx = *reinterpret_cast<const f32x4*>(fx + i0), vy = *reinterpret_cast<const f32x4*>(fy + i0);
#pragma unroll
        for (int j = 0; j < kCompPx; ++j) dx[j] = vx[j], dy[j] = vy[j];
    } else {
#pragma unroll
        for (int j = 0; j < kCompPx; ++j) {
            dx[j] = i0 + j < n ? fx[i0 + j] : 0.0f;
            dy[j] = i0 + j < n ? fy[i0 + j] : 0.0f;
        }
    }
    int y = i0 / w, x = i0 - y * w;
    float ox[kCompPx], oy[kCompPx];
#pragma unroll
    for (int j = 0; j < kCompPx; ++j) {
        const double xd = (double)x, yd = (double)y;
        const double X = h00 * xd + h01 * yd + h02, Y = h10 * xd + h11 * yd + h12, D = h20 * xd + h21 * yd + h22;
        const float cxf = (float)(X / D - xd), cyf = (float)(Y / D - yd);
        ox[j] = dx[j] - cxf;
        oy[j] = dy[j] - cyf;
        if (++x == w) x = 0, ++y;
    }
    float* ox_dst = out + (size_t)blockIdx.y * 2 * n;
    float* oy_dst = ox_dst + n;
    if (vec4 & 1) {
        *reinterpret_cast<f32x4*>(ox_dst + i0) = f32x4{ox[0], ox[1], ox[2], ox[3]};
        *reinterpret_cast<f32x4*>(oy_dst + i0) = f32x4{oy[0], oy[1], oy[2], oy[3]};
    } else {
#pragma unroll
        for (int j = 0; j < kCompPx; ++j)
            if (i0 + j < n) ox_dst[i0 + j] = ox[j], oy_dst[i0 + j] = oy[j];
    }
}

// S53: frames [n_seq][fps][h][w] (u8 or f32, TV-L1's input) -> pairs f32 [N][2][h][w], N = n_seq * (fps - 1), TV-L1 input
// again: plane 0 of pair n = s * (fps - 1) + k is frame k of sequence s as float, plane 1 is frame k + 1 resampled at
// H[n] (x, y, 1)^T, so that the camera's motion between the two planes is gone.  Block (blockIdx.x, blockIdx.y = pair);
// each thread owns kWarpPx consecutive pixels.  The position is evaluated as S22 evaluates it (double, left to right, no
// fused multiply-add), the blend is S17's (float32, no fmaf), and a pixel whose position is not inside the frame (D <= 0
// and NaN included) keeps frame k's own value: no evidence, no residual motion.  A gather: no atomics, no workspace.
// vec bit 0: 16-byte aligned pairs and planes of a multiple of 4 pixels (one 16-byte store per plane); bit 1: the same for
// the frames (one 16-byte load of frame k for f32, one 4-byte load for u8, which needs 4-byte alignment only).
constexpr int kWarpThreads = 256;
constexpr int kWarpPx = 4;

template <typename T>
__global__ void __launch_bounds__(kWarpThreads) k_frames_warp_pairs(const T* __restrict__ frames, const double* __restrict__ Hin,
                                                                    float* __restrict__ pairs, int w, int h, int fps, int vec)
{
    typedef T Tx4 __attribute__((ext_vector_type(4)));
    const int n = w * h;
    const int i0 = (blockIdx.x * kWarpThreads + threadIdx.x) * kWarpPx;
    if (i0 >= n) return;
    const int pair = blockIdx.y;
    const int s = pair / (fps - 1), k = pair - s * (fps - 1);
    const T* __restrict__ fa = frames + ((size_t)s * fps + k) * n;  // frame k
    const T* __restrict__ fb = fa + n;                              // frame k + 1
    const double* __restrict__ H = Hin + (size_t)pair * 9;
    const double h00 = H[0], h01 = H[1], h02 = H[2], h10 = H[3], h11 = H[4], h12 = H[5], h20 = H[6], h21 = H[7], h22 = H[8];
    float own[kWarpPx];
    if (vec & 2) {
        const Tx4 v = *reinterpret_cast<const Tx4*>(fa + i0);
#pragma unroll
        for (int j = 0; j < kWarpPx; ++j) own[j] = (float)v[j];
    } else {
#pragma unroll
        for (int j = 0; j < kWarpPx; ++j) own[j] = i0 + j < n ? (float)fa[i0 + j] : 0.0f;
    }
    const double xmax = (double)(w - 1), ymax = (double)(h - 1);
    int y = i0 / w, x = i0 - y * w;
    float val[kWarpPx];
#pragma unroll
    for (int j = 0; j < kWarpPx; ++j) {
        const double xd = (double)x, yd = (double)y;
        const double X = h00 * xd + h01 * yd + h02, Y = h10 * xd + h11 * yd + h12, D = h20 * xd + h21 * yd + h22;
        const double px = X / D, py = Y / D;
        const bool inside = D > 0.0 && px >= 0.0 && px <= xmax && py >= 0.0 && py <= ymax;  // a NaN fails every comparison
        const double pxs = inside ? px : 0.0, pys = inside ? py : 0.0;                     // the taps stay in the frame
        const double fx0 = floor(pxs), fy0 = floor(pys);
        const float ax = (float)(pxs - fx0), ay = (float)(pys - fy0);
        const int x0 = (int)fx0, y0 = (int)fy0;
        const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
        const T* r0 = fb + (size_t)y0 * w;
        const T* r1 = fb + (size_t)y1 * w;
        const float a = (float)r0[x0], b = (float)r0[x1], c = (float)r1[x0], d = (float)r1[x1];
        const float top = a + ax * (b - a);
        const float bot = c + ax * (d - c);
        val[j] = inside ? top + ay * (bot - top) : own[j];
        if (++x == w) x = 0, ++y;
    }
    float* p0 = pairs + (size_t)pair * 2 * n;
    float* p1 = p0 + n;
    if (vec & 1) {
        *reinterpret_cast<f32x4*>(p0 + i0) = f32x4{own[0], own[1], own[2], own[3]};
        *reinterpret_cast<f32x4*>(p1 + i0) = f32x4{val[0], val[1], val[2], val[3]};
    } else {
#pragma unroll
        for (int j = 0; j < kWarpPx; ++j)
            if (i0 + j < n) p0[i0 + j] = own[j], p1[i0 + j] = val[j];
    }
}

static constexpr int kMaxGridY = 65535;
static constexpr long long kMaxPlane = 0x7fffffffLL - 3 * kCompThreads * kCompPx;  // w*h and i0 + 3 stay in int

extern "C" int va_flow_homography(va_ctx* ctx, const void* flow, int n_fields, int w, int h, int iters, double c0_sq,
                                  double cmin_sq, void* H, void* stats, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_flow_homography: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(flow != nullptr && H != nullptr && stats != nullptr, "va_flow_homography: NULL buffer");
    VA_CHECK_ARG(n_fields >= 1 && w >= 1 && h >= 1, "va_flow_homography: bad shape");
    VA_CHECK_ARG(iters >= 1 && iters <= kFitMaxIters, "va_flow_homography: iters must be in 1..%d, got %d", kFitMaxIters, iters);
    VA_CHECK_ARG(cmin_sq > 0.0 && cmin_sq <= c0_sq && c0_sq < 1e300,
                 "va_flow_homography: need 0 < c_min^2 <= c_0^2 (finite), got %g and %g", cmin_sq, c0_sq);
    VA_CHECK_ARG((long long)w * h <= kMaxPlane, "va_flow_homography: %dx%d planes exceed one launch", w, h);
    k_flow_homography<<<(unsigned)n_fields, kFitThreads, 0, (hipStream_t)stream>>>((const float*)flow, (double*)H, (double*)stats,
                                                                                  w, h, iters, c0_sq, cmin_sq);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_flow_compensate(va_ctx* ctx, const void* flow, int n_fields, int w, int h, const void* H, void* out,
                                  void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_flow_compensate: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(flow != nullptr && H != nullptr && out != nullptr, "va_flow_compensate: NULL buffer");
    VA_CHECK_ARG(n_fields >= 1 && w >= 1 && h >= 1, "va_flow_compensate: bad shape");
    VA_CHECK_ARG(n_fields <= kMaxGridY, "va_flow_compensate: %d fields exceed %d per call", n_fields, kMaxGridY);
    VA_CHECK_ARG((long long)w * h <= kMaxPlane, "va_flow_compensate: %dx%d planes exceed one launch", w, h);
    const int n = w * h;
    const uintptr_t f0 = reinterpret_cast<uintptr_t>(flow), o0 = reinterpret_cast<uintptr_t>(out);
    const uintptr_t bytes = (uintptr_t)n_fields * 2 * n * sizeof(float);
    VA_CHECK_ARG(f0 == o0 || f0 + bytes <= o0 || o0 + bytes <= f0,
                 "va_flow_compensate: out must be the flow buffer itself or must not overlap it");
    const int vec4 = (n % 4 == 0 && o0 % 16 == 0 ? 1 : 0) | (n % 4 == 0 && f0 % 16 == 0 ? 2 : 0);
    const dim3 g((unsigned)va_cdiv(n, kCompThreads * kCompPx), (unsigned)n_fields);
    k_flow_compensate<<<g, kCompThreads, 0, (hipStream_t)stream>>>((const float*)flow, (const double*)H, (float*)out, w, h, vec4);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_frames_warp_pairs(va_ctx* ctx, const void* frames, int frames_are_u8, int n_seq, int frames_per_seq, int w,
                                    int h, const void* H, void* pairs, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_frames_warp_pairs: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(frames != nullptr && H != nullptr && pairs != nullptr, "va_frames_warp_pairs: NULL buffer");
    VA_CHECK_ARG(frames_are_u8 == 0 || frames_are_u8 == 1, "va_frames_warp_pairs: frames_are_u8 must be 0 or 1");
    VA_CHECK_ARG(n_seq >= 1 && frames_per_seq >= 2 && w >= 1 && h >= 1,
                 "va_frames_warp_pairs: bad shape (a sequence holds at least two frames)");
    const long long n_pairs = (long long)n_seq * (frames_per_seq - 1);
    VA_CHECK_ARG(n_pairs <= kMaxGridY, "va_frames_warp_pairs: %lld pairs exceed %d per call", n_pairs, kMaxGridY);
    VA_CHECK_ARG((long long)w * h <= kMaxPlane, "va_frames_warp_pairs: %dx%d planes exceed one launch", w, h);
    const int n = w * h;
    const size_t elem = frames_are_u8 ? 1 : sizeof(float);
    const uintptr_t f0 = reinterpret_cast<uintptr_t>(frames), o0 = reinterpret_cast<uintptr_t>(pairs);
    const uintptr_t fbytes = (uintptr_t)n_seq * frames_per_seq * n * elem, obytes = (uintptr_t)n_pairs * 2 * n * sizeof(float);
    VA_CHECK_ARG(f0 + fbytes <= o0 || o0 + obytes <= f0, "va_frames_warp_pairs: pairs must not overlap the frames");
    const int vec = (n % 4 == 0 && o0 % 16 == 0 ? 1 : 0) | (n % 4 == 0 && f0 % (4 * elem) == 0 ? 2 : 0);
    const dim3 g((unsigned)va_cdiv(n, kWarpThreads * kWarpPx), (unsigned)n_pairs);
    if (frames_are_u8)
        k_frames_warp_pairs<unsigned char><<<g, kWarpThreads, 0, (hipStream_t)stream>>>(
            (const unsigned char*)frames, (const double*)H, (float*)pairs, w, h, frames_per_seq, vec);
    else
        k_frames_warp_pairs<float><<<g, kWarpThreads, 0, (hipStream_t)stream>>>((const float*)frames, (const double*)H,
                                                                                (float*)pairs, w, h, frames_per_seq, vec);
    VA_LAUNCH_CHECK();
    return VA_OK;
}
