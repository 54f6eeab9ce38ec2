// Kernel SVMs on the device: the chi-square and linear Gram matrices, Laptev's normaliser, the
// exponential combine, and a one-vs-rest fit over any positive semi-definite Gram matrix K.
//
// The fit keeps linear_svm_fit's model (svm.hip): L2-regularised squared hinge, regularised bias s.  With Kt = K + s^2 and
// H = Kt + I / (2C), class row r (y_i = +1 where label i is the row's class, else -1) has the dual
//
//   min over alpha >= 0 of  1/2 alpha^T ((y y^T) o H) alpha - e^T alpha,    beta = y alpha,  intercept = s^2 sum_i beta_i.
//
// The vectors of the solver are stored class-major, [rows][n].  Every product H V runs on v_mfma_f64_16x16x4_f64 for all rows at
// once (operand layout: v4d in va_feature_device.h); H is never formed: s^2 and the diagonal are added as K is read.  Every sum
// has a fixed order, there are no atomics: the result is a function of the inputs alone.
#include "va_feature_device.h"

namespace {

constexpr int kKsvmCgSteps = 100;   // CG steps enqueued per outer step (a row whose CG has converged skips the rest)
constexpr int kKsvmLsTrials = 40;   // halvings of the step length tried before the step is refused
constexpr double kKsvmArmijo = 1e-4;
constexpr int kKsvmMaxRows = 16384, kKsvmMaxClasses = 1024;
constexpr int kGramMaxDim = 65536, kGramMaxRows = 1 << 20, kGramMaxChunk = 32;
constexpr int kKsvmMaxChannels = VA_CHI2_MAX_CHANNELS;
constexpr size_t kCombineMaxCount = (size_t)1 << 38;  // 2^30 workgroups of 256 lanes: inside what one grid's x extent holds
constexpr int kKsvmFields = VA_KSVM_FIT_FIELDS;

// ---- Gram matrices

// D[i][j] = sum_k (x[i][k] - y[j][k])^2 / (x[i][k] + y[j][k]) over k = c0 .. c1-1 in ascending order, one accumulator per
// result, a term whose denominator is 0 counted as 0; every operation is an IEEE float64 one (no contraction), so the sum can
// be restated bit for bit.  A workgroup computes 64 x 64 results, a lane the 4 x 4 of them at rows ty + 16a, columns tx + 16b;
// `chunk` columns of both operands are staged in LDS at a time, [k][row], which changes no bit.  sym: y == x, only the tiles
// on and above the diagonal are computed and every result above the diagonal is written to its mirror place as well.
template <typename T>
__global__ void __launch_bounds__(256) k_chi2_distance(const T* __restrict__ x, const T* __restrict__ y, int m, int n, int d, int c0, int c1,
                                                       int chunk, int sym, double* __restrict__ out)
{
    __shared__ double xs[kGramMaxChunk][65], ys[kGramMaxChunk][65];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (sym && bj < bi) return;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i0 = bi * 64, j0 = bj * 64;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int k0 = c0; k0 < c1; k0 += chunk) {
        const int kc = min(chunk, c1 - k0);
        __syncthreads();
        for (int e = threadIdx.x; e < 64 * kc; e += 256) {
            const int r = e / kc, kk = e - r * kc;
            xs[kk][r] = (double)x[(size_t)min(i0 + r, m - 1) * d + k0 + kk];
            ys[kk][r] = (double)y[(size_t)min(j0 + r, n - 1) * d + k0 + kk];
        }
        __syncthreads();
        for (int kk = 0; kk < kc; ++kk) {
            double xv[4], yv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) xv[a] = xs[kk][ty + 16 * a];
#pragma unroll
            for (int b = 0; b < 4; ++b) yv[b] = ys[kk][tx + 16 * b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const double df = xv[a] - yv[b];
                    const double sm = xv[a] + yv[b];
                    const double term = (df * df) / sm;
                    acc[a][b] = acc[a][b] + (sm == 0.0 ? 0.0 : term);
                }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            if (i >= m || j >= n || (sym && i > j)) continue;
            out[(size_t)i * n + j] = acc[a][b];
            if (sym && i < j) out[(size_t)j * n + i] = acc[a][b];
        }
}

// G[i][j] = sum_k x[i][k] y[j][k] on the float64 MFMA: a workgroup computes 64 x 64 results, wave w the rows 16w .. 16w+15.
// k is walked 16 at a time; lane (q = lane>>4) reads the values k0 + 4q .. k0 + 4q + 3 of its row of x and of y and feeds value
// s to MFMA number s of the group, as k_svm_fwd does.  sym: as k_chi2_distance.
template <typename T>
__global__ void __launch_bounds__(256) k_linear_gram(const T* __restrict__ x, const T* __restrict__ y, int m, int n, int d, int sym,
                                                     double* __restrict__ out)
{
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (sym && bj < bi) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
    const int rowbase = bi * 64 + wave * 16, j0 = bj * 64;
    const T* __restrict__ xr = x + (size_t)min(rowbase + r16, m - 1) * d;
    const T* yr[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) yr[t] = y + (size_t)min(j0 + 16 * t + r16, n - 1) * d;
    v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < d; k0 += 16) {
        const int kb = k0 + 4 * q;
        double a[4], b[4][4];
        if (k0 + 16 <= d) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                a[s] = (double)xr[kb + s];
#pragma unroll
                for (int t = 0; t < 4; ++t) b[t][s] = (double)yr[t][kb + s];
            }
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = kb + s, kl = min(k, d - 1);
                a[s] = k < d ? (double)xr[kl] : 0.0;
#pragma unroll
                for (int t = 0; t < 4; ++t) b[t][s] = k < d ? (double)yr[t][kl] : 0.0;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[t][s], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int i = rowbase + q + 4 * reg, j = j0 + 16 * t + r16;
            if (i >= m || j >= n || (sym && i > j)) continue;
            out[(size_t)i * n + j] = acc[t][reg];
            if (sym && i < j) out[(size_t)j * n + i] = acc[t][reg];
        }
}

// rowsum[i] = sum_{j > i} D[i][j]: lane l adds j = i + 1 + l, i + 1 + l + 256, ... in ascending order, then va_wg_sum256
__global__ void __launch_bounds__(256) k_upper_rowsum(const double* __restrict__ D, int n, double* __restrict__ rowsum)
{
    __shared__ double red[4];
    const int i = blockIdx.x;
    double acc = 0.0;
    for (int j = i + 1 + threadIdx.x; j < n; j += 256) acc = acc + D[(size_t)i * n + j];
    acc = va_wg_sum256(acc, red);
    if (threadIdx.x == 0) rowsum[i] = acc;
}

// out[0] = (sum_i rowsum[i]) / (n (n - 1) / 2): lane l adds i = l, l + 256, ... in ascending order, then va_wg_sum256
__global__ void __launch_bounds__(256) k_upper_mean(const double* __restrict__ rowsum, int n, double* __restrict__ out)
{
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc = acc + rowsum[i];
    acc = va_wg_sum256(acc, red);
    if (threadIdx.x == 0) out[0] = acc / (0.5 * (double)n * (double)(n - 1));
}

struct KsvmChannels {
    const double* d[kKsvmMaxChannels];
    double w[kKsvmMaxChannels];
};

// K = exp(-(w_0 D_0 + w_1 D_1 + ...)), the products added in channel order
__global__ void __launch_bounds__(256) k_chi2_combine(KsvmChannels ch, int nch, size_t count, double* __restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    double acc = ch.w[0] * ch.d[0][e];
    for (int c = 1; c < nch; ++c) acc = acc + ch.w[c] * ch.d[c][e];
    out[e] = exp(-acc);
}

// ---- the fit

// out[j][i] = sum_k V[j][k] H[k][i], H = K + s2 + diag I (H is symmetric: its column i is read as row i of K): a workgroup
// computes 64 class rows x 64 columns i, wave w the columns 16w .. 16w+15 (A = V, B = H, so a lane's results are contiguous in
// i).  k is walked 16 at a time as in k_linear_gram.  MASKED: out = mask[j][i] ? out : 0, every class row's own face.
template <bool MASKED>
__global__ void __launch_bounds__(256) k_ksvm_prod(const double* __restrict__ K, int n, double s2, double diag, int c,
                                                   const double* __restrict__ V, const int* __restrict__ flags, const int* __restrict__ mask,
                                                   double* __restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
    const int j0 = blockIdx.y * 64;
    if (!va_tile_is_live(flags, j0, c, lane)) return;
    const int ibase = blockIdx.x * 64 + wave * 16;
    const int ic = min(ibase + r16, n - 1);
    const double* __restrict__ kr = K + (size_t)ic * n;
    const double* vr[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) vr[t] = V + (size_t)min(j0 + 16 * t + r16, c - 1) * n;
    v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < n; k0 += 16) {
        const int kb = k0 + 4 * q;
        double a[4][4], b[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = kb + s, kl = min(k, n - 1);
            const double h = (kr[kl] + s2) + (k == ic ? diag : 0.0);
            b[s] = k < n ? h : 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t) a[t][s] = k < n ? vr[t][kl] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t][s], b[s], acc[t], 0, 0, 0);
    }
    const int i = ibase + r16;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int j = j0 + 16 * t + q + 4 * reg;
            if (j >= c || i >= n) continue;
            const size_t idx = (size_t)j * n + i;
            out[idx] = (!MASKED || mask[idx]) ? acc[t][reg] : 0.0;
        }
}

struct KsvmState {
    double *B, *HB, *BC, *Z, *X, *R, *P, *HP, *Q;           // [c][n]
    int* free;                                              // [c][n]
    double *q, *pgn, *nsv, *steps, *rr, *cgtol, *cgs, *ref;  // [c]
    int *live, *notdone, *tight;                            // [c]
};

__global__ void __launch_bounds__(256) k_ksvm_init(KsvmState s, int c, int n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)c * n) {
        s.B[i] = s.HB[i] = s.BC[i] = s.Z[i] = s.X[i] = s.R[i] = s.P[i] = s.HP[i] = s.Q[i] = 0.0;
        s.free[i] = 0;
    }
    if (i < (size_t)c) {
        s.q[i] = s.pgn[i] = s.nsv[i] = s.steps[i] = s.rr[i] = s.cgtol[i] = s.cgs[i] = s.ref[i] = 0.0;
        s.live[i] = s.tight[i] = 0;
        s.notdone[i] = 1;
    }
}

// After HB = H B, one workgroup per class row: f = Kt B = HB - B / (2C), the violators V = {1 - y f > 0} (the row's face, kept
// in `free`), the feasible candidate BC = B on V where y B > 0 and exactly 0 elsewhere, and ref = |B - 2C y max(0, 1 - y f)| /
// (2C), the size of the Newton system's right-hand side.
__global__ void __launch_bounds__(256) k_ksvm_face(KsvmState s, const int* __restrict__ lab, int n, int pos_off, double C)
{
    __shared__ double red[4];
    const int r = blockIdx.x;
    if (!s.notdone[r]) return;
    const size_t base = (size_t)r * n;
    const double twoC = 2.0 * C;
    double dd = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double y = lab[i] == r + pos_off ? 1.0 : -1.0;
        const double b = s.B[base + i];
        const double m = 1.0 - y * (s.HB[base + i] - b / twoC);
        const bool sv = m > 0.0;
        s.free[base + i] = sv ? 1 : 0;
        s.BC[base + i] = (sv && y * b > 0.0) ? b : 0.0;
        const double diff = b - (sv ? twoC * y * m : 0.0);
        dd = dd + diff * diff;
    }
    dd = va_wg_sum256(dd, red);
    if (threadIdx.x == 0) s.ref[r] = sqrt(dd) / twoC;
}

// After Z = H BC: the dual's gradient g = y Z - 1 at the candidate, its projected norm, the stop rule |pg| <= tol sqrt(n), the
// support-vector count and the dual objective; a row that goes on starts its CG at X = BC with R = P = (y - Z) on the face and
// the forcing term min(0.1, sqrt(ref / sqrt(n))) (0 after a refused step), never below tol sqrt(n) / 4.  A row that has stopped
// is never touched again.
__global__ void __launch_bounds__(256) k_ksvm_grad(KsvmState s, const int* __restrict__ lab, int n, int pos_off, double tol)
{
    __shared__ double red[4];
    const int r = blockIdx.x;
    if (!s.notdone[r]) return;
    const size_t base = (size_t)r * n;
    double pp = 0.0, rs = 0.0, cnt = 0.0, qq = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double y = lab[i] == r + pos_off ? 1.0 : -1.0;
        const double z = s.Z[base + i], bc = s.BC[base + i];
        const double g = y * z - 1.0;
        const double pg = y * bc > 0.0 ? g : fmin(g, 0.0);
        const double res = s.free[base + i] ? y - z : 0.0;
        s.R[base + i] = res;
        s.P[base + i] = res;
        s.X[base + i] = bc;
        pp = pp + pg * pg;
        rs = rs + res * res;
        cnt = cnt + (bc != 0.0 ? 1.0 : 0.0);
        qq = qq + bc * (0.5 * z - y);
    }
    pp = va_wg_sum256(pp, red);
    rs = va_wg_sum256(rs, red);
    cnt = va_wg_sum256(cnt, red);
    qq = va_wg_sum256(qq, red);
    if (threadIdx.x == 0) {
        const double rootn = sqrt((double)n), pgn = sqrt(pp), ref = s.ref[r];
        const int go_on = pgn <= tol * rootn ? 0 : 1;
        const double eta = s.tight[r] ? 0.0 : fmin(0.1, sqrt(ref / rootn));
        const double cgtol = fmax(eta * ref, 0.25 * tol * rootn);
        s.q[r] = qq;
        s.pgn[r] = pgn;
        s.nsv[r] = cnt;
        s.rr[r] = rs;
        s.cgtol[r] = cgtol;
        s.notdone[r] = go_on;
        s.live[r] = (go_on && sqrt(rs) > cgtol) ? 1 : 0;
    }
}

// After HP = H P on the face, one CG step of every row whose CG is live: alpha = rr / P.HP, X += alpha P, R -= alpha HP;
// |R| <= cgtol ends the row's CG, else P = R + (|R|^2 / rr) P.
__global__ void __launch_bounds__(256) k_ksvm_cg(KsvmState s, int n)
{
    __shared__ double red[4];
    const int r = blockIdx.x;
    if (!s.live[r]) return;
    const size_t base = (size_t)r * n;
    const double rr = s.rr[r], cgtol = s.cgtol[r];
    double php = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) php = php + s.P[base + i] * s.HP[base + i];
    php = va_wg_sum256(php, red);
    if (!(php > 0.0)) {  // P = 0 or not finite: the solution found so far is the step's target
        if (threadIdx.x == 0) s.live[r] = 0;
        return;
    }
    const double alpha = rr / php;
    double rn = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        s.X[base + i] = s.X[base + i] + alpha * s.P[base + i];
        const double res = s.R[base + i] - alpha * s.HP[base + i];
        s.R[base + i] = res;
        rn = rn + res * res;
    }
    rn = va_wg_sum256(rn, red);
    if (threadIdx.x == 0) s.cgs[r] = s.cgs[r] + 1.0;
    if (sqrt(rn) <= cgtol) {
        if (threadIdx.x == 0) s.live[r] = 0;
        return;
    }
    const double beta = rn / rr;
    for (int i = threadIdx.x; i < n; i += 256) s.P[base + i] = s.R[base + i] + beta * s.P[base + i];
    if (threadIdx.x == 0) s.rr[r] = rn;
}

// The step S = X - B of every row that has not stopped, kept in X
__global__ void __launch_bounds__(256) k_ksvm_dir(KsvmState s, int n)
{
    const int r = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (!s.notdone[r] || i >= n) return;
    const size_t idx = (size_t)r * n + i;
    s.X[idx] = s.X[idx] - s.B[idx];
}

// After Q = H S, the line search of every row that has not stopped, with no further product: with KS = Q - S / (2C) the
// function values at B + t S are f + t KS.  t = 1, 1/2, 1/4, ... until P(B + tS) - P(B) <= 1e-4 t slope, where P(B) = 1/2 B.Kt B
// + C sum max(0, 1 - y f)^2 is the primal objective written in B, slope = KS.(B - 2C y h(0)) its derivative along S and the
// difference is summed term by term, t B.KS + t^2/2 S.KS + C sum_i (h_i(t) - h_i(0)) (h_i(t) + h_i(0)).  Then B += t S; a refused
// step sets `tight`, which makes the next CG exact.
__global__ void __launch_bounds__(256) k_ksvm_ls(KsvmState s, const int* __restrict__ lab, int n, int pos_off, double C)
{
    __shared__ double red[4];
    const int r = blockIdx.x;
    if (!s.notdone[r]) return;
    const size_t base = (size_t)r * n;
    const double twoC = 2.0 * C;
    double sl = 0.0, bks = 0.0, sks = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double y = lab[i] == r + pos_off ? 1.0 : -1.0;
        const double b = s.B[base + i], sv = s.X[base + i];
        const double ks = s.Q[base + i] - sv / twoC;
        const double h0 = fmax(0.0, 1.0 - y * (s.HB[base + i] - b / twoC));
        sl = sl + ks * (b - twoC * y * h0);
        bks = bks + b * ks;
        sks = sks + sv * ks;
    }
    sl = va_wg_sum256(sl, red);
    bks = va_wg_sum256(bks, red);
    sks = va_wg_sum256(sks, red);
    double t = 1.0;
    bool found = false;
    if (sl < 0.0) {
        for (int trial = 0; trial < kKsvmLsTrials; ++trial) {
            double acc = 0.0;
            for (int i = threadIdx.x; i < n; i += 256) {
                const double y = lab[i] == r + pos_off ? 1.0 : -1.0;
                const double b = s.B[base + i], sv = s.X[base + i];
                const double ks = s.Q[base + i] - sv / twoC;
                const double f = s.HB[base + i] - b / twoC;
                const double h0 = fmax(0.0, 1.0 - y * f);
                const double ht = fmax(0.0, 1.0 - y * (f + t * ks));
                acc = acc + (ht - h0) * (ht + h0);
            }
            acc = va_wg_sum256(acc, red);
            const double delta = t * bks + 0.5 * t * t * sks + C * acc;
            if (delta <= kKsvmArmijo * t * sl) {
                found = true;
                break;
            }
            t = 0.5 * t;
        }
    }
    if (threadIdx.x == 0) s.tight[r] = found ? 0 : 1;
    if (!found) return;  // step length 0
    for (int i = threadIdx.x; i < n; i += 256) s.B[base + i] = s.B[base + i] + t * s.X[base + i];
    if (threadIdx.x == 0) s.steps[r] = s.steps[r] + 1.0;
}

__global__ void __launch_bounds__(256) k_ksvm_export(KsvmState s, int n, double s2, double* __restrict__ dual_coef,
                                                     double* __restrict__ intercept, double* __restrict__ stats)
{
    __shared__ double red[4];
    const int r = blockIdx.x;
    const size_t base = (size_t)r * n;
    double sum = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double bc = s.BC[base + i];
        dual_coef[base + i] = bc;
        sum = sum + bc;
    }
    sum = va_wg_sum256(sum, red);
    if (threadIdx.x == 0) {
        intercept[r] = s2 * sum;
        stats[5 * r + 0] = s.q[r];
        stats[5 * r + 1] = s.pgn[r];
        stats[5 * r + 2] = s.nsv[r];
        stats[5 * r + 3] = s.steps[r];
        stats[5 * r + 4] = s.cgs[r];
    }
}

// The workspace, in order: nine [c][n] vectors, the [c][n] face, eight [c] scalars, three [c] flags; every part starts on a
// 256-byte boundary.
size_t ksvm_layout(int n, int c, char* base, KsvmState* st)
{
    va_carver ws{base};
    KsvmState s;
    double** vec[9] = {&s.B, &s.HB, &s.BC, &s.Z, &s.X, &s.R, &s.P, &s.HP, &s.Q};
    for (double** v : vec) *v = ws.take<double>((size_t)c * n);
    s.free = ws.take<int>((size_t)c * n);
    double** sca[8] = {&s.q, &s.pgn, &s.nsv, &s.steps, &s.rr, &s.cgtol, &s.cgs, &s.ref};
    for (double** v : sca) *v = ws.take<double>((size_t)c);
    s.live = ws.take<int>((size_t)c);
    s.notdone = ws.take<int>((size_t)c);
    s.tight = ws.take<int>((size_t)c);
    if (st) *st = s;
    return ws.off;
}

bool ksvm_sizes_ok(int n, int rows)
{
    if (n < 2 || n > kKsvmMaxRows || rows < 1 || rows == 2 || rows > kKsvmMaxClasses) {
        va_set_error("va_kernel_svm_fit: need 2 <= n <= %d, n_class_rows 1 or 3 .. %d (got %d, %d)", kKsvmMaxRows, kKsvmMaxClasses, n, rows);
        return false;
    }
    return true;
}

bool ksvm_finite(double v) { return v - v == 0.0; }

// One problem's launch geometry and state: what every phase of the fit's loop needs.  The launches exist in this one copy;
// va_kernel_svm_fit and va_kernel_svm_fit_phase both enqueue them through it.
struct KsvmRun {
    const double* K;
    const int* lab;
    int n, c, pos_off;
    double C, s2, diag, tol;
    KsvmState s;
    hipStream_t st;
    dim3 gprod;

    void prod(const double* V, const int* flags, double* out) const
    {
        k_ksvm_prod<false><<<gprod, 256, 0, st>>>(K, n, s2, diag, c, V, flags, nullptr, out);
    }
    void init() const { k_ksvm_init<<<(unsigned)(((size_t)c * n + 255) / 256), 256, 0, st>>>(s, c, n); }
    // the face and the candidate at B, its projected gradient, the stop rule, and the start of the next CG
    void eval() const
    {
        prod(s.B, s.notdone, s.HB);
        k_ksvm_face<<<c, 256, 0, st>>>(s, lab, n, pos_off, C);
        prod(s.BC, s.notdone, s.Z);
        k_ksvm_grad<<<c, 256, 0, st>>>(s, lab, n, pos_off, tol);
    }
    void cg(int rounds) const
    {
        for (int it = 0; it < rounds; ++it) {
            k_ksvm_prod<true><<<gprod, 256, 0, st>>>(K, n, s2, diag, c, s.P, s.live, s.free, s.HP);
            k_ksvm_cg<<<c, 256, 0, st>>>(s, n);
        }
    }
    void line_search() const
    {
        k_ksvm_dir<<<dim3(va_cdiv(n, 256), c), 256, 0, st>>>(s, n);
        prod(s.X, s.notdone, s.Q);
        k_ksvm_ls<<<c, 256, 0, st>>>(s, lab, n, pos_off, C);
    }
};

// The argument checks va_kernel_svm_fit and va_kernel_svm_fit_phase share; fills `run` when they pass.
int ksvm_prepare(const void* k, const void* y, int n, int n_classes, double C, double intercept_scaling, double tol, void* workspace,
                 size_t workspace_bytes, void* stream, KsvmRun* run)
{
    VA_CHECK_ARG(n_classes >= 2 && n_classes <= kKsvmMaxClasses, "va_kernel_svm_fit: need 2 <= n_classes <= %d (got %d)", kKsvmMaxClasses,
                 n_classes);
    const int c = n_classes == 2 ? 1 : n_classes, pos_off = n_classes == 2 ? 1 : 0;
    if (!ksvm_sizes_ok(n, c)) return VA_ERR_INVALID;
    VA_CHECK_ARG(ksvm_finite(C) && C > 0.0, "va_kernel_svm_fit: C must be finite and > 0 (got %g)", C);
    VA_CHECK_ARG(ksvm_finite(tol) && tol > 0.0, "va_kernel_svm_fit: tol must be finite and > 0 (got %g)", tol);
    VA_CHECK_ARG(ksvm_finite(intercept_scaling) && intercept_scaling >= 0.0,
                 "va_kernel_svm_fit: intercept_scaling must be finite and >= 0 (got %g)", intercept_scaling);
    KsvmRun r;
    r.K = (const double*)k;
    r.lab = (const int*)y;
    r.n = n, r.c = c, r.pos_off = pos_off;
    r.C = C, r.s2 = intercept_scaling * intercept_scaling, r.diag = 1.0 / (2.0 * C), r.tol = tol;
    r.st = (hipStream_t)stream;
    r.gprod = dim3(va_cdiv(n, 64), va_cdiv(c, 64));
    const size_t need = ksvm_layout(n, c, (char*)workspace, &r.s);
    if (workspace_bytes < need) {
        va_set_error("va_kernel_svm_fit: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return VA_ERR_WORKSPACE;
    }
    VA_CHECK_ARG(((size_t)workspace & 7) == 0, "va_kernel_svm_fit: workspace must be 8-byte aligned");
    *run = r;
    return VA_OK;
}

int gram_check(const char* who, const void* x, const void* out, int m, int n, int d, bool sym)
{
    VA_CHECK_ARG(x && out, "%s: NULL pointer", who);
    VA_CHECK_ARG(m >= 1 && m <= kGramMaxRows && (sym || (n >= 1 && n <= kGramMaxRows)) && d >= 1 && d <= kGramMaxDim,
                 "%s: need 1 <= m, n <= %d rows and 1 <= d <= %d columns (got %d, %d, %d)", who, kGramMaxRows, kGramMaxDim, m, n, d);
    return VA_OK;
}

}  // namespace

extern "C" int va_chi2_distance(va_ctx* ctx, const void* x, const void* y, int m, int n, int d, int c0, int c1, int x_is_f64, int chunk,
                                void* out, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_chi2_distance: ctx is NULL");
    VA_USE_DEVICE(ctx);
    const bool sym = y == nullptr;
    const int rc = gram_check("va_chi2_distance", x, out, m, n, d, sym);
    if (rc != VA_OK) return rc;
    VA_CHECK_ARG(0 <= c0 && c0 < c1 && c1 <= d, "va_chi2_distance: need 0 <= c0 < c1 <= d (got %d, %d, d = %d)", c0, c1, d);
    VA_CHECK_ARG(chunk == 0 || (chunk >= 1 && chunk <= kGramMaxChunk), "va_chi2_distance: chunk must be 0 or 1 .. %d (got %d)", kGramMaxChunk,
                 chunk);
    VA_CHECK_ARG(x_is_f64 == 0 || x_is_f64 == 1, "va_chi2_distance: x_is_f64 must be 0 or 1 (got %d)", x_is_f64);
    const int cols = sym ? m : n, ck = chunk == 0 ? 16 : chunk;
    const dim3 grid(va_cdiv(cols, 64), va_cdiv(m, 64));
    if (x_is_f64)
        k_chi2_distance<double><<<grid, 256, 0, (hipStream_t)stream>>>((const double*)x, (const double*)(sym ? x : y), m, cols, d, c0, c1, ck, sym,
                                                                       (double*)out);
    else
        k_chi2_distance<float><<<grid, 256, 0, (hipStream_t)stream>>>((const float*)x, (const float*)(sym ? x : y), m, cols, d, c0, c1, ck, sym,
                                                                      (double*)out);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_linear_gram(va_ctx* ctx, const void* x, const void* y, int m, int n, int d, int x_is_f64, void* out, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_linear_gram: ctx is NULL");
    VA_USE_DEVICE(ctx);
    const bool sym = y == nullptr;
    const int rc = gram_check("va_linear_gram", x, out, m, n, d, sym);
    if (rc != VA_OK) return rc;
    VA_CHECK_ARG(x_is_f64 == 0 || x_is_f64 == 1, "va_linear_gram: x_is_f64 must be 0 or 1 (got %d)", x_is_f64);
    const int cols = sym ? m : n;
    const dim3 grid(va_cdiv(cols, 64), va_cdiv(m, 64));
    if (x_is_f64)
        k_linear_gram<double><<<grid, 256, 0, (hipStream_t)stream>>>((const double*)x, (const double*)(sym ? x : y), m, cols, d, sym, (double*)out);
    else
        k_linear_gram<float><<<grid, 256, 0, (hipStream_t)stream>>>((const float*)x, (const float*)(sym ? x : y), m, cols, d, sym, (double*)out);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_upper_mean(va_ctx* ctx, const void* dist, int n, void* rowsum, void* mean, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_upper_mean: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(dist && rowsum && mean, "va_upper_mean: NULL pointer");
    VA_CHECK_ARG(n >= 2 && n <= kGramMaxRows, "va_upper_mean: need 2 <= n <= %d (got %d)", kGramMaxRows, n);
    k_upper_rowsum<<<n, 256, 0, (hipStream_t)stream>>>((const double*)dist, n, (double*)rowsum);
    VA_LAUNCH_CHECK();
    k_upper_mean<<<1, 256, 0, (hipStream_t)stream>>>((const double*)rowsum, n, (double*)mean);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_chi2_combine(va_ctx* ctx, const void* const* dist, const double* weights, int n_channels, size_t count, void* out,
                               void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_chi2_combine: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(dist && weights && out, "va_chi2_combine: NULL pointer");
    VA_CHECK_ARG(n_channels >= 1 && n_channels <= kKsvmMaxChannels, "va_chi2_combine: need 1 <= n_channels <= %d (got %d)", kKsvmMaxChannels,
                 n_channels);
    VA_CHECK_ARG(count >= 1 && count <= kCombineMaxCount, "va_chi2_combine: need 1 <= count <= %zu elements (got %zu)", kCombineMaxCount, count);
    KsvmChannels ch = {};
    for (int c = 0; c < n_channels; ++c) {
        VA_CHECK_ARG(dist[c] != nullptr, "va_chi2_combine: dist[%d] is NULL", c);
        VA_CHECK_ARG(ksvm_finite(weights[c]) && weights[c] >= 0.0, "va_chi2_combine: need finite weights >= 0 (weights[%d] = %g)", c, weights[c]);
        ch.d[c] = (const double*)dist[c];
        ch.w[c] = weights[c];
    }
    k_chi2_combine<<<(unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream>>>(ch, n_channels, count, (double*)out);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" size_t va_kernel_svm_fit_workspace_bytes(int n, int n_class_rows)
{
    if (!ksvm_sizes_ok(n, n_class_rows)) return 0;
    return ksvm_layout(n, n_class_rows, nullptr, nullptr);
}

extern "C" int va_kernel_svm_fit(va_ctx* ctx, const void* k, const void* y, int n, int n_classes, double C, double intercept_scaling,
                                 double tol, int outer_iters, int restart, void* dual_coef, void* intercept, void* stats, void* workspace,
                                 size_t workspace_bytes, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_kernel_svm_fit: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(k && y && dual_coef && intercept && stats && workspace, "va_kernel_svm_fit: NULL pointer");
    VA_CHECK_ARG(outer_iters >= 0 && outer_iters <= 1000, "va_kernel_svm_fit: need 0 <= outer_iters <= 1000 (got %d)", outer_iters);
    VA_CHECK_ARG(restart == 0 || restart == 1, "va_kernel_svm_fit: restart must be 0 or 1 (got %d)", restart);
    KsvmRun run;
    const int rc = ksvm_prepare(k, y, n, n_classes, C, intercept_scaling, tol, workspace, workspace_bytes, stream, &run);
    if (rc != VA_OK) return rc;
    if (restart) {
        run.init();
        run.eval();
        VA_LAUNCH_CHECK();
    }
    for (int it = 0; it < outer_iters; ++it) {
        run.cg(kKsvmCgSteps);
        run.line_search();
        run.eval();
        VA_LAUNCH_CHECK();
    }
    k_ksvm_export<<<run.c, 256, 0, run.st>>>(run.s, n, run.s2, (double*)dual_coef, (double*)intercept, (double*)stats);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" size_t va_kernel_svm_fit_layout(int n, int n_class_rows, size_t* offsets, int count)
{
    if (!ksvm_sizes_ok(n, n_class_rows)) return 0;
    if (offsets == nullptr || count != kKsvmFields) {
        va_set_error("va_kernel_svm_fit_layout: offsets must hold exactly %d fields (got %s, count %d)", kKsvmFields,
                     offsets ? "a pointer" : "NULL", count);
        return 0;
    }
    KsvmState s;
    const size_t total = ksvm_layout(n, n_class_rows, nullptr, &s);
    const void* field[kKsvmFields] = {s.B, s.HB, s.BC, s.Z, s.X, s.R, s.P, s.HP, s.Q, s.free, s.q, s.pgn, s.nsv, s.steps,
                                      s.rr, s.cgtol, s.cgs, s.ref, s.live, s.notdone, s.tight};
    for (int i = 0; i < kKsvmFields; ++i) offsets[i] = (size_t)(uintptr_t)field[i];
    return total;
}

extern "C" int va_kernel_svm_fit_phase(va_ctx* ctx, const void* k, const void* y, int n, int n_classes, double C, double intercept_scaling,
                                       double tol, int phase, int count, void* workspace, size_t workspace_bytes, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_kernel_svm_fit_phase: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(k && y && workspace, "va_kernel_svm_fit_phase: NULL pointer");
    VA_CHECK_ARG(phase >= VA_KSVM_PHASE_INIT && phase <= VA_KSVM_PHASE_LINE_SEARCH, "va_kernel_svm_fit_phase: unknown phase %d", phase);
    VA_CHECK_ARG(phase != VA_KSVM_PHASE_CG || (count >= 1 && count <= kKsvmCgSteps),
                 "va_kernel_svm_fit_phase: the CG phase needs 1 <= count <= %d (got %d)", kKsvmCgSteps, count);
    KsvmRun run;
    const int rc = ksvm_prepare(k, y, n, n_classes, C, intercept_scaling, tol, workspace, workspace_bytes, stream, &run);
    if (rc != VA_OK) return rc;
    switch (phase) {
    case VA_KSVM_PHASE_INIT: run.init(); break;
    case VA_KSVM_PHASE_EVAL: run.eval(); break;
    case VA_KSVM_PHASE_CG: run.cg(count); break;
    default: run.line_search(); break;
    }
    VA_LAUNCH_CHECK();
    return VA_OK;
}
