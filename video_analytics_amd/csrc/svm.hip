// Fitting the fusion SVM on the device: LinearSVC()'s problem, liblinear's L2R_L2LOSS_SVC posed
// one-vs-rest, solved by a primal Newton-CG in float64 with every class row advanced together.
//
//   f_r(w) = 1/2 |w|^2 + C sum_i max(0, 1 - y_i w.[x_i, s])^2,   y_i = +1 where label i is class r, else -1
//
// The vectors of the solver (iterate W, gradient G, Newton direction S, CG residual R and direction P, H P) are stored
// class-major, [rows][D] with D = dim + 1: row r is [coef_r, intercept_r / s].  The homogeneous column s is supplied by the
// product kernels; X is never copied.  With s = 0 the last coordinate has gradient W[D-1] = 0 and stays 0.
//
// Both products run on v_mfma_f64_16x16x4_f64 (operand layout: v4d in va_feature_device.h).  Every sum has a fixed order, there
// are no atomics: the result is a function of the inputs alone.
#include "va_feature_device.h"

namespace {

constexpr int kSvmCgSteps = 100;    // CG steps enqueued per Newton step (a class whose CG has converged skips the rest)
constexpr int kSvmChunkRows = 256;  // rows of X per partial sum of the transposed product
constexpr int kSvmLsTrials = 40;    // halvings of the step length tried before the step is refused
constexpr double kSvmArmijo = 1e-4;

enum { SVM_EVAL = 0, SVM_CG = 1, SVM_LS = 2 };

// out[i][j] = sum_k Xh[i][k] P[j][k], Xh = [X, s]: a workgroup computes 64 rows x 64 class rows, wave w rows 16w .. 16w+15.
// k is walked 16 at a time; lane (q = lane>>4) reads the four consecutive values k0 + 4q .. k0 + 4q + 3 of its row of X and
// of P and feeds value s to MFMA number s of the group (both operands agree on the assignment, so the products are those of
// the sum; the order of the additions is fixed).  Fused epilogues:
//   SVM_EVAL: M = out, U = active ? M - y : 0 (active: 1 - y M > 0), losspart[row block][j] = sum over the block's rows of
//             the squared hinge, rows ascending within a lane, then lane groups, then waves.
//   SVM_CG:   U = active(M) ? out : 0.
//   SVM_LS:   Q = out.
template <int MODE>
__global__ void __launch_bounds__(256) k_svm_fwd(const double* __restrict__ X, const int* __restrict__ lab, int n, int d, double sc, int c,
                                                 int pos_off, const double* __restrict__ P, const int* __restrict__ flags,
                                                 double* __restrict__ M, double* __restrict__ U, double* __restrict__ Q,
                                                 double* __restrict__ losspart)
{
    __shared__ double red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
    const int c0 = blockIdx.y * 64;
    if (!va_tile_is_live(flags, c0, c, lane)) return;
    const int D = d + 1;
    const int rowbase = blockIdx.x * 64 + wave * 16;
    const double* __restrict__ xr = X + (size_t)min(rowbase + r16, n - 1) * d;
    const double* pr[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) pr[t] = P + (size_t)min(c0 + 16 * t + r16, c - 1) * D;
    v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < D; k0 += 16) {
        const int kb = k0 + 4 * q;
        double a[4], b[4][4];
        if (k0 + 16 <= d) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                a[s] = xr[kb + s];
#pragma unroll
                for (int t = 0; t < 4; ++t) b[t][s] = pr[t][kb + s];
            }
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = kb + s;
                a[s] = k < d ? xr[k] : (k == d ? sc : 0.0);
#pragma unroll
                for (int t = 0; t < 4; ++t) b[t][s] = pr[t][min(k, d)];
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[t][s], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = c0 + 16 * t + r16;
        double lsum = 0.0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = rowbase + q + 4 * reg;
            const bool ok = col < c && row < n;
            const size_t idx = (size_t)row * c + col;
            const double o = acc[t][reg];
            if (MODE == SVM_LS) {
                if (ok) Q[idx] = o;
            } else {
                const double y = ok && lab[row] == col + pos_off ? 1.0 : -1.0;
                const double m = MODE == SVM_EVAL ? o : (ok ? M[idx] : 0.0);
                const double h = 1.0 - y * m;
                const bool act = h > 0.0;
                if (ok) {
                    if (MODE == SVM_EVAL) {
                        M[idx] = o;
                        U[idx] = act ? o - y : 0.0;
                        lsum = lsum + (act ? h * h : 0.0);
                    } else {
                        U[idx] = act ? o : 0.0;
                    }
                }
            }
        }
        if (MODE == SVM_EVAL) {
            lsum = lsum + __shfl_xor(lsum, 16, 64);
            lsum = lsum + __shfl_xor(lsum, 32, 64);
            if (q == 0) red[wave][16 * t + r16] = lsum;
        }
    }
    if (MODE == SVM_EVAL) {
        __syncthreads();
        const int col = c0 + threadIdx.x;
        if (threadIdx.x < 64 && col < c)
            losspart[(size_t)blockIdx.x * c + col] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    }
}

// Stage one of Xh^T U, reduced over the rows of one chunk: part[chunk][j][k] = sum_{i in chunk} U[i][j] Xh[i][k], i ascending
// four at a time.  A workgroup computes 64 class rows x 64 columns k, wave w the columns 16w .. 16w+15 (A = U^T, B = Xh, so a
// lane's results are contiguous in k).  Stage two, the sum over the chunks in ascending order, is in the per-class kernels.
__global__ void __launch_bounds__(256) k_svm_xtu(const double* __restrict__ X, int n, int d, double sc, int c, const double* __restrict__ U,
                                                 const int* __restrict__ flags, double* __restrict__ part)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r16 = lane & 15;
    const int j0 = blockIdx.y * 64;
    const int D = d + 1;
    const int kbase = blockIdx.z * 64 + wave * 16;
    if (kbase >= D) return;
    if (!va_tile_is_live(flags, j0, c, lane)) return;
    const int k = kbase + r16;
    const int i_beg = blockIdx.x * kSvmChunkRows, i_end = min(i_beg + kSvmChunkRows, n);
    int jl[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) jl[t] = min(j0 + 16 * t + r16, c - 1);
    v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int i0 = i_beg; i0 < i_end; i0 += 4) {
        const int i = i0 + q;
        const int il = min(i, i_end - 1);
        double b = k < d ? X[(size_t)il * d + k] : (k == d ? sc : 0.0);
        if (i >= i_end) b = 0.0;
        const double* __restrict__ ur = U + (size_t)il * c;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ur[jl[t]], b, acc[t], 0, 0, 0);
    }
    if (k >= D) return;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int j = j0 + 16 * t + q + 4 * reg;
            if (j < c) part[((size_t)blockIdx.x * c + j) * D + k] = acc[t][reg];
        }
}

struct SvmState {
    double *W, *G, *S, *R, *P, *HP;        // [c][D]
    double *M, *U, *Q;                     // [n][c]
    double* part;                          // [chunks][c][D]
    double* losspart;                      // [row blocks][c]
    double *f, *gn, *g0, *steps, *rr, *cgtol, *cgs;  // [c]
    int *live, *notdone;                   // [c]
};

__global__ void __launch_bounds__(256) k_svm_init(SvmState s, int c, int D)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)c * D) s.W[i] = s.G[i] = s.S[i] = s.R[i] = s.P[i] = s.HP[i] = 0.0;
    if (i < (size_t)c) {
        s.f[i] = s.gn[i] = s.g0[i] = s.steps[i] = s.rr[i] = s.cgtol[i] = s.cgs[i] = 0.0;
        s.live[i] = 0;
        s.notdone[i] = 1;
    }
}

// After SVM_EVAL and k_svm_xtu, one workgroup per class row: G = W + 2C sum_chunks part, f, |G|; the stop rule
// |G| <= tol |G(0)| (first = 1: this is G(0)); a class that goes on starts its CG at S = 0, R = P = -G with the forcing term
// min(0.1, sqrt(|G| / |G(0)|)).  A class that has stopped is never touched again.
__global__ void __launch_bounds__(256) k_svm_cls_grad(SvmState s, int c, int D, int chunks, int row_blocks, double C, double tol, int first)
{
    __shared__ double red[4];
    const int r = blockIdx.x;
    if (!s.notdone[r]) return;
    const size_t base = (size_t)r * D;
    double ww = 0.0, gg = 0.0, ls = 0.0;
    for (int k = threadIdx.x; k < D; k += 256) {
        const double w = s.W[base + k];
        const double g = w + 2.0 * C * va_strided_sum(s.part, chunks, (size_t)c * D, base + k);
        s.G[base + k] = g;
        s.S[base + k] = 0.0;
        s.R[base + k] = -g;
        s.P[base + k] = -g;
        ww = ww + w * w;
        gg = gg + g * g;
    }
    for (int b = threadIdx.x; b < row_blocks; b += 256) ls = ls + s.losspart[(size_t)b * c + r];
    ww = va_wg_sum256(ww, red);
    gg = va_wg_sum256(gg, red);
    ls = va_wg_sum256(ls, red);
    if (threadIdx.x == 0) {
        const double gn = sqrt(gg);
        const double g0 = first ? gn : s.g0[r];
        const int go_on = gn <= tol * g0 ? 0 : 1;
        s.f[r] = 0.5 * ww + C * ls;
        s.gn[r] = gn;
        s.g0[r] = g0;
        s.rr[r] = gg;
        s.cgtol[r] = fmin(0.1, sqrt(gn / g0)) * gn;
        s.notdone[r] = go_on;
        s.live[r] = go_on;
    }
}

// After SVM_CG and k_svm_xtu, one CG step of every class whose CG is live: HP = P + 2C sum_chunks part, alpha = rr / P.HP,
// S += alpha P, R -= alpha HP; |R| <= cgtol ends the class's CG, else beta = |R|^2 / rr and P = R + beta P.
__global__ void __launch_bounds__(256) k_svm_cls_cg(SvmState s, int c, int D, int chunks, double C)
{
    __shared__ double red[4];
    const int r = blockIdx.x;
    if (!s.live[r]) return;
    const size_t base = (size_t)r * D;
    const double rr = s.rr[r], cgtol = s.cgtol[r];
    double php = 0.0;
    for (int k = threadIdx.x; k < D; k += 256) {
        const double p = s.P[base + k];
        const double hp = p + 2.0 * C * va_strided_sum(s.part, chunks, (size_t)c * D, base + k);
        s.HP[base + k] = hp;
        php = php + p * hp;
    }
    php = va_wg_sum256(php, red);
    if (!(php > 0.0)) {  // P = 0 or not finite: the direction found so far is the step
        if (threadIdx.x == 0) s.live[r] = 0;
        return;
    }
    const double alpha = rr / php;
    double rn = 0.0;
    for (int k = threadIdx.x; k < D; k += 256) {
        s.S[base + k] = s.S[base + k] + alpha * s.P[base + k];
        const double res = s.R[base + k] - alpha * s.HP[base + k];
        s.R[base + k] = res;
        rn = rn + res * res;
    }
    rn = va_wg_sum256(rn, red);
    if (threadIdx.x == 0) s.cgs[r] = s.cgs[r] + 1.0;
    if (sqrt(rn) <= cgtol) {
        if (threadIdx.x == 0) s.live[r] = 0;
        return;
    }
    const double beta = rn / rr;
    for (int k = threadIdx.x; k < D; k += 256) s.P[base + k] = s.R[base + k] + beta * s.P[base + k];
    if (threadIdx.x == 0) s.rr[r] = rn;
}

// After SVM_LS (Q = Xh S), the line search of every class that has not stopped, with no further product: the margins at
// W + t S are M + t Q.  t = 1, 1/2, 1/4, ... until f(W + tS) - f(W) <= 1e-4 t G.S, the difference summed term by term,
//   t W.S + t^2/2 S.S + C sum_i (h_i(t) - h_i(0)) (h_i(t) + h_i(0)),   h_i(t) = max(0, 1 - y_i (M_i + t Q_i)),
// so that it keeps its accuracy where f itself no longer changes in its leading digits.  Then W += t S.
__global__ void __launch_bounds__(256) k_svm_cls_ls(SvmState s, const int* __restrict__ lab, int n, int c, int D, int pos_off, double C)
{
    __shared__ double red[4];
    const int r = blockIdx.x;
    if (!s.notdone[r]) return;
    const size_t base = (size_t)r * D;
    double ws = 0.0, ss = 0.0, gs = 0.0;
    for (int k = threadIdx.x; k < D; k += 256) {
        const double sv = s.S[base + k];
        ws = ws + s.W[base + k] * sv;
        ss = ss + sv * sv;
        gs = gs + s.G[base + k] * sv;
    }
    ws = va_wg_sum256(ws, red);
    ss = va_wg_sum256(ss, red);
    gs = va_wg_sum256(gs, red);
    double t = 1.0;
    bool found = false;
    if (gs < 0.0) {
        for (int trial = 0; trial < kSvmLsTrials; ++trial) {
            double acc = 0.0;
            for (int i = threadIdx.x; i < n; i += 256) {
                const double y = lab[i] == r + pos_off ? 1.0 : -1.0;
                const double m = s.M[(size_t)i * c + r];
                const double h0 = fmax(0.0, 1.0 - y * m);
                const double ht = fmax(0.0, 1.0 - y * (m + t * s.Q[(size_t)i * c + r]));
                acc = acc + (ht - h0) * (ht + h0);
            }
            acc = va_wg_sum256(acc, red);
            const double delta = t * ws + 0.5 * t * t * ss + C * acc;
            if (delta <= kSvmArmijo * t * gs) {
                found = true;
                break;
            }
            t = 0.5 * t;
        }
    }
    if (!found) return;  // step length 0
    for (int k = threadIdx.x; k < D; k += 256) s.W[base + k] = s.W[base + k] + t * s.S[base + k];
    if (threadIdx.x == 0) s.steps[r] = s.steps[r] + 1.0;
}

__global__ void __launch_bounds__(256) k_svm_export(SvmState s, int d, double sc, double* __restrict__ coef, double* __restrict__ intercept,
                                                    double* __restrict__ stats)
{
    const int r = blockIdx.x;
    const size_t base = (size_t)r * (d + 1);
    for (int k = threadIdx.x; k < d; k += 256) coef[(size_t)r * d + k] = s.W[base + k];
    if (threadIdx.x == 0) {
        intercept[r] = sc * s.W[base + d];
        stats[4 * r + 0] = s.f[r];
        stats[4 * r + 1] = s.gn[r];
        stats[4 * r + 2] = s.g0[r];
        stats[4 * r + 3] = s.steps[r];
    }
}

__global__ void k_svm_cg_steps(SvmState s, int c, double* __restrict__ out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < c) out[r] = s.cgs[r];
}

constexpr int kSvmMaxDim = 8192, kSvmMaxClasses = 4096;
constexpr int kSvmFields = VA_SVM_FIT_FIELDS;  // the fields of SvmState, in svm_layout's order

// The workspace, in order: six [c][D] vectors, three [n][c] matrices, the partial sums of both reductions, seven [c] scalars,
// two [c] flags; every part starts on a 256-byte boundary.
size_t svm_layout(int n, int dim, int c, char* base, SvmState* st)
{
    const size_t D = (size_t)dim + 1;
    const size_t chunks = (size_t)va_cdiv(n, kSvmChunkRows), row_blocks = (size_t)va_cdiv(n, 64);
    va_carver ws{base};
    SvmState s;
    double** vec[6] = {&s.W, &s.G, &s.S, &s.R, &s.P, &s.HP};
    for (double** v : vec) *v = ws.take<double>((size_t)c * D);
    double** mat[3] = {&s.M, &s.U, &s.Q};
    for (double** m : mat) *m = ws.take<double>((size_t)n * c);
    s.part = ws.take<double>(chunks * c * D);
    s.losspart = ws.take<double>(row_blocks * c);
    double** sca[7] = {&s.f, &s.gn, &s.g0, &s.steps, &s.rr, &s.cgtol, &s.cgs};
    for (double** v : sca) *v = ws.take<double>((size_t)c);
    s.live = ws.take<int>((size_t)c);
    s.notdone = ws.take<int>((size_t)c);
    if (st) *st = s;
    return ws.off;
}

bool svm_sizes_ok(int n, int dim, int rows)
{
    if (n < 2 || dim < 1 || dim > kSvmMaxDim || rows < 1 || rows == 2 || rows > kSvmMaxClasses) {
        va_set_error("va_linear_svm_fit: need n >= 2, 1 <= dim <= %d, n_class_rows 1 or 3 .. %d (got %d, %d, %d)", kSvmMaxDim,
                     kSvmMaxClasses, n, dim, rows);
        return false;
    }
    return true;
}

bool svm_finite(double v) { return v - v == 0.0; }

}  // namespace

extern "C" size_t va_linear_svm_fit_workspace_bytes(int n, int dim, int n_class_rows)
{
    if (!svm_sizes_ok(n, dim, n_class_rows)) return 0;
    return svm_layout(n, dim, n_class_rows, nullptr, nullptr);
}

namespace {

// One problem's launch geometry and state: what every phase of the fit's loop needs.  The launches exist in this one copy;
// va_linear_svm_fit and va_linear_svm_fit_phase both enqueue them through it.
struct SvmRun {
    const double* X;
    const int* lab;
    int n, dim, c, pos_off, D, chunks, row_blocks;
    double C, sc, tol;
    SvmState s;
    hipStream_t st;
    dim3 gfwd, gxtu;

    void init() const { k_svm_init<<<(unsigned)(((size_t)c * D + 255) / 256), 256, 0, st>>>(s, c, D); }
    // margins, loss and gradient at W, the stop rule, and the start of the next CG
    void eval(int first) const
    {
        k_svm_fwd<SVM_EVAL><<<gfwd, 256, 0, st>>>(X, lab, n, dim, sc, c, pos_off, s.W, s.notdone, s.M, s.U, s.Q, s.losspart);
        k_svm_xtu<<<gxtu, 256, 0, st>>>(X, n, dim, sc, c, s.U, s.notdone, s.part);
        k_svm_cls_grad<<<c, 256, 0, st>>>(s, c, D, chunks, row_blocks, C, tol, first);
    }
    void cg(int rounds) const
    {
        for (int cg = 0; cg < rounds; ++cg) {
            k_svm_fwd<SVM_CG><<<gfwd, 256, 0, st>>>(X, lab, n, dim, sc, c, pos_off, s.P, s.live, s.M, s.U, s.Q, s.losspart);
            k_svm_xtu<<<gxtu, 256, 0, st>>>(X, n, dim, sc, c, s.U, s.live, s.part);
            k_svm_cls_cg<<<c, 256, 0, st>>>(s, c, D, chunks, C);
        }
    }
    void line_search() const
    {
        k_svm_fwd<SVM_LS><<<gfwd, 256, 0, st>>>(X, lab, n, dim, sc, c, pos_off, s.S, s.notdone, s.M, s.U, s.Q, s.losspart);
        k_svm_cls_ls<<<c, 256, 0, st>>>(s, lab, n, c, D, pos_off, C);
    }
};

// The argument checks va_linear_svm_fit and va_linear_svm_fit_phase share; fills `run` when they pass.
int svm_prepare(const void* x, const void* y, int n, int dim, int n_classes, double C, double intercept_scaling, double tol,
                void* workspace, size_t workspace_bytes, void* stream, SvmRun* run)
{
    VA_CHECK_ARG(n_classes >= 2 && n_classes <= kSvmMaxClasses, "va_linear_svm_fit: need 2 <= n_classes <= %d (got %d)", kSvmMaxClasses,
                 n_classes);
    const int c = n_classes == 2 ? 1 : n_classes, pos_off = n_classes == 2 ? 1 : 0;
    if (!svm_sizes_ok(n, dim, c)) return VA_ERR_INVALID;
    VA_CHECK_ARG(svm_finite(C) && C > 0.0, "va_linear_svm_fit: C must be finite and > 0 (got %g)", C);
    VA_CHECK_ARG(svm_finite(tol) && tol > 0.0, "va_linear_svm_fit: tol must be finite and > 0 (got %g)", tol);
    VA_CHECK_ARG(svm_finite(intercept_scaling) && intercept_scaling >= 0.0,
                 "va_linear_svm_fit: intercept_scaling must be finite and >= 0 (got %g)", intercept_scaling);
    SvmRun r;
    r.X = (const double*)x;
    r.lab = (const int*)y;
    r.n = n, r.dim = dim, r.c = c, r.pos_off = pos_off;
    r.D = dim + 1, r.chunks = va_cdiv(n, kSvmChunkRows), r.row_blocks = va_cdiv(n, 64);
    r.C = C, r.sc = intercept_scaling, r.tol = tol;
    r.st = (hipStream_t)stream;
    r.gfwd = dim3(r.row_blocks, va_cdiv(c, 64));
    r.gxtu = dim3(r.chunks, va_cdiv(c, 64), va_cdiv(r.D, 64));
    const size_t need = svm_layout(n, dim, c, (char*)workspace, &r.s);
    if (workspace_bytes < need) {
        va_set_error("va_linear_svm_fit: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return VA_ERR_WORKSPACE;
    }
    VA_CHECK_ARG(((size_t)workspace & 7) == 0, "va_linear_svm_fit: workspace must be 8-byte aligned");
    *run = r;
    return VA_OK;
}

}  // namespace

extern "C" int va_linear_svm_fit(va_ctx* ctx, const void* x, const void* y, int n, int dim, int n_classes, double C, double intercept_scaling,
                                 double tol, int newton_iters, int restart, void* coef, void* intercept, void* stats, void* workspace,
                                 size_t workspace_bytes, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_linear_svm_fit: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x && y && coef && intercept && stats && workspace, "va_linear_svm_fit: NULL pointer");
    VA_CHECK_ARG(newton_iters >= 0 && newton_iters <= 1000, "va_linear_svm_fit: need 0 <= newton_iters <= 1000 (got %d)", newton_iters);
    VA_CHECK_ARG(restart == 0 || restart == 1, "va_linear_svm_fit: restart must be 0 or 1 (got %d)", restart);
    SvmRun run;
    const int rc = svm_prepare(x, y, n, dim, n_classes, C, intercept_scaling, tol, workspace, workspace_bytes, stream, &run);
    if (rc != VA_OK) return rc;
    if (restart) {
        run.init();
        run.eval(1);
        VA_LAUNCH_CHECK();
    }
    for (int it = 0; it < newton_iters; ++it) {
        run.cg(kSvmCgSteps);
        run.line_search();
        run.eval(0);
        VA_LAUNCH_CHECK();
    }
    k_svm_export<<<run.c, 256, 0, run.st>>>(run.s, dim, run.sc, (double*)coef, (double*)intercept, (double*)stats);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" size_t va_linear_svm_fit_layout(int n, int dim, int n_class_rows, size_t* offsets, int count)
{
    if (!svm_sizes_ok(n, dim, n_class_rows)) return 0;
    if (offsets == nullptr || count != kSvmFields) {
        va_set_error("va_linear_svm_fit_layout: offsets must hold exactly %d fields (got %s, count %d)", kSvmFields,
                     offsets ? "a pointer" : "NULL", count);
        return 0;
    }
    SvmState s;
    const size_t total = svm_layout(n, dim, n_class_rows, nullptr, &s);
    const void* field[kSvmFields] = {s.W, s.G, s.S, s.R, s.P, s.HP, s.M, s.U, s.Q, s.part, s.losspart, s.f, s.gn, s.g0,
                                     s.steps, s.rr, s.cgtol, s.cgs, s.live, s.notdone};
    for (int i = 0; i < kSvmFields; ++i) offsets[i] = (size_t)(uintptr_t)field[i];
    return total;
}

extern "C" int va_linear_svm_fit_phase(va_ctx* ctx, const void* x, const void* y, int n, int dim, int n_classes, double C,
                                       double intercept_scaling, double tol, int phase, int count, void* workspace, size_t workspace_bytes,
                                       void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_linear_svm_fit_phase: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x && y && workspace, "va_linear_svm_fit_phase: NULL pointer");
    VA_CHECK_ARG(phase >= VA_SVM_PHASE_INIT && phase <= VA_SVM_PHASE_LINE_SEARCH, "va_linear_svm_fit_phase: unknown phase %d", phase);
    VA_CHECK_ARG(phase != VA_SVM_PHASE_CG || (count >= 1 && count <= kSvmCgSteps),
                 "va_linear_svm_fit_phase: the CG phase needs 1 <= count <= %d (got %d)", kSvmCgSteps, count);
    SvmRun run;
    const int rc = svm_prepare(x, y, n, dim, n_classes, C, intercept_scaling, tol, workspace, workspace_bytes, stream, &run);
    if (rc != VA_OK) return rc;
    switch (phase) {
    case VA_SVM_PHASE_INIT: run.init(); break;
    case VA_SVM_PHASE_EVAL_FIRST: run.eval(1); break;
    case VA_SVM_PHASE_EVAL: run.eval(0); break;
    case VA_SVM_PHASE_CG: run.cg(count); break;
    default: run.line_search(); break;
    }
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_linear_svm_fit_cg_steps(va_ctx* ctx, int n, int dim, int n_class_rows, const void* workspace, size_t workspace_bytes,
                                          void* cg_steps, void* stream)
{
    VA_CHECK_ARG(ctx != nullptr, "va_linear_svm_fit_cg_steps: ctx is NULL");
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(workspace && cg_steps, "va_linear_svm_fit_cg_steps: NULL pointer");
    if (!svm_sizes_ok(n, dim, n_class_rows)) return VA_ERR_INVALID;
    SvmState s;
    const size_t need = svm_layout(n, dim, n_class_rows, (char*)workspace, &s);
    if (workspace_bytes < need) {
        va_set_error("va_linear_svm_fit_cg_steps: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return VA_ERR_WORKSPACE;
    }
    k_svm_cg_steps<<<va_cdiv(n_class_rows, 256), 256, 0, (hipStream_t)stream>>>(s, n_class_rows, (double*)cg_steps);
    VA_LAUNCH_CHECK();
    return VA_OK;
}
