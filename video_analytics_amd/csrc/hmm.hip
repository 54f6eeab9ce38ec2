// HMM action segmentation on the device: the Gaussian emission table, batched Viterbi decoding, the scaled
// forward-backward pass and the Gaussian statistics of the modelled project's Sheet04.py (Kuehne, Arslan and Serre, CVPR 2014)
// -- its GrammarContext.getEmissionProbs (:242-252), its Viterbi (:520-560) and its BaumWelch and LearnGaussians (:284-513) --
// as thousands of independent (sequence, model) chains, one per workgroup.
//
// Everything is float64.  The emission sum runs over the columns in ascending order with one rounding per operation (the
// tree builds with -ffp-contract=off); Viterbi adds and compares only, which are exact, so a score and a path are the bits of
// the recursion as S99 writes it; every sum of the forward-backward pass and of the statistics has a written order.  There
// are no atomics.
#include "va_feature_device.h"

#include <climits>
#include <cmath>

namespace {

constexpr int kHmmMaxDim = 512, kHmmMaxStates = 1024;
constexpr int kWaveStates = 64;   // the single-wave form: a model of at most this many states ...
constexpr int kWaveEdges = 512;   // ... and this many edges, which then live in LDS
constexpr int kBtBlock = 16;      // frames of backpointers staged in LDS per step of the backtrack
constexpr int kWgThreads = 256;   // the workgroup form: 256 threads x 4 states
constexpr unsigned short kNoPred = 0xFFFF;

enum { HMM_OK = 0, HMM_NO_PATH = 1, HMM_NAN = 2, HMM_BAD_JOB = 3 };

// ---- S98 emissions --------------------------------------------------------------------------------------------------------

// logB[t][g] = c_g - 0.5 q, q = sum_d ((x_d - mu_gd) (x_d - mu_gd)) iv_gd, d ascending.  A workgroup makes 16 frames x 64
// Gaussians; the columns pass through LDS 32 at a time: the Gaussians' rows transposed (a lane reads its own Gaussian at
// consecutive doubles), the frames' rows as they are (every lane of a wave reads one address).  Thread (g = tid & 63,
// ty = tid >> 6) owns frames ty, ty + 4, ty + 8, ty + 12 of the tile.
constexpr int kEmG = 64, kEmT = 16, kEmD = 32, kEmGLd = kEmG + 1;
template <typename X>
__global__ void __launch_bounds__(256) k_hmm_emissions(const X* __restrict__ x, int t_total, int d, const double* __restrict__ mu,
                                                       const double* __restrict__ iv, const double* __restrict__ cst, int G,
                                                       double* __restrict__ logb)
{
    __shared__ double smu[kEmD * kEmGLd], siv[kEmD * kEmGLd], sx[kEmT * kEmD];
    const int tid = threadIdx.x, gl = tid & 63, ty = tid >> 6;
    const int g0 = blockIdx.x * kEmG;
    const long long t0 = (long long)blockIdx.y * kEmT;
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < d; c0 += kEmD) {
        __syncthreads();
        for (int i = tid; i < kEmG * kEmD; i += 256) {
            const int g = i / kEmD, c = i % kEmD;
            const bool in = g0 + g < G && c0 + c < d;
            smu[c * kEmGLd + g] = in ? mu[(size_t)(g0 + g) * d + c0 + c] : 0.0;
            siv[c * kEmGLd + g] = in ? iv[(size_t)(g0 + g) * d + c0 + c] : 0.0;
        }
        for (int i = tid; i < kEmT * kEmD; i += 256) {
            const int r = i / kEmD, c = i % kEmD;
            sx[i] = (t0 + r < t_total && c0 + c < d) ? (double)x[(size_t)(t0 + r) * d + c0 + c] : 0.0;
        }
        __syncthreads();
        const int cn = d - c0 < kEmD ? d - c0 : kEmD;
        for (int c = 0; c < cn; ++c) {
            const double m = smu[c * kEmGLd + gl], w = siv[c * kEmGLd + gl];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double df = sx[(ty + 4 * k) * kEmD + c] - m;
                const double sq = df * df;
                q[k] = q[k] + sq * w;
            }
        }
    }
    if (g0 + gl < G) {
        const double c = cst[g0 + gl];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long t = t0 + ty + 4 * k;
            if (t < t_total) logb[(size_t)t * G + g0 + gl] = c - 0.5 * q[k];
        }
    }
}

// ---- S99 Viterbi ----------------------------------------------------------------------------------------------------------

struct HmmBatch {
    const double* logb;     // [t_total][g]
    const int* seq_ptr;     // [n_seqs + 1] frames
    const int* state_ptr;   // [n_models + 1] into emit, log_pi, log_final; model m's pred_ptr starts at state_ptr[m] + m
    const int* edge_ptr;    // [n_models + 1] into pred_idx, pred_logp
    const int* emit;
    const int* pred_ptr;
    const int* pred_idx;
    const double* pred_logp;
    const double* log_pi;
    const double* log_final;
    const int* jobs;        // [n_jobs][3]: sequence, model, want_path
    const long long* path_off;
    const long long* bp_off;
    double* score;
    int* status;
    int* path;
    unsigned short* bp;
    long long path_elems, bp_elems;
    int t_total, g, n_seqs, n_models, n_states_total, n_edges_total;
    // forward-backward only (S100)
    const int* succ_ptr;    // rows like pred_ptr's: the successors of every state, ascending
    const int* succ_idx;
    const int* succ_edge;   // the edge's place in the model's pred_idx / pred_logp
    const double* edge_p;   // exp(pred_logp), exp(log_pi), exp(log_final): k_hmm_exp's
    const double* pi_p;
    const double* fin_p;
    const long long* gamma_off;
    const long long* xi_off;
    const long long* mc_off;
    double* gamma;
    double* xi;
    double* mc;             // per job and frame: (m_t, c_t)
    double* loglik;
    long long gamma_elems, xi_elems, mc_elems;
};

// The sizes of one job, and whether they stay inside the arrays of the call.
struct HmmJob {
    int s, m, want, N, E, T, s0, e0;
    long long f0;
};
__device__ __forceinline__ bool hmm_job_load(const HmmBatch& a, int job, HmmJob& j)
{
    j.s = a.jobs[3 * job], j.m = a.jobs[3 * job + 1], j.want = a.jobs[3 * job + 2];
    j.N = j.E = j.T = j.s0 = j.e0 = 0, j.f0 = 0;
    if (!(j.s >= 0 && j.s < a.n_seqs && j.m >= 0 && j.m < a.n_models)) return false;
    j.s0 = a.state_ptr[j.m], j.N = a.state_ptr[j.m + 1] - j.s0;
    j.e0 = a.edge_ptr[j.m], j.E = a.edge_ptr[j.m + 1] - j.e0;
    j.f0 = a.seq_ptr[j.s], j.T = a.seq_ptr[j.s + 1] - a.seq_ptr[j.s];
    return j.N >= 1 && j.N <= kHmmMaxStates && j.E >= 0 && j.T >= 1 && j.s0 >= 0 && j.s0 + j.N <= a.n_states_total && j.e0 >= 0 &&
           j.e0 + j.E <= a.n_edges_total && j.f0 >= 0 && j.f0 + j.T <= a.t_total;
}

// (value, index) of the larger value, the lower index where the values are equal
__device__ __forceinline__ void hmm_take_better(double& v, int& i, double v2, int i2)
{
    if (v2 > v || (v2 == v && i2 < i)) v = v2, i = i2;
}

// One (sequence, model) chain per workgroup.  THREADS = 64, SPT = 1 is the single-wave form: the workgroup is one wave, its
// barriers cost nothing and the model's edges sit in LDS.  THREADS = 256, SPT = 4 is the workgroup form up to 1024 states: the
// edges are read through the caches.  Both keep delta double-buffered in LDS with one barrier per frame, load logB a group
// of frames ahead, and write backpointers only for a job that wants its path.  Every branch around a barrier is uniform
// over the workgroup.
template <int THREADS, int SPT>
__global__ void __launch_bounds__(THREADS) k_hmm_viterbi(const HmmBatch a)
{
    constexpr bool kWave = THREADS == kWaveStates;
    constexpr int kCap = THREADS * SPT;
    __shared__ double dl[2][kCap];
    __shared__ unsigned short bpl[kBtBlock * kCap];
    __shared__ int eidx[kWave ? kWaveEdges : 1];
    __shared__ double elp[kWave ? kWaveEdges : 1];
    __shared__ double redv[THREADS / 64];
    __shared__ int redi[THREADS / 64];
    __shared__ int cur_state;

    const int tid = threadIdx.x, job = blockIdx.x;
    const double kNaN = __longlong_as_double(0x7ff8000000000000LL), kNegInf = -INFINITY;

    // a job whose sizes leave the arrays of the call is answered with status 3
    HmmJob jb;
    bool ok = hmm_job_load(a, job, jb);
    const int m = jb.m, want = jb.want, N = jb.N, E = jb.E, T = jb.T, s0 = jb.s0, e0 = jb.e0;
    const long long f0 = jb.f0;
    long long po = 0, bo = 0;
    if (ok && want) {
        po = a.path_off[job], bo = a.bp_off[job];
        ok = po >= 0 && po + T <= a.path_elems && bo >= 0 && bo + (long long)T * N <= a.bp_elems;
    }
    const bool wave_job = ok && N <= kWaveStates && E <= kWaveEdges;
    if (!ok) {
        if (kWave && tid == 0) a.score[job] = kNaN, a.status[job] = HMM_BAD_JOB;
        return;
    }
    if (wave_job != kWave) return;

    const int* pptr = a.pred_ptr + s0 + m;
    const int* gidx = a.pred_idx + e0;
    const double* glp = a.pred_logp + e0;
    int em[SPT], pb[SPT], pe[SPT];
    int bad_model = 0;
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int j = tid + k * THREADS;
        em[k] = 0, pb[k] = 0, pe[k] = 0;
        if (j < N) {
            em[k] = a.emit[s0 + j], pb[k] = pptr[j], pe[k] = pptr[j + 1];
            if ((unsigned)em[k] >= (unsigned)a.g || pb[k] < 0 || pe[k] < pb[k] || pe[k] > E) bad_model = 1, em[k] = 0, pe[k] = pb[k] = 0;
            for (int e = pb[k]; e < pe[k]; ++e)
                if ((unsigned)gidx[e] >= (unsigned)N) bad_model = 1;
        }
    }
    if (kWave)
        for (int e = tid; e < E; e += THREADS) eidx[e] = gidx[e], elp[e] = glp[e];
    if (__syncthreads_or(bad_model)) {
        if (tid == 0) a.score[job] = kNaN, a.status[job] = HMM_BAD_JOB;
        return;
    }

    const double* lb = a.logb + (size_t)f0 * a.g;
    unsigned short* bp = a.bp + bo;
    int bad = 0;
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int j = tid + k * THREADS;
        if (j < N) {
            const double v = a.log_pi[s0 + j] + lb[em[k]];
            dl[0][j] = v;
            bad |= v != v;
        }
    }
    // logB does not depend on the chain: the frames go in groups of kAhead, and a group's values are loaded while the group
    // before it runs, so that a step never waits for memory
    constexpr int kAhead = kWave ? 8 : 2;
    double here[kAhead][SPT], ahead[kAhead][SPT];
    auto load_group = [&](double (&dst)[kAhead][SPT], int tb) {
#pragma unroll
        for (int f = 0; f < kAhead; ++f)
#pragma unroll
            for (int k = 0; k < SPT; ++k)
                dst[f][k] = (tid + k * THREADS < N && tb + f < T) ? lb[(size_t)(tb + f) * a.g + em[k]] : 0.0;
    };
    load_group(here, 1);
    for (int tb = 1; tb < T; tb += kAhead) {
        load_group(ahead, tb + kAhead);
#pragma unroll
        for (int f = 0; f < kAhead; ++f) {
            const int t = tb + f;
            if (t >= T) break;
            const double* prev = dl[(t - 1) & 1];
            double* now = dl[t & 1];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < SPT; ++k) {
                const int j = tid + k * THREADS;
                if (j < N) {
                    double best = kNegInf;
                    int arg = kNoPred;
                    for (int e = pb[k]; e < pe[k]; ++e) {
                        const int i = kWave ? eidx[e] : gidx[e];
                        const double cand = prev[i] + (kWave ? elp[e] : glp[e]);
                        if (cand > best) best = cand, arg = i;
                    }
                    const double v = best + here[f][k];
                    now[j] = v;
                    bad |= v != v;
                    if (want) bp[(size_t)t * N + j] = (unsigned short)arg;
                }
            }
        }
#pragma unroll
        for (int f = 0; f < kAhead; ++f)
#pragma unroll
            for (int k = 0; k < SPT; ++k) here[f][k] = ahead[f][k];
    }
    __syncthreads();

    // score = max_j (delta_{T-1}[j] + log_final[j]), the lowest j on ties
    const double* last = dl[(T - 1) & 1];
    double bv = kNegInf;
    int bi = INT_MAX;
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int j = tid + k * THREADS;
        if (j < N) {
            const double v = last[j] + a.log_final[s0 + j];
            bad |= v != v;
            hmm_take_better(bv, bi, v, j);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double v2 = __shfl_xor(bv, off, 64);
        const int i2 = __shfl_xor(bi, off, 64);
        hmm_take_better(bv, bi, v2, i2);
    }
    if ((tid & 63) == 0) redv[tid >> 6] = bv, redi[tid >> 6] = bi;
    bad = __syncthreads_or(bad);
    for (int w = 0; w < THREADS / 64; ++w) hmm_take_better(bv, bi, redv[w], redi[w]);
    const int st = bad ? HMM_NAN : (bv == kNegInf ? HMM_NO_PATH : HMM_OK);
    if (tid == 0) a.score[job] = bad ? kNaN : bv, a.status[job] = st;
    if (!want) return;

    int* path = a.path + po;
    if (st != HMM_OK) {
        for (int t = tid; t < T; t += THREADS) path[t] = -1;
        return;
    }
    // the backtrack: kBtBlock frames of backpointers at a time pass into LDS, where one lane follows them
    if (tid == 0) cur_state = bi;
    for (int t0 = (T - 1) / kBtBlock * kBtBlock; t0 >= 0; t0 -= kBtBlock) {
        const int t1 = t0 + kBtBlock < T ? t0 + kBtBlock : T;
        const int lo = t0 > 1 ? t0 : 1;  // frame 0 has no backpointers
        __syncthreads();
        for (int i = (lo - t0) * N + tid; i < (t1 - t0) * N; i += THREADS) bpl[i] = bp[(size_t)t0 * N + i];
        __syncthreads();
        if (tid == 0) {
            int c = cur_state;
            for (int t = t1 - 1; t >= lo; --t) {
                path[t] = c;
                c = bpl[(t - t0) * N + c];
            }
            if (t0 == 0) path[0] = c;
            cur_state = c;
        }
    }
}

// ---- S100 forward-backward ------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_hmm_exp(const double* __restrict__ in, long long n, double* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = exp(in[i]);
}

// The sum of one double per thread over the workgroup, the same bits in every thread: an xor butterfly over the lanes of each
// wave (offsets 32 .. 1), then the waves in ascending order.  red: THREADS / 64 doubles that no thread writes again before the
// next barrier of the caller.
template <int THREADS>
__device__ __forceinline__ double hmm_wg_sum(double v, double* red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    if (THREADS == 64) return v;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int w = 1; w < THREADS / 64; ++w) r = r + red[w];
    return r;
}

// One (sequence, model) job per workgroup, in the two forms of k_hmm_viterbi.  The forward pass leaves alpha-hat in the job's
// gamma rows and (m_t, c_t) in its mc rows; the backward pass turns the rows into gamma and sums xi per edge, each edge by the
// thread that owns its target state (in LDS in the single-wave form, in the job's xi row otherwise), frames descending.
template <int THREADS, int SPT>
__global__ void __launch_bounds__(THREADS) k_hmm_fb(const HmmBatch a)
{
    constexpr bool kWave = THREADS == kWaveStates;
    constexpr int kCap = THREADS * SPT;
    constexpr int kLdsEdges = kWave ? kWaveEdges : 1;
    __shared__ double al[2][kCap], wl[2][kCap];
    __shared__ int eidx[kLdsEdges], sidx[kLdsEdges], sedge[kLdsEdges];
    __shared__ double epl[kLdsEdges], xil[kLdsEdges];
    __shared__ double red[2][THREADS / 64];

    const int tid = threadIdx.x, job = blockIdx.x;
    const double kNaN = __longlong_as_double(0x7ff8000000000000LL), kNegInf = -INFINITY;
    HmmJob jb;
    bool ok = hmm_job_load(a, job, jb);
    const int m = jb.m, N = jb.N, E = jb.E, T = jb.T, s0 = jb.s0, e0 = jb.e0;
    long long go = 0, xo = 0, mo = 0;
    if (ok) {
        go = a.gamma_off[job], xo = a.xi_off[job], mo = a.mc_off[job];
        ok = go >= 0 && go + (long long)T * N <= a.gamma_elems && xo >= 0 && xo + E <= a.xi_elems && mo >= 0 &&
             mo + 2LL * T <= a.mc_elems;
    }
    if (!ok) {
        if (kWave && tid == 0) a.loglik[job] = kNaN, a.status[job] = HMM_BAD_JOB;
        return;
    }
    if ((N <= kWaveStates && E <= kWaveEdges) != kWave) return;

    const int* pptr = a.pred_ptr + s0 + m;
    const int* sptr = a.succ_ptr + s0 + m;
    const int* gidx = a.pred_idx + e0;
    const int* gsidx = a.succ_idx + e0;
    const int* gsedge = a.succ_edge + e0;
    const double* gep = a.edge_p + e0;
    const int* emit = a.emit + s0;
    const double* lb = a.logb + (size_t)jb.f0 * a.g;
    double* gam = a.gamma + go;
    double* xig = a.xi + xo;
    double* mc = a.mc + mo;

    int em[SPT], pb[SPT], pe[SPT], sb[SPT], se[SPT];
    int bad_model = 0;
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int j = tid + k * THREADS;
        em[k] = pb[k] = pe[k] = sb[k] = se[k] = 0;
        if (j < N) {
            em[k] = emit[j], pb[k] = pptr[j], pe[k] = pptr[j + 1], sb[k] = sptr[j], se[k] = sptr[j + 1];
            if ((unsigned)em[k] >= (unsigned)a.g || pb[k] < 0 || pe[k] < pb[k] || pe[k] > E || sb[k] < 0 || se[k] < sb[k] || se[k] > E)
                bad_model = 1, em[k] = pb[k] = pe[k] = sb[k] = se[k] = 0;
            for (int e = pb[k]; e < pe[k]; ++e)
                if ((unsigned)gidx[e] >= (unsigned)N) bad_model = 1;
            for (int e = sb[k]; e < se[k]; ++e)
                if ((unsigned)gsidx[e] >= (unsigned)N || (unsigned)gsedge[e] >= (unsigned)E) bad_model = 1;
        }
    }
    if (__syncthreads_or(bad_model)) {
        if (tid == 0) a.loglik[job] = kNaN, a.status[job] = HMM_BAD_JOB;
        return;
    }
    for (int e = tid; e < E; e += THREADS) {
        if (kWave)
            eidx[e] = gidx[e], epl[e] = gep[e], sidx[e] = gsidx[e], sedge[e] = gsedge[e], xil[e] = 0.0;
        else
            xig[e] = 0.0;
    }

    // m_t = max_j logB[t][emit j], every frame on its own; a NaN or +inf there is status 2, a frame of -inf alone status 1
    int nan_seen = 0, dead = 0;
    for (int t = tid; t < T; t += THREADS) {
        double mx = kNegInf;
        for (int j = 0; j < N; ++j) {
            const double v = lb[(size_t)t * a.g + emit[j]];
            nan_seen |= (v != v) || v == INFINITY;
            mx = v > mx ? v : mx;
        }
        mc[2 * t] = mx;
        dead |= mx == kNegInf;
    }
    nan_seen = __syncthreads_or(nan_seen);
    dead = __syncthreads_or(dead);
    int st = nan_seen ? HMM_NAN : (dead ? HMM_NO_PATH : HMM_OK);

    double ll = 0.0, beta[SPT];
    if (st == HMM_OK) {
        // forward
        double cur[SPT];
        for (int t = 0; t < T; ++t) {
            const double mt = mc[2 * t];
            const double* prev = al[(t - 1) & 1];
            if (t > 0) __syncthreads();
#pragma unroll
            for (int k = 0; k < SPT; ++k) {
                const int j = tid + k * THREADS;
                cur[k] = 0.0;
                if (j < N) {
                    const double b = exp(lb[(size_t)t * a.g + em[k]] - mt);
                    double sum;
                    if (t == 0) {
                        sum = a.pi_p[s0 + j];
                    } else {
                        sum = 0.0;
                        for (int e = pb[k]; e < pe[k]; ++e) sum = sum + prev[kWave ? eidx[e] : gidx[e]] * (kWave ? epl[e] : gep[e]);
                    }
                    cur[k] = b * sum;
                }
            }
            double part = cur[0];
#pragma unroll
            for (int k = 1; k < SPT; ++k) part = part + cur[k];
            const double c = hmm_wg_sum<THREADS>(part, red[t & 1]);
            if (!(c > 0.0 && c < INFINITY)) {
                st = c == 0.0 ? HMM_NO_PATH : HMM_NAN;
                break;
            }
#pragma unroll
            for (int k = 0; k < SPT; ++k) {
                const int j = tid + k * THREADS;
                if (j < N) {
                    cur[k] = cur[k] / c;
                    al[t & 1][j] = cur[k];
                    gam[(size_t)t * N + j] = cur[k];
                }
            }
            if (tid == 0) mc[2 * t + 1] = c, ll = ll + (log(c) + mt);
        }
        if (st == HMM_OK) {
            // the end: c_T = sum_j alpha-hat_{T-1}[j] final[j], beta-hat_{T-1} = final / c_T
            double fin[SPT], part = 0.0;
#pragma unroll
            for (int k = 0; k < SPT; ++k) {
                const int j = tid + k * THREADS;
                fin[k] = j < N ? a.fin_p[s0 + j] : 0.0;
                part = part + (j < N ? cur[k] * fin[k] : 0.0);
            }
            __syncthreads();
            const double c = hmm_wg_sum<THREADS>(part, red[T & 1]);
            if (!(c > 0.0 && c < INFINITY)) {
                st = c == 0.0 ? HMM_NO_PATH : HMM_NAN;
            } else {
                ll = ll + log(c);
#pragma unroll
                for (int k = 0; k < SPT; ++k) {
                    const int j = tid + k * THREADS;
                    beta[k] = fin[k] / c;
                    if (j < N) gam[(size_t)(T - 1) * N + j] = cur[k] * beta[k];
                }
            }
        }
    }
    __syncthreads();  // the rows of gamma and mc written above are read below by other threads
    if (st != HMM_OK) {
        for (long long i = tid; i < (long long)T * N; i += THREADS) gam[i] = 0.0;
        for (int e = tid; e < E; e += THREADS) xig[e] = 0.0;
        if (tid == 0) a.loglik[job] = st == HMM_NAN ? kNaN : kNegInf, a.status[job] = st;
        return;
    }

    // backward
    for (int t = T - 2; t >= 0; --t) {
        const int par = t & 1;
        const double mt = mc[2 * (t + 1)], ct = mc[2 * (t + 1) + 1];
        double at[SPT], w[SPT];
#pragma unroll
        for (int k = 0; k < SPT; ++k) {
            const int j = tid + k * THREADS;
            at[k] = w[k] = 0.0;
            if (j < N) {
                const double b = exp(lb[(size_t)(t + 1) * a.g + em[k]] - mt);
                w[k] = (b * beta[k]) / ct;
                at[k] = gam[(size_t)t * N + j];
                wl[par][j] = w[k];
                al[par][j] = at[k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SPT; ++k) {
            const int j = tid + k * THREADS;
            if (j < N) {
                double sum = 0.0;
                for (int e = sb[k]; e < se[k]; ++e) {
                    const int to = kWave ? sidx[e] : gsidx[e];
                    const int pos = kWave ? sedge[e] : gsedge[e];
                    sum = sum + (kWave ? epl[pos] : gep[pos]) * wl[par][to];
                }
                beta[k] = sum;
                for (int e = pb[k]; e < pe[k]; ++e) {
                    const double add = (al[par][kWave ? eidx[e] : gidx[e]] * (kWave ? epl[e] : gep[e])) * w[k];
                    if (kWave)
                        xil[e] = xil[e] + add;
                    else
                        xig[e] = xig[e] + add;
                }
                gam[(size_t)t * N + j] = at[k] * beta[k];
            }
        }
    }
    if (kWave) {
        __syncthreads();
        for (int e = tid; e < E; e += THREADS) xig[e] = xil[e];
    }
    if (tid == 0) a.loglik[job] = ll, a.status[job] = HMM_OK;
}

// ---- S100 statistics ------------------------------------------------------------------------------------------------------

// stats[g] = [ sum w | sum w x [d] | sum w (x x) [d] ] for Gaussian g = blockIdx.x and the 64 columns of blockIdx.y.  Soft: w is
// gamma of the contributions contrib_ptr[g] .. contrib_ptr[g + 1] - 1, each (first frame, frames, states of its model, state)
// with its job's gamma rows at contrib_off; hard: w = 1 on the frames whose align is g.  Wave v of the four adds the frames
// t = v, v + 4, ... of every contribution in ascending order, contributions ascending; the result is ((p0 + p1) + p2) + p3.
// A contribution that leaves the arrays turns the Gaussian's count into NaN.
__global__ void __launch_bounds__(256) k_hmm_stats(const void* __restrict__ xv, int x_is_f64, int t_total, int d, int mode,
                                                   const double* __restrict__ gamma, long long gamma_elems,
                                                   const int* __restrict__ contrib_ptr, const int* __restrict__ contrib,
                                                   const long long* __restrict__ contrib_off, int n_contrib,
                                                   const int* __restrict__ align, double* __restrict__ stats)
{
    __shared__ double part[3][4][64];
    const int g = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int col = blockIdx.y * 64 + lane;
    const bool live = col < d;
    const float* xf = (const float*)xv;
    const double* xd = (const double*)xv;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    bool broken = false;
    if (mode == 0) {
        int c0 = contrib_ptr[g], c1 = contrib_ptr[g + 1];
        if (c0 < 0 || c1 < c0 || c1 > n_contrib) broken = true, c1 = c0 = 0;
        for (int c = c0; c < c1; ++c) {
            const int f0 = contrib[4 * c], T = contrib[4 * c + 1], N = contrib[4 * c + 2], j = contrib[4 * c + 3];
            const long long off = contrib_off[c];
            if (f0 < 0 || T < 1 || (long long)f0 + T > t_total || N < 1 || j < 0 || j >= N || off < 0 || off + (long long)T * N > gamma_elems) {
                broken = true;
                continue;
            }
            const double* gm = gamma + off + j;
            for (int t = wv; t < T; t += 4) {
                const double w = gm[(size_t)t * N];
                const size_t at = (size_t)(f0 + t) * d + col;
                const double x = live ? (x_is_f64 ? xd[at] : (double)xf[at]) : 0.0;
                s0 = s0 + w;
                s1 = s1 + w * x;
                s2 = s2 + w * (x * x);
            }
        }
    } else {
        for (int t = wv; t < t_total; t += 4) {
            if (align[t] != g) continue;
            const size_t at = (size_t)t * d + col;
            const double x = live ? (x_is_f64 ? xd[at] : (double)xf[at]) : 0.0;
            s0 = s0 + 1.0;
            s1 = s1 + x;
            s2 = s2 + x * x;
        }
    }
    part[0][wv][lane] = s0, part[1][wv][lane] = s1, part[2][wv][lane] = s2;
    __syncthreads();
    if (wv == 0 && live) {
        double r[3];
        for (int q = 0; q < 3; ++q) r[q] = ((part[q][0][lane] + part[q][1][lane]) + part[q][2][lane]) + part[q][3][lane];
        double* out = stats + (size_t)g * (1 + 2 * d);
        if (col == 0) out[0] = broken ? __longlong_as_double(0x7ff8000000000000LL) : r[0];
        out[1 + col] = r[1];
        out[1 + d + col] = r[2];
    }
}

struct HmmFbPlan {
    double *edge_p, *pi_p, *fin_p, *mc;
    size_t bytes;
};
HmmFbPlan hmm_fb_plan(void* base, int n_states_total, int n_edges_total, size_t mc_elems)
{
    va_carver ws{base};
    HmmFbPlan p;
    p.edge_p = ws.take<double>((size_t)(n_edges_total > 0 ? n_edges_total : 1));
    p.pi_p = ws.take<double>((size_t)n_states_total);
    p.fin_p = ws.take<double>((size_t)n_states_total);
    p.mc = ws.take<double>(mc_elems);
    p.bytes = ws.off;
    return p;
}

int hmm_check_sizes(const char* who, long long t_total, int g)
{
    VA_CHECK_ARG(t_total >= 1 && t_total <= INT_MAX, "%s: t_total out of range: need 1 <= t_total <= %d (got %lld)", who, INT_MAX, t_total);
    VA_CHECK_ARG(g >= 1 && g <= 65535 * kEmG, "%s: g out of range: need 1 <= g <= %d (got %d)", who, 65535 * kEmG, g);
    return VA_OK;
}

}  // namespace

extern "C" int va_hmm_wave_states(void) { return kWaveStates; }
extern "C" int va_hmm_wave_edges(void) { return kWaveEdges; }
extern "C" int va_hmm_backtrack_block(void) { return kBtBlock; }

extern "C" int va_hmm_emissions(va_ctx* ctx, const void* x, int x_is_f64, int t_total, int d, const void* means, const void* inv_var,
                                const void* consts, int g, void* logb, void* stream)
{
    const char* who = "va_hmm_emissions";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x && means && inv_var && consts && logb, "%s: NULL pointer", who);
    VA_CHECK_ARG(x_is_f64 == 0 || x_is_f64 == 1, "%s: x_is_f64 must be 0 or 1 (got %d)", who, x_is_f64);
    if (int rc = hmm_check_sizes(who, t_total, g)) return rc;
    VA_CHECK_ARG(d >= 1 && d <= kHmmMaxDim, "%s: d out of range: need 1 <= d <= %d (got %d)", who, kHmmMaxDim, d);
    const long long by = ((long long)t_total + kEmT - 1) / kEmT;
    hipStream_t st = (hipStream_t)stream;
    // a grid's y extent holds 65535 tiles of frames: longer inputs go in slices
    for (long long b0 = 0; b0 < by; b0 += 65535) {
        const long long nb = by - b0 < 65535 ? by - b0 : 65535, r0 = b0 * kEmT;
        const int rows = (int)((long long)t_total - r0 < nb * kEmT ? (long long)t_total - r0 : nb * kEmT);
        const dim3 grid(va_cdiv(g, kEmG), (unsigned)nb);
        double* out = (double*)logb + (size_t)r0 * g;
        if (x_is_f64)
            k_hmm_emissions<double><<<grid, 256, 0, st>>>((const double*)x + (size_t)r0 * d, rows, d, (const double*)means,
                                                          (const double*)inv_var, (const double*)consts, g, out);
        else
            k_hmm_emissions<float><<<grid, 256, 0, st>>>((const float*)x + (size_t)r0 * d, rows, d, (const double*)means,
                                                         (const double*)inv_var, (const double*)consts, g, out);
    }
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_hmm_viterbi(va_ctx* ctx, const void* logb, int t_total, int g, const void* seq_ptr, int n_seqs, const void* state_ptr,
                              const void* edge_ptr, int n_models, int n_states_total, int n_edges_total, const void* emit,
                              const void* pred_ptr, const void* pred_idx, const void* pred_logp, const void* log_pi,
                              const void* log_final, const void* jobs, int n_jobs, const void* path_off, const void* bp_off,
                              void* score, void* status, void* path, size_t path_elems, size_t bp_elems, void* workspace,
                              size_t workspace_bytes, void* stream)
{
    const char* who = "va_hmm_viterbi";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(logb && seq_ptr && state_ptr && edge_ptr && emit && pred_ptr && log_pi && log_final && jobs && score && status,
                 "%s: NULL pointer", who);
    if (int rc = hmm_check_sizes(who, t_total, g)) return rc;
    VA_CHECK_ARG(n_seqs >= 1 && n_models >= 1 && n_jobs >= 1, "%s: need n_seqs, n_models, n_jobs >= 1 (got %d, %d, %d)", who, n_seqs,
                 n_models, n_jobs);
    VA_CHECK_ARG(n_states_total >= 1 && n_edges_total >= 0, "%s: need n_states_total >= 1 and n_edges_total >= 0 (got %d, %d)", who,
                 n_states_total, n_edges_total);
    VA_CHECK_ARG(n_edges_total == 0 || (pred_idx && pred_logp), "%s: NULL pointer (pred_idx, pred_logp)", who);
    VA_CHECK_ARG(path_elems <= (size_t)LLONG_MAX && bp_elems <= (size_t)LLONG_MAX / 2, "%s: path_elems or bp_elems out of range", who);
    VA_CHECK_ARG((path_elems == 0 && bp_elems == 0) || (path && path_off && bp_off),
                 "%s: a call that decodes paths needs path, path_off and bp_off", who);
    VA_CHECK_ARG(bp_elems == 0 || (workspace != nullptr && ((size_t)workspace & 255) == 0),
                 "%s: workspace must be a 256-byte aligned DEVICE pointer", who);
    if (workspace_bytes < bp_elems * sizeof(unsigned short)) {
        va_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, bp_elems * sizeof(unsigned short));
        return VA_ERR_WORKSPACE;
    }
    HmmBatch a{};
    a.logb = (const double*)logb, a.seq_ptr = (const int*)seq_ptr, a.state_ptr = (const int*)state_ptr, a.edge_ptr = (const int*)edge_ptr;
    a.emit = (const int*)emit, a.pred_ptr = (const int*)pred_ptr, a.pred_idx = (const int*)pred_idx, a.pred_logp = (const double*)pred_logp;
    a.log_pi = (const double*)log_pi, a.log_final = (const double*)log_final, a.jobs = (const int*)jobs;
    a.path_off = (const long long*)path_off, a.bp_off = (const long long*)bp_off;
    a.score = (double*)score, a.status = (int*)status, a.path = (int*)path, a.bp = (unsigned short*)workspace;
    a.path_elems = (long long)path_elems, a.bp_elems = (long long)bp_elems;
    a.t_total = t_total, a.g = g, a.n_seqs = n_seqs, a.n_models = n_models, a.n_states_total = n_states_total, a.n_edges_total = n_edges_total;
    hipStream_t st = (hipStream_t)stream;
    // every job is offered to both forms; each takes the jobs of its size and leaves at once on the others
    k_hmm_viterbi<kWaveStates, 1><<<n_jobs, kWaveStates, 0, st>>>(a);
    k_hmm_viterbi<kWgThreads, kHmmMaxStates / kWgThreads><<<n_jobs, kWgThreads, 0, st>>>(a);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" size_t va_hmm_fb_workspace_bytes(int n_states_total, int n_edges_total, size_t mc_elems)
{
    if (n_states_total < 1 || n_edges_total < 0 || mc_elems < 2 || mc_elems > ((size_t)1 << 40)) {
        va_set_error("va_hmm_fb_workspace_bytes: need n_states_total >= 1, n_edges_total >= 0 and 2 <= mc_elems <= 2^40 (got %d, %d, %zu)",
                     n_states_total, n_edges_total, mc_elems);
        return 0;
    }
    return hmm_fb_plan(nullptr, n_states_total, n_edges_total, mc_elems).bytes;
}

extern "C" int va_hmm_forward_backward(va_ctx* ctx, const void* logb, int t_total, int g, const void* seq_ptr, int n_seqs,
                                       const void* state_ptr, const void* edge_ptr, int n_models, int n_states_total, int n_edges_total,
                                       const void* emit, const void* pred_ptr, const void* pred_idx, const void* pred_logp,
                                       const void* log_pi, const void* log_final, const void* succ_ptr, const void* succ_idx,
                                       const void* succ_edge, const void* jobs, int n_jobs, const void* gamma_off, const void* xi_off,
                                       const void* mc_off, void* gamma, size_t gamma_elems, void* xi, size_t xi_elems, size_t mc_elems,
                                       void* loglik, void* status, void* workspace, size_t workspace_bytes, void* stream)
{
    const char* who = "va_hmm_forward_backward";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(logb && seq_ptr && state_ptr && edge_ptr && emit && pred_ptr && log_pi && log_final && succ_ptr && jobs && gamma_off &&
                     xi_off && mc_off && gamma && xi && loglik && status,
                 "%s: NULL pointer", who);
    if (int rc = hmm_check_sizes(who, t_total, g)) return rc;
    VA_CHECK_ARG(n_seqs >= 1 && n_models >= 1 && n_jobs >= 1, "%s: need n_seqs, n_models, n_jobs >= 1 (got %d, %d, %d)", who, n_seqs,
                 n_models, n_jobs);
    VA_CHECK_ARG(n_states_total >= 1 && n_edges_total >= 0, "%s: need n_states_total >= 1 and n_edges_total >= 0 (got %d, %d)", who,
                 n_states_total, n_edges_total);
    VA_CHECK_ARG(n_edges_total == 0 || (pred_idx && pred_logp && succ_idx && succ_edge), "%s: NULL pointer (edges)", who);
    VA_CHECK_ARG(gamma_elems >= 1 && gamma_elems <= (size_t)LLONG_MAX / 8 && xi_elems <= (size_t)LLONG_MAX / 8 && mc_elems >= 2 &&
                     mc_elems <= ((size_t)1 << 40),
                 "%s: gamma_elems, xi_elems or mc_elems out of range", who);
    VA_CHECK_ARG(workspace != nullptr && ((size_t)workspace & 255) == 0, "%s: workspace must be a 256-byte aligned DEVICE pointer", who);
    const HmmFbPlan p = hmm_fb_plan(workspace, n_states_total, n_edges_total, mc_elems);
    if (workspace_bytes < p.bytes) {
        va_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, p.bytes);
        return VA_ERR_WORKSPACE;
    }
    HmmBatch a{};
    a.logb = (const double*)logb, a.seq_ptr = (const int*)seq_ptr, a.state_ptr = (const int*)state_ptr, a.edge_ptr = (const int*)edge_ptr;
    a.emit = (const int*)emit, a.pred_ptr = (const int*)pred_ptr, a.pred_idx = (const int*)pred_idx, a.pred_logp = (const double*)pred_logp;
    a.log_pi = (const double*)log_pi, a.log_final = (const double*)log_final, a.jobs = (const int*)jobs;
    a.status = (int*)status;
    a.t_total = t_total, a.g = g, a.n_seqs = n_seqs, a.n_models = n_models, a.n_states_total = n_states_total, a.n_edges_total = n_edges_total;
    a.succ_ptr = (const int*)succ_ptr, a.succ_idx = (const int*)succ_idx, a.succ_edge = (const int*)succ_edge;
    a.edge_p = p.edge_p, a.pi_p = p.pi_p, a.fin_p = p.fin_p, a.mc = p.mc;
    a.gamma_off = (const long long*)gamma_off, a.xi_off = (const long long*)xi_off, a.mc_off = (const long long*)mc_off;
    a.gamma = (double*)gamma, a.xi = (double*)xi, a.loglik = (double*)loglik;
    a.gamma_elems = (long long)gamma_elems, a.xi_elems = (long long)xi_elems, a.mc_elems = (long long)mc_elems;
    hipStream_t st = (hipStream_t)stream;
    if (n_edges_total > 0) k_hmm_exp<<<va_cdiv(n_edges_total, 256), 256, 0, st>>>((const double*)pred_logp, n_edges_total, p.edge_p);
    k_hmm_exp<<<va_cdiv(n_states_total, 256), 256, 0, st>>>((const double*)log_pi, n_states_total, p.pi_p);
    k_hmm_exp<<<va_cdiv(n_states_total, 256), 256, 0, st>>>((const double*)log_final, n_states_total, p.fin_p);
    k_hmm_fb<kWaveStates, 1><<<n_jobs, kWaveStates, 0, st>>>(a);
    k_hmm_fb<kWgThreads, kHmmMaxStates / kWgThreads><<<n_jobs, kWgThreads, 0, st>>>(a);
    VA_LAUNCH_CHECK();
    return VA_OK;
}

extern "C" int va_hmm_gauss_stats(va_ctx* ctx, const void* x, int x_is_f64, int t_total, int d, int g, int mode, const void* gamma,
                                  size_t gamma_elems, const void* contrib_ptr, const void* contrib, const void* contrib_off, int n_contrib,
                                  const void* align, void* stats, void* stream)
{
    const char* who = "va_hmm_gauss_stats";
    VA_CHECK_ARG(ctx != nullptr, "%s: ctx is NULL", who);
    VA_USE_DEVICE(ctx);
    VA_CHECK_ARG(x && stats, "%s: NULL pointer", who);
    VA_CHECK_ARG(x_is_f64 == 0 || x_is_f64 == 1, "%s: x_is_f64 must be 0 or 1 (got %d)", who, x_is_f64);
    VA_CHECK_ARG(mode == 0 || mode == 1, "%s: mode must be 0 (gamma) or 1 (alignment) (got %d)", who, mode);
    VA_CHECK_ARG(t_total >= 1, "%s: t_total out of range: need t_total >= 1 (got %d)", who, t_total);
    VA_CHECK_ARG(d >= 1 && d <= kHmmMaxDim, "%s: d out of range: need 1 <= d <= %d (got %d)", who, kHmmMaxDim, d);
    VA_CHECK_ARG(g >= 1 && g <= 0x7fffffff / (1 + 2 * kHmmMaxDim), "%s: g out of range (got %d)", who, g);
    if (mode == 0)
        VA_CHECK_ARG(gamma && contrib_ptr && n_contrib >= 0 && (n_contrib == 0 || (contrib && contrib_off)) &&
                         gamma_elems <= (size_t)LLONG_MAX / 8,
                     "%s: the gamma mode needs gamma, contrib_ptr, contrib and contrib_off", who);
    else
        VA_CHECK_ARG(align != nullptr, "%s: the alignment mode needs align", who);
    k_hmm_stats<<<dim3(g, va_cdiv(d, 64)), 256, 0, (hipStream_t)stream>>>(x, x_is_f64, t_total, d, mode, (const double*)gamma,
                                                                        (long long)gamma_elems, (const int*)contrib_ptr,
                                                                        (const int*)contrib, (const long long*)contrib_off, n_contrib,
                                                                        (const int*)align, (double*)stats);
    VA_LAUNCH_CHECK();
    return VA_OK;
}
