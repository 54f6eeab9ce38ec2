// Multi-task consensus loss (the two-stream paper's multi-task learning, Sheet03/notes.txt:88-96): the third
// form of the training step's loss launch, beside k_ce_fwd_bwd and k_ce_consensus_fwd_bwd (train.hip).  It lives in a file
// of its own: tests/test_train_kernels_gpu.py pins the set of kernels train.hip launches to its own table, and this kernel's
// table is tests/test_multitask_gpu.py's.
#include "vgg_internal.h"

namespace {

constexpr int kMaxVideos = 64;  // the step's batch limit: one thread per video, one wavefront

// H heads of C_0 .. C_{H-1} classes share one last layer of C = sum C_t outputs: head t owns the logit columns
// [off[t], off[t + 1]).  Logits z[B][K][C] of B videos of K snippets each, labels i64 [B] LOCAL to the video's head, tasks i32
// [B].  Per video v of task t: m[v][c] = (((z[v][0][c] + z[v][1][c]) + ...) + z[v][K-1][c]) / (float)K on the head's columns
// (S20's mean); loss, hit and gradient are k_ce_fwd_bwd's expressions on that slice with inv_t = 1 / (float)n_t, n_t = the
// number of videos of task t, in the place of 1 / B; the columns outside the slice get 0; every snippet receives g / (float)K.
// Row 0 of a video's K gradient rows holds m until the gradient replaces it element by element (as k_ce_consensus_fwd_bwd).
// out[2 + 2H] = {loss, hits, loss_0 .. loss_{H-1}, hits_0 .. hits_{H-1}}: loss_t = (0.0f + l_v1 + l_v2 + ...) * inv_t over the
// head's videos in video order (0 for a head without videos), loss = (loss_t1 + loss_t2) + ... over the heads that have videos
// in head order.  No atomics: thread 0 forms every sum from LDS in a fixed order.
// A task outside [0, H) or a label outside [0, C_task): nothing is read out of bounds; loss, that head's loss_t (valid task)
// and all K * C gradient entries of the video become NaN, as the siblings do for a bad label.
__global__ void __launch_bounds__(kMaxVideos) k_ce_multitask_fwd_bwd(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                                     const int* __restrict__ tasks, int B, int K, int C, va_heads h,
                                                                     float* __restrict__ dlogits, float* __restrict__ out)
{
    __shared__ float sloss[kMaxVideos];
    __shared__ int scorr[kMaxVideos];
    __shared__ int stask[kMaxVideos];  // -1: outside [0, H)
    __shared__ int scount[VA_MAX_HEADS];
    const int v = threadIdx.x;
    int t = -1;
    if (v < B) {
        t = tasks[v];
        if (t < 0 || t >= h.n) t = -1;
    }
    stask[v] = t;
    __syncthreads();
    if (v < VA_MAX_HEADS) {  // n_t, by thread t
        int cnt = 0;
        for (int b = 0; b < B; ++b) cnt += (stask[b] == v);
        scount[v] = cnt;
    }
    __syncthreads();
    const float nan = __builtin_nanf("");
    if (v < B) {
        const float fk = (float)K;
        const float* z = logits + (size_t)v * K * C;
        float* l = dlogits + (size_t)v * K * C;
        float loss = nan;
        int corr = 0;
        if (t < 0) {
            for (size_t i = 0; i < (size_t)K * C; ++i) l[i] = nan;
        } else {
            int o = 0, ct = 0;  // the head's first column and size: constant indices only, the table stays in registers
#pragma unroll
            for (int q = 0; q < VA_MAX_HEADS; ++q)
                if (t == q) { o = h.off[q]; ct = h.off[q + 1] - h.off[q]; }
            const float inv_t = 1.0f / (float)scount[t];
            const long long y = labels[v];
            const bool yok = y >= 0 && y < (long long)ct;
            const float outside = yok ? 0.0f : nan;
            for (int j = 0; j < K; ++j) {  // the columns of the other heads: [0, o) and [o + ct, C)
                for (int c = 0; c < o; ++c) l[(size_t)j * C + c] = outside;
                for (int c = o + ct; c < C; ++c) l[(size_t)j * C + c] = outside;
            }
            const float* zs = z + o;
            float* ls = l + o;
            for (int c = 0; c < ct; ++c) {
                float s = zs[c];
                for (int j = 1; j < K; ++j) s += zs[(size_t)j * C + c];
                ls[c] = s / fk;
            }
            float mx = ls[0];
            int am = 0;
            for (int c = 1; c < ct; ++c)
                if (ls[c] > mx) { mx = ls[c]; am = c; }
            float se = 0.0f;
            for (int c = 0; c < ct; ++c) se += expf(ls[c] - mx);
            loss = yok ? (logf(se) + mx) - ls[yok ? y : 0] : nan;
            corr = (yok && am == (int)y);
            const float inv = yok ? 1.0f / se : nan;
            for (int c = 0; c < ct; ++c) {
                const float g = (expf(ls[c] - mx) * inv - (c == (int)y ? 1.0f : 0.0f)) * inv_t;
                const float gk = g / fk;
                for (int j = 0; j < K; ++j) ls[(size_t)j * C + c] = gk;
            }
        }
        sloss[v] = loss;
        scorr[v] = corr;
    }
    __syncthreads();
    if (v == 0) {
        float total = 0.0f;
        int hits = 0;
        bool first = true, bad_task = false;
        for (int q = 0; q < h.n; ++q) {
            float L = 0.0f;
            int Cc = 0;
            for (int b = 0; b < B; ++b)
                if (stask[b] == q) { L += sloss[b]; Cc += scorr[b]; }
            const int cnt = scount[q];
            const float lt = cnt > 0 ? L * (1.0f / (float)cnt) : 0.0f;
            out[2 + q] = lt;
            out[2 + h.n + q] = (float)Cc;
            if (cnt > 0) {
                total = first ? lt : total + lt;
                first = false;
            }
            hits += Cc;
        }
        for (int b = 0; b < B; ++b) bad_task = bad_task || stask[b] < 0;
        out[0] = bad_task ? nan : total;
        out[1] = (float)hits;
    }
}

}  // namespace

int va_heads_from_sizes(const char* who, int n_heads, const int* head_sizes, int n_classes, va_heads* out)
{
    VA_CHECK_ARG(head_sizes != nullptr, "%s: head_sizes is NULL", who);
    VA_CHECK_ARG(n_heads >= 1 && n_heads <= VA_MAX_HEADS, "%s: %d heads out of range [1,%d]", who, n_heads, VA_MAX_HEADS);
    va_heads h{};
    h.n = n_heads;
    for (int t = 0; t < n_heads; ++t) {
        VA_CHECK_ARG(head_sizes[t] >= 1 && head_sizes[t] <= (1 << 20), "%s: head %d has %d classes (need 1..2^20)", who, t, head_sizes[t]);
        h.off[t + 1] = h.off[t] + head_sizes[t];
    }
    for (int t = n_heads + 1; t <= VA_MAX_HEADS; ++t) h.off[t] = h.off[n_heads];
    VA_CHECK_ARG(n_classes < 0 || h.off[n_heads] == n_classes, "%s: the heads hold %d classes, the model's last layer %d", who, h.off[n_heads],
                 n_classes);
    *out = h;
    return VA_OK;
}

int va_ce_multitask(const float* logits, const long long* labels, const int* tasks, int videos, int segments, const va_heads& h,
                    float* dlogits, float* out, hipStream_t st)
{
    VA_CHECK_ARG(videos >= 1 && videos <= kMaxVideos && segments >= 1 && (long long)videos * segments <= kMaxVideos,
                 "multi-task loss: %d videos x %d snippets out of range (one thread per video, at most %d rows)", videos, segments, kMaxVideos);
    k_ce_multitask_fwd_bwd<<<1, kMaxVideos, 0, st>>>(logits, labels, tasks, videos, segments, h.off[h.n], h, dlogits, out);
    return VA_OK;
}
