"""The kernel SVM on one MI355X: Gram matrices, the dual fit, and the dual route against the primal one.
Prints one JSON line per measurement.

    python tools/bench_ksvm.py [--n 9537] [--classes 101] [--reps 5] [--warmup 1] [--wide 33024] [--skip gram_linear ...] [--host]

Every figure is the median of --reps timings with HIP events around the whole Python call (its statistics reads included),
after --warmup calls of the same shape; the variants of one comparison are interleaved, one repetition of each in turn.

  chi2_gram      ``ksvm.chi2_distance`` on n x 256 and n x 4096 float32 histograms, symmetric form: terms/s, counted over the
                 tiles the kernel computes, beside what the float64 vector pipe could deliver for the kernel's instruction count
                 per term -- 16 float64 and 2 32-bit vector instructions in the compiled inner loop, a wave's float64
                 instruction issuing over 4 clocks and a 32-bit one over 2 (the 78.6 TFLOP/s float64 vector peak is one FMA per
                 lane every 4 clocks on 1024 SIMDs at 2.4 GHz)
  gram_linear    ``ksvm.linear_gram`` on n x --wide float32 rows (Sheet02's Fisher vectors), beside the 78.6 TFLOP/s float64
                 matrix peak
  fit            ``ksvm.kernel_svm_fit`` on n rows x --classes classes over the linear kernel of 512 descriptors and over the
                 chi-square kernel of 256-word histograms, with outer and CG step counts
  routes         Gram + dual fit against ``fusion.linear_svm_fit`` on the same n x 512 x --classes problem
  --host         for scale only: sklearn's ``SVC(kernel="precomputed")`` on the host at a tenth of the rows"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_VALU_PER_TERM, B32_VALU_PER_TERM = 16, 2
SIMDS, CLOCK_HZ, F64_MATRIX_PEAK = 1024, 2.4e9, 78.6e12


def descriptors(n, k, d=512, seed=0):
    rng = np.random.RandomState(seed)
    labels = np.concatenate([np.arange(k), rng.randint(0, k, size=n - k)])[rng.permutation(n)]
    mu = rng.randn(k, d)
    return np.maximum(0.0, 0.3 * mu[labels] + rng.randn(n, d)).astype(np.float32), labels


def histograms(n, k, words, seed=0):
    """L1-normalised word counts of 200 draws per video from a class-dependent distribution over ``words`` words."""
    rng = np.random.RandomState(seed)
    labels = np.concatenate([np.arange(k), rng.randint(0, k, size=n - k)])[rng.permutation(n)]
    logits = 1.5 * rng.randn(k, words)
    p = np.exp(logits - logits.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    cum = np.cumsum(p, 1)
    draws = rng.rand(n, 200)
    h = np.zeros((n, words), dtype=np.float32)
    for i in range(n):
        np.add.at(h[i], np.minimum(np.searchsorted(cum[labels[i]], draws[i]), words - 1), 1.0)
    return h / h.sum(1, keepdims=True), labels


def timed(torch, variants, reps, warmup):
    """variants: {name: callable}; -> {name: (median ms, min, max, last result)}, one repetition of each in turn."""
    ms, last = {k: [] for k in variants}, {}
    for i in range(warmup + reps):
        for name, fn in variants.items():
            beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            beg.record()
            last[name] = fn()
            end.record()
            torch.cuda.synchronize()
            if i >= warmup:
                ms[name].append(beg.elapsed_time(end))
    return {k: (statistics.median(v), min(v), max(v), last[k]) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=9537)
    ap.add_argument("--classes", type=int, default=101)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--wide", type=int, default=33024)
    ap.add_argument("--skip", nargs="*", default=[], choices=["chi2_gram", "gram_linear", "fit", "routes"])
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_ksvm.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    from video_analytics_amd import fusion, ksvm
    n, k = args.n, args.classes
    common = dict(n=n, reps=args.reps)

    def emit(metric, **row):
        print(json.dumps(dict(metric=metric, **common, **row)), flush=True)

    if "chi2_gram" not in args.skip:
        data = {w: torch.as_tensor(histograms(n, k, w)[0]).cuda() for w in (256, 4096)}
        res = timed(torch, {w: (lambda x=x: ksvm.chi2_distance(x)) for w, x in data.items()}, args.reps, args.warmup)
        tiles = (n + 63) // 64
        bound = SIMDS * CLOCK_HZ * 64 / (4 * F64_VALU_PER_TERM + 2 * B32_VALU_PER_TERM)
        for w, (med, lo, hi, _) in res.items():
            terms = tiles * (tiles + 1) // 2 * 4096 * w
            emit("chi2_gram", words=w, ms=round(med, 2), ms_min=round(lo, 2), ms_max=round(hi, 2), terms_computed=terms,
                 terms_per_s=terms / (med * 1e-3), f64_valu_bound_terms_per_s=bound, share_of_bound=round(terms / (med * 1e-3) / bound, 3))
        del data
    if "gram_linear" not in args.skip:
        x = torch.randn((n, args.wide), dtype=torch.float32, device="cuda")
        med, lo, hi, _ = timed(torch, {"g": lambda: ksvm.linear_gram(x)}, args.reps, args.warmup)["g"]
        tiles = (n + 63) // 64
        flop = 2.0 * (tiles * (tiles + 1) // 2) * 4096 * args.wide
        emit("gram_linear", dim=args.wide, ms=round(med, 2), ms_min=round(lo, 2), ms_max=round(hi, 2), tflops=round(flop / (med * 1e-3) / 1e12, 2),
             share_of_f64_matrix_peak=round(flop / (med * 1e-3) / F64_MATRIX_PEAK, 4))
        del x
    X, labels = descriptors(n, k)
    xd = torch.as_tensor(X).cuda()
    if "fit" not in args.skip:
        H, hl = histograms(n, k, 256)
        grams = {"linear": (ksvm.linear_gram(xd), labels), "chi2": (ksvm.chi2_kernel(torch.as_tensor(H).cuda())[0], hl)}
        res = timed(torch, {name: (lambda K=K, y=y: ksvm.kernel_svm_fit(K, y, return_info=True)) for name, (K, y) in grams.items()},
                    args.reps, args.warmup)
        for name, (med, lo, hi, out) in res.items():
            info = out[3]
            emit("fit", kernel=name, classes=k, ms=round(med, 2), ms_min=round(lo, 2), ms_max=round(hi, 2), converged=bool(info["converged"]),
                 outer_steps=int(info["n_iter"]), outer_steps_sum=int(info["steps"].sum()), cg_steps_max=int(info["cg_steps"].max()),
                 cg_steps_sum=int(info["cg_steps"].sum()), support_vectors_mean=float(info["n_sv"].mean()), rel_pg_max=float(info["rel_pg"].max()))
        del grams
    if "routes" not in args.skip:
        res = timed(torch, {"primal": lambda: fusion.linear_svm_fit(xd, labels, return_info=True),
                            "dual": lambda: ksvm.kernel_svm_fit(ksvm.linear_gram(xd), labels, return_info=True),
                            "gram_only": lambda: ksvm.linear_gram(xd)}, args.reps, args.warmup)
        emit("routes", dim=512, classes=k, primal_ms=round(res["primal"][0], 2), dual_ms=round(res["dual"][0], 2),
             gram_ms=round(res["gram_only"][0], 2), primal_newton_steps=int(res["primal"][3][3]["n_iter"]),
             dual_outer_steps=int(res["dual"][3][3]["n_iter"]), winner="primal" if res["primal"][0] < res["dual"][0] else "dual")
    if args.host:
        from sklearn import svm
        m = n // 10
        K = ksvm.linear_gram(xd[:m]).cpu().numpy()
        t0 = time.perf_counter()
        svm.SVC(kernel="precomputed").fit(K, labels[:m])
        emit("host_scale", rows=m, sklearn_svc_precomputed_s=round(time.perf_counter() - t0, 2))


if __name__ == "__main__":
    main()
