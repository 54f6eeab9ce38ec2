"""The cost of the bag-of-words codebook on one MI355X.  One JSON line per measurement.

    python tools/bench_codebook.py [--rows 1000000] [--reps 5] [--warmup 1] [--host]

  assign_ms          one ``va_kmeans_assign`` pass at --rows x 144, K = 256 and K = 4096 (labels, d2, inertia)
  lloyd_step_ms      one assignment and one ``va_kmeans_update`` at those shapes
  gmm_hard_ms        one ``va_gmm_stats(VA_GMM_HARD)`` pass on the same rows at K = 256: the only way to take a Lloyd step
                     without this module; ``assign_over_gmm_hard`` and ``lloyd_over_gmm_hard`` are the ratios, whichever way
                     they fall
  seed_ms            ``va_kmeans_seed`` at K = 256 and K = 4096 (one run each at 4096: K dependent steps)
  kmeans_fit_ms      a whole ``codebook.kmeans_fit`` at K = 256 with its iteration count (one run)
  bow_encode_ms      ``va_bow_encode`` for 100 videos of 3,000 points, K = 256 and K = 4096

HIP events around each call, median of --reps with the range; the variants of one shape are interleaved (one call of each per
round), so drift reaches all of them alike.  Beside each time stand the float64 FLOP/s it amounts to (2 n K d for the
products; the direct distances and the sums are not counted), next to the device's float64 matrix peak (78.6 TFLOP/s, the
vendor's figure), and the bytes that must cross memory at least once (x read once per kernel that walks it, the outputs
written once), next to the HBM peak of 8 TB/s: which bound a pass obeys shows there.

--host adds ``sklearn.cluster.KMeans`` on the host, where it is installed, at a tenth of the rows, one run: a figure to set
the scale, not a like-for-like race.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_MATRIX_PEAK_TFLOPS, HBM_PEAK_TBS = 78.6, 8.0
D = 144


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def report(metric, ms, flops, nbytes, **more):
    med = statistics.median(ms)
    print(json.dumps(dict(metric=metric, ms=round(med, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), reps=len(ms),
                          f64_tflops=round(flops / med / 1e9, 3), f64_matrix_peak_tflops=F64_MATRIX_PEAK_TFLOPS,
                          tb_per_s=round(nbytes / med / 1e9, 4), hbm_peak_tb_per_s=HBM_PEAK_TBS, **more)), flush=True)
    return med


def descriptors(n, d, k, dev, seed=0):
    """non-negative float32 rows of unit norm around k prototypes, as normalised HOG/HOF descriptors are"""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    protos = torch.rand((k, d), generator=g, device=dev, dtype=torch.float32) ** 3
    z = torch.randint(0, k, (n,), generator=g, device=dev)
    x = (protos[z] + 0.3 * torch.rand((n, d), generator=g, device=dev, dtype=torch.float32) ** 3)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def interleaved(variants, warmup, reps):
    """{name: [ms]}: one call of each variant per round"""
    out = {name: [] for name in variants}
    for r in range(warmup + reps):
        for name, fn in variants.items():
            ms = timed(fn)[1]
            if r >= warmup:
                out[name].append(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from video_analytics_amd import codebook, fisher
    dev = torch.device("cuda", 0)
    n = args.rows
    x = descriptors(n, D, 256, dev)
    seg1 = np.array([0, n], dtype=np.int64)
    rng = np.random.RandomState(0)

    for k in (256, 4096):
        centres = x[torch.as_tensor(rng.permutation(n)[:k], device=dev)].double()
        labels = codebook.assign(x, centres)[0]

        def lloyd(c=centres):
            lab = codebook.assign(x, c, want_d2=False)[0]
            return codebook.update(x, lab, c)

        variants = {"assign": lambda c=centres: codebook.assign(x, c), "update": lambda c=centres, l=labels: codebook.update(x, l, c),
                    "lloyd": lloyd}
        if k <= fisher.MAX_GMM_COMPONENTS:
            w, var = torch.full((k,), 1.0 / k, dtype=torch.float64, device=dev), torch.ones((k, D), dtype=torch.float64, device=dev)
            variants["gmm_hard"] = lambda c=centres: fisher.gmm_stats(x, seg1, w, c, var, "hard")
        t = interleaved(variants, args.warmup, args.reps)
        flops = 2.0 * n * k * D
        a = report("assign_ms", t["assign"], flops, 2 * 4.0 * n * D + 12.0 * n, rows=n, d=D, k=k,
                   note="bytes: x by the product kernel and by the direct distances, labels and d2 written")
        report("update_ms", t["update"], 0.0, 4.0 * n * D + 4 * 4.0 * n, rows=n, d=D, k=k,
               note="bytes: labels twice, the permutation written and read, x gathered once")
        s = report("lloyd_step_ms", t["lloyd"], flops, 3 * 4.0 * n * D + 20.0 * n, rows=n, d=D, k=k)
        if "gmm_hard" in t:
            g = report("gmm_hard_ms", t["gmm_hard"], 2.0 * n * k * (2 * D) + 2.0 * n * k * (1 + 2 * D), 2 * 4.0 * n * D + 2 * 8.0 * n * k,
                       rows=n, d=D, k=k, note="the E-step kernels in VA_GMM_HARD mode: a [batch, K] one-hot written and multiplied back")
            print(json.dumps(dict(metric="ratio", k=k, assign_over_gmm_hard=round(a / g, 4), lloyd_over_gmm_hard=round(s / g, 4))), flush=True)
        u = rng.random_sample(k)
        t = [timed(lambda: codebook.seed(x, k, u))[1] for _ in range(1 + (args.reps if k == 256 else 1))][1:]
        report("seed_ms", t, 0.0, 4.0 * n * D * (k - 1) + 16.0 * n * (k - 1), rows=n, d=D, k=k, ms_per_centre=round(statistics.median(t) / k, 4),
               note="K - 1 dependent steps of four launches; bytes: x and m read, m written, per step")

    fit, ms = timed(lambda: codebook.kmeans_fit(x, 256, seed=0))
    steps = fit.n_iter + 1
    report("kmeans_fit_ms", [ms], 2.0 * n * 256 * D * steps, 3 * 4.0 * n * D * steps, rows=n, d=D, k=256, n_iter=fit.n_iter,
           converged=fit.converged, inertia=fit.inertia, empty_clusters=int((fit.counts == 0).sum()), ms_per_step=round(ms / steps, 3),
           note="k-means++ seeding, the variance pass, n_iter Lloyd steps and the final assignment")

    nv, per = 100, 3000
    xv = x[:nv * per] if n >= nv * per else descriptors(nv * per, D, 256, dev, seed=2)
    segs = np.arange(nv + 1, dtype=np.int64) * per
    for k in (256, 4096):
        centres = xv[torch.as_tensor(rng.permutation(nv * per)[:k], device=dev)].double()
        t = [timed(lambda: codebook.bow_encode(xv, segs, centres))[1] for _ in range(args.warmup + args.reps)][args.warmup:]
        report("bow_encode_ms", t, 2.0 * nv * per * k * D, 4.0 * nv * per * D + 8.0 * nv * per + 4.0 * nv * k, videos=nv, points_per_video=per,
               d=D, k=k)

    if args.host:
        try:
            from sklearn.cluster import KMeans
        except ImportError:
            print(json.dumps(dict(metric="host_sklearn", note="scikit-learn is not installed here")), flush=True)
            return
        rows = n // 10
        hx = x[:rows].double().cpu().numpy()
        t0 = time.perf_counter()
        km = KMeans(n_clusters=256, n_init=1, random_state=0).fit(hx)
        print(json.dumps(dict(metric="host_sklearn", rows=rows, d=D, k=256, kmeans_fit_s=round(time.perf_counter() - t0, 3), n_iter=int(km.n_iter_),
                              threads=os.environ.get("OMP_NUM_THREADS"),
                              note="a host figure at a tenth of the rows, one unrepeated run: not a like-for-like race")), flush=True)


if __name__ == "__main__":
    main()
