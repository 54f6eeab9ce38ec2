"""The cost of PCA, mixture fitting and Fisher-vector encoding on one MI355X.  One JSON line per measurement.

    python tools/bench_fisher.py [--rows 1000000] [--reps 5] [--warmup 1] [--host]

  pca_moments_ms, pca_transform_ms   ``va_pca_moments`` and ``va_pca_transform`` at --rows x 426 -> 64
  gmm_stats_ms                       one ``va_gmm_stats`` pass at --rows x 64, K = 256 (the E-step of a fit)
  gmm_fit_ms                         a whole ``fisher.gmm_fit`` at that shape with its iteration count (one run: it is long)
  fisher_vectors_ms                  ``fisher.fisher_vectors`` for 100 videos of 26,000 rows

HIP events around each call, median of --reps with the range.  Beside each time stand the float64 FLOP/s it amounts to, next
to the device's float64 matrix peak (78.6 TFLOP/s, the vendor's figure), and the bytes that must cross memory at least once
(every input read once per kernel that needs it, every output written once; the responsibilities of a statistics pass written
once and read once), next to the HBM peak of 8 TB/s (6.29 TB/s is what a copy reaches): which bound a pass obeys shows there.

--host adds scikit-learn on the host, where it is installed: ``PCA.fit`` and ONE ``GaussianMixture`` EM iteration at 100,000
rows -- a tenth of the rows, a host figure to set the scale, not a like-for-like race.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_MATRIX_PEAK_TFLOPS, HBM_PEAK_TBS, HBM_COPY_TBS = 78.6, 8.0, 6.29
D_DESC, D_PCA, K = 426, 64, 256


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
                          tb_per_s=round(nbytes / med / 1e9, 3), hbm_peak_tb_per_s=HBM_PEAK_TBS, hbm_copy_tb_per_s=HBM_COPY_TBS, **more)),
          flush=True)


def mixture(n, d, k, dev, seed=0):
    """float32 rows [n,d] on the device drawn from k diagonal Gaussians, and those Gaussians"""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    mu = torch.randn((k, d), generator=g, device=dev, dtype=torch.float32) * 2.0
    sd = 0.5 + torch.rand((k, d), generator=g, device=dev, dtype=torch.float32)
    z = torch.randint(0, k, (n,), generator=g, device=dev)
    x = mu[z] + torch.randn((n, d), generator=g, device=dev, dtype=torch.float32) * sd[z]
    w = torch.full((k,), 1.0 / k, dtype=torch.float64, device=dev)
    return x.contiguous(), w, mu.double(), (sd * sd).double()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from video_analytics_amd import _ffi, fisher
    dev = torch.device("cuda", 0)
    n = args.rows

    def reps(fn):
        return [timed(fn)[1] for _ in range(args.warmup + args.reps)][args.warmup:]

    # PCA at n x 426 -> 64
    g = torch.Generator(device=dev).manual_seed(1)
    desc = torch.rand((n, D_DESC), generator=g, device=dev, dtype=torch.float32)
    L, ctx, st = _ffi.lib(), _ffi.ctx(0), _ffi.stream_ptr(dev)
    need = L.va_pca_workspace_bytes(n, D_DESC)
    ws = torch.empty((need // 8,), dtype=torch.float64, device=dev)
    sums = torch.empty((1 + D_DESC + D_DESC * D_DESC,), dtype=torch.float64, device=dev)
    t = reps(lambda: _ffi.check(L.va_pca_moments(ctx, _ffi.ptr(desc), n, D_DESC, 1, _ffi.ptr(sums), _ffi.ptr(ws), need, st)))
    report("pca_moments_ms", t, 2.0 * n * (D_DESC + 1) * (D_DESC + 2) / 2, 4.0 * n * D_DESC,
           rows=n, d=D_DESC, chunk_rows=L.va_pca_chunk_rows(n, D_DESC), workspace_mb=round(need / 2 ** 20, 1),
           note="FLOPs: the upper triangle of [X,1]^T [X,1]")
    model = fisher.pca_fit(desc[:200000], D_PCA)
    mean, comp = (torch.as_tensor(a).to(dev) for a in (model.mean, model.components))
    out = torch.empty((n, D_PCA), dtype=torch.float32, device=dev)
    t = reps(lambda: _ffi.check(L.va_pca_transform(ctx, _ffi.ptr(desc), n, D_DESC, _ffi.ptr(mean), _ffi.ptr(comp), D_PCA, _ffi.ptr(out), st)))
    report("pca_transform_ms", t, 2.0 * n * D_DESC * D_PCA, 4.0 * n * (D_DESC + D_PCA), rows=n, d=D_DESC, m=D_PCA)
    del desc, out, ws

    # one statistics pass and a whole fit at n x 64, K = 256
    x, w, mu, var = mixture(n, D_PCA, K, dev)
    seg = np.array([0, n], dtype=np.int64)
    t = reps(lambda: fisher.gmm_stats(x, seg, w, mu, var))
    flops = 2.0 * n * K * (2 * D_PCA) + 2.0 * n * K * (1 + 2 * D_PCA)
    moved = 2 * 4.0 * n * D_PCA + 2 * 8.0 * n * K
    p = _ffi.default_gmm_params()
    report("gmm_stats_ms", t, flops, moved, rows=n, d=D_PCA, k=K, chunk_rows=p.chunk_rows, batch_rows=p.batch_rows,
           workspace_mb=round(L.va_gmm_workspace_bytes(n, D_PCA, K, 1, ctypes.byref(p)) / 2 ** 20, 1))
    fit, ms = timed(lambda: fisher.gmm_fit(x, K, seed=0))
    passes = fit.n_iter + 11  # 10 Lloyd passes, one more hard pass, then one pass per iteration
    report("gmm_fit_ms", [ms], flops * passes, moved * passes, rows=n, d=D_PCA, k=K, n_iter=fit.n_iter, converged=fit.converged,
           passes=passes, lower_bound=fit.lower_bound, ms_per_pass=round(ms / passes, 3))

    # Fisher vectors of 100 videos of 26,000 rows
    nv, per = 100, 26000
    xv = x[:nv * per] if n >= nv * per else mixture(nv * per, D_PCA, K, dev, seed=2)[0]
    segs = np.arange(nv + 1, dtype=np.int64) * per
    t = reps(lambda: fisher.fisher_vectors(xv, segs, fit))
    report("fisher_vectors_ms", t, flops * nv * per / n, moved * nv * per / n, videos=nv, rows_per_video=per, d=D_PCA, k=K,
           vector_length=K + 2 * K * D_PCA)

    if args.host:
        try:
            from sklearn.decomposition import PCA
            from sklearn.mixture import GaussianMixture
        except ImportError:
            print(json.dumps(dict(metric="host_sklearn", note="scikit-learn is not installed here")), flush=True)
            return
        import warnings
        rows = 100000
        hd = np.random.RandomState(0).rand(rows, D_DESC)
        t0 = time.perf_counter()
        PCA(n_components=D_PCA).fit(hd)
        t_pca = time.perf_counter() - t0
        hx = x[:rows].double().cpu().numpy()
        gm = GaussianMixture(K, covariance_type="diag", weights_init=w.cpu().numpy(), means_init=mu.cpu().numpy(),
                             precisions_init=1.0 / var.cpu().numpy(), max_iter=1, tol=0.0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            gm.fit(hx)
            t_em = time.perf_counter() - t0
        print(json.dumps(dict(metric="host_sklearn", rows=rows, pca_fit_s=round(t_pca, 3), gmm_em_iteration_s=round(t_em, 3),
                              threads=os.environ.get("OMP_NUM_THREADS"),
                              note="a host figure at a tenth of the rows, one unrepeated run each: not a like-for-like race")), flush=True)


if __name__ == "__main__":
    main()
