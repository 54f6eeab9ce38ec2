"""The fusion SVM's fit on one MI355X against ``LinearSVC().fit`` on the same machine's host.  Prints one
JSON line per shape.

    python tools/bench_svm_fit.py [--shapes descriptors scores] [--n 9537] [--classes 101] [--reps 5] [--warmup 1] [--no-host]

``descriptors``: synthetic post-ReLU descriptors ``max(0, 0.3 mu_class + N(0,1))``, ``[n, 512]`` float32 on the device (what
``video.evaluateVideos`` hands over); ``scores``: the stacked softmax scores of two streams, ``[n, 2 classes]``.  Reported:
milliseconds of ``fusion.linear_svm_fit`` (HIP events around the whole Python call, its statistics reads included; median,
min and max of --reps after --warmup), the Newton steps and the CG steps (largest per class row, and summed over the rows),
the seconds of ``LinearSVC()`` with its defaults on the host, and for both solutions the largest
``|grad f_r| / |grad f_r(0)|`` over the class rows, recomputed here in numpy float64."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(shape, n, k, seed=0):
    """-> (X float32 [n, d], labels int64 [n]); every class present."""
    rng = np.random.RandomState(seed)
    labels = np.concatenate([np.arange(k), rng.randint(0, k, size=n - k)])[rng.permutation(n)]
    if shape == "descriptors":
        mu = rng.randn(k, 512)
        return np.maximum(0.0, 0.3 * mu[labels] + rng.randn(n, 512)).astype(np.float32), labels
    streams = []
    for _ in range(2):  # softmax scores of a stream that is right about two times in three
        logits = rng.randn(n, k)
        hit = rng.rand(n) < 0.67
        guess = np.where(hit, labels, rng.randint(0, k, size=n))
        logits[np.arange(n), guess] += 4.0
        e = np.exp(logits - logits.max(1, keepdims=True))
        streams.append(e / e.sum(1, keepdims=True))
    return np.concatenate(streams, axis=1).astype(np.float32), labels


def rel_gradient(coef, intercept, X, labels, classes, C=1.0):
    """max_r |grad f_r(w)| / |grad f_r(0)| in float64, f_r the squared-hinge objective with the regularised bias."""
    Xa = np.concatenate([X.astype(np.float64), np.ones((X.shape[0], 1))], axis=1)
    pos = classes[1:] if len(classes) == 2 else classes
    Y = np.where(labels[None, :] == pos[:, None], 1.0, -1.0)
    W = np.concatenate([np.atleast_2d(coef), np.atleast_1d(intercept)[:, None]], axis=1)
    m = W @ Xa.T
    g = W + 2.0 * C * (np.where(1.0 - Y * m > 0.0, m - Y, 0.0) @ Xa)
    g0 = 2.0 * C * ((-Y) @ Xa)
    return float((np.linalg.norm(g, axis=1) / np.linalg.norm(g0, axis=1)).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", choices=["descriptors", "scores"], default=["descriptors", "scores"])
    ap.add_argument("--n", type=int, default=9537)
    ap.add_argument("--classes", type=int, default=101)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--no-host", action="store_true", help="skip LinearSVC().fit on the host")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_svm_fit.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    from video_analytics_amd import fusion
    for shape in args.shapes:
        X, labels = synthetic(shape, args.n, args.classes)
        xd = torch.as_tensor(X).cuda()
        ms, wall = [], []
        for i in range(args.warmup + args.reps):
            beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            beg.record()
            coef, intercept, classes, info = fusion.linear_svm_fit(xd, labels, tol=args.tol, return_info=True)
            end.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms.append(beg.elapsed_time(end))
                wall.append(1e3 * (time.perf_counter() - t0))
        row = dict(metric="svm_fit", shape=shape, n=int(X.shape[0]), dim=int(X.shape[1]), classes=args.classes, tol=args.tol, reps=args.reps,
                   device_ms=round(statistics.median(ms), 2), device_ms_min=round(min(ms), 2), device_ms_max=round(max(ms), 2),
                   device_wall_ms=round(statistics.median(wall), 2), converged=bool(info["converged"]), newton_steps=int(info["n_iter"]),
                   newton_steps_sum=int(info["steps"].sum()), cg_steps_max=int(info["cg_steps"].max()), cg_steps_sum=int(info["cg_steps"].sum()),
                   device_rel_grad=rel_gradient(coef, intercept, X, labels, classes))
        print(json.dumps(dict(row, partial="device only")), flush=True)
        if not args.no_host:
            from sklearn import svm
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                t0 = time.perf_counter()
                clf = svm.LinearSVC().fit(X.astype(np.float64), labels)
                row["host_linearsvc_s"] = round(time.perf_counter() - t0, 2)
            row["host_converged"] = not any("converge" in str(w.message).lower() for w in caught)
            row["host_n_iter"] = int(np.max(clf.n_iter_))
            row["host_rel_grad"] = rel_gradient(clf.coef_, clf.intercept_, X, labels, clf.classes_)
            row["speedup"] = round(1e3 * row["host_linearsvc_s"] / row["device_ms"], 1)
            row["predictions_differ"] = int((fusion.linear_svm_predict(X, coef, intercept, classes)
                                             != fusion.linear_svm_predict(X, clf.coef_, clf.intercept_, clf.classes_)).sum())
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
