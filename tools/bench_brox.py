"""The cost of Brox optical flow on one MI355X.  Prints one JSON line per measurement.

    python tools/bench_brox.py [--clips 32] [--reps 5] [--warmup 1]

  brox_flow_ms         ``flow.tvl1_flow_concurrent`` (two streams, the benchmark's way) of --clips clips x 11 frames at
                       224x224 with a BroxParams at the defaults (named here value by value) against TV-L1's fixed
                       5 x 5 x 300, interleaved in one process; HIP events around the whole call, median of --reps.
  brox_inner_step_ms   ``va_brox_inner_step`` alone (the coefficients and solver_iters = 10 sweeps) on --clips x 10 fields of
                       every level of the 224x224 pyramid, with the kernel shape the library picks and, on the tiled levels,
                       with 10 and 2 sweeps per launch: milliseconds, pixel-sweeps per second, launches.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULTS = dict(alpha=0.197, gamma=50.0, scale_step=0.8, omega=1.9, epsilon=1e-3, nscales=16, warps=1, inner_iters=10,
                solver_iters=10)


def timed(fn):
    """fn() between two HIP events on the current stream -> (its result, milliseconds)."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch
    from video_analytics_amd import _ffi, synth
    from video_analytics_amd import flow as vflow
    dev = torch.device("cuda", 0)
    gray = synth.synth_clips(args.clips, seed=0)[1].to(dev)
    pairs = args.clips * (gray.shape[1] - 1)
    params = {"brox": _ffi.default_brox_params(**DEFAULTS),
              "tvl1": _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)}
    out = torch.empty((pairs, 2, 224, 224), dtype=torch.float32, device=dev)
    times = {name: [] for name in params}
    finite = {}
    for i in range(args.warmup + args.reps):  # interleaved: brox, tvl1, brox, ...
        for name in params:
            _, ms = timed(lambda: vflow.tvl1_flow_concurrent(gray, params[name], 2, out=out))
            finite[name] = bool(torch.isfinite(out).all().item())
            if i >= args.warmup:
                times[name].append(ms)
    sizes = vflow.pyramid_sizes(224, 224, params["brox"])
    sweeps = sum(w * h for w, h in sizes) * DEFAULTS["warps"] * DEFAULTS["inner_iters"] * DEFAULTS["solver_iters"]
    row = {}
    for name, ms in times.items():
        row[name + "_ms"] = round(statistics.median(ms), 3)
        row[name + "_ms_all"] = [round(t, 3) for t in ms]
    print(json.dumps(dict(metric="brox_flow_ms", clips=args.clips, pairs=pairs, reps=args.reps, brox=DEFAULTS, levels=len(sizes),
                          pixel_sweeps_per_pair=sweeps, tvl1="300 iters x 5 warps x 5 scales, exact math", streams=2, finite=finite,
                          brox_over_tvl1=round(row["brox_ms"] / row["tvl1_ms"], 4), **row)), flush=True)

    L, ctx = _ffi.lib(), _ffi.ctx(0)
    for (w, h) in sizes:
        n = pairs
        g = torch.Generator(device=dev).manual_seed(w)
        f = [torch.randn((n, h, w), device=dev, generator=g) * s for s in (0.05, 0.05, 0.02, 0.02, 0.02, 0.05, 0.02, 0.02, 1.5, 1.5)]
        du, dv = torch.zeros((n, h, w), device=dev), torch.zeros((n, h, w), device=dev)
        scratch = torch.empty(4 * n * h * w, device=dev)
        shapes = [("library", {})]
        if ((w + 1) // 2) * h > 3072:  # tiled by default: the other sweep depths
            shapes += [("K10", dict(sweeps_per_launch=10)), ("K2", dict(sweeps_per_launch=2))]
        for label, tune in shapes:
            p = _ffi.default_brox_params(**dict(DEFAULTS, **tune))

            def step():
                _ffi.check(L.va_brox_inner_step(ctx, *[_ffi.ptr(f[0])] * 3, *[_ffi.ptr(t) for t in f], _ffi.ptr(du), _ffi.ptr(dv), n, w, h,
                                                ctypes.byref(p), _ffi.ptr(scratch), scratch.numel() * 4, _ffi.stream_ptr(dev)))
            ms = []
            for i in range(args.warmup + args.reps):
                du.zero_()
                dv.zero_()
                t = timed(step)[1]
                if i >= args.warmup:
                    ms.append(t)
            med = statistics.median(ms)
            print(json.dumps(dict(metric="brox_inner_step_ms", width=w, height=h, fields=n, shape=label, solver_iters=10,
                                  ms=round(med, 4), ms_all=[round(t, 4) for t in ms],
                                  gpixel_sweeps_per_s=round(n * w * h * 10 / med / 1e6, 2),
                                  finite=bool(torch.isfinite(du).all().item()))), flush=True)


if __name__ == "__main__":
    main()
