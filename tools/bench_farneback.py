"""The cost of Farneback optical flow on one MI355X.  Prints one JSON line per measurement.

    python tools/bench_farneback.py [--clips 32] [--reps 5] [--warmup 1]

  farneback_flow_ms     ``flow.tvl1_flow_concurrent`` (two streams, the benchmark's way) of --clips clips x 11 frames at
                        224x224 with a FarnebackParams at the defaults (named here value by value) against Brox at its
                        defaults and TV-L1's fixed 5 x 5 x 300, interleaved in one process; HIP events around the whole
                        call, median of --reps.
  farneback_polyexp_ms  ``va_farneback_polyexp`` alone on --clips x 11 fields of every level of the 224x224 pyramid, per tile
                        shape: milliseconds and pixels per second.
  farneback_pass_ms     ``va_farneback_pass`` alone (one pass, winsize 15, box window) on --clips x 10 pairs of every level,
                        on coefficients of real frames and a flow of about 1.5 px, per tile shape.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULTS = dict(pyr_scale=0.5, poly_sigma=1.2, levels=3, winsize=15, iterations=3, poly_n=5, gaussian=0)
BROX = dict(alpha=0.197, gamma=50.0, scale_step=0.8, omega=1.9, epsilon=1e-3, nscales=16, warps=1, inner_iters=10, solver_iters=10)
TILES = [(0, 0), (16, 16), (32, 8), (32, 32), (64, 8), (64, 16), (64, 32), (128, 8)]  # (0, 0): the library's own


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
    params = {"farneback": _ffi.default_farneback_params(**DEFAULTS), "brox": _ffi.default_brox_params(**BROX),
              "tvl1": _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)}
    out = torch.empty((pairs, 2, 224, 224), dtype=torch.float32, device=dev)
    times = {name: [] for name in params}
    finite = {}
    for i in range(args.warmup + args.reps):  # interleaved: farneback, brox, tvl1, farneback, ...
        for name in params:
            _, ms = timed(lambda: vflow.tvl1_flow_concurrent(gray, params[name], 2, out=out))
            finite[name] = bool(torch.isfinite(out).all().item())
            if i >= args.warmup:
                times[name].append(ms)
    sizes = vflow.pyramid_sizes(224, 224, params["farneback"])
    row = {}
    for name, ms in times.items():
        row[name + "_ms"] = round(statistics.median(ms), 3)
        row[name + "_ms_all"] = [round(t, 3) for t in ms]
    print(json.dumps(dict(metric="farneback_flow_ms", clips=args.clips, pairs=pairs, reps=args.reps, farneback=DEFAULTS, brox=BROX,
                          levels=len(sizes), tvl1="300 iters x 5 warps x 5 scales, exact math", streams=2, finite=finite,
                          farneback_over_brox=round(row["farneback_ms"] / row["brox_ms"], 4),
                          farneback_over_tvl1=round(row["farneback_ms"] / row["tvl1_ms"], 4), **row)), flush=True)

    L, ctx = _ffi.lib(), _ffi.ctx(0)
    frames = gray.float()
    for (w, h) in sizes:
        # the level's frames: a plain resize is enough for a timing (S1 is not what is measured here)
        fr = frames if w == 224 else torch.nn.functional.interpolate(frames, size=(h, w), mode="bilinear", align_corners=False)
        fr = fr.contiguous()
        n = fr.shape[0] * fr.shape[1]
        coef = torch.empty((n, 5, h, w), device=dev)
        for (tw, th) in TILES:
            p = _ffi.default_farneback_params(**dict(DEFAULTS, poly_tile_w=tw, poly_tile_h=th))

            def expand():
                _ffi.check(L.va_farneback_polyexp(ctx, _ffi.ptr(fr), n, w, h, ctypes.byref(p), _ffi.ptr(coef), _ffi.stream_ptr(dev)))
            ms = [timed(expand)[1] for _ in range(args.warmup + args.reps)][args.warmup:]
            med = statistics.median(ms)
            print(json.dumps(dict(metric="farneback_polyexp_ms", width=w, height=h, fields=n, tile=[tw, th], poly_n=DEFAULTS["poly_n"],
                                  ms=round(med, 4), ms_all=[round(t, 4) for t in ms], gpixels_per_s=round(n * w * h / med / 1e6, 2),
                                  finite=bool(torch.isfinite(coef).all().item()))), flush=True)
        c = coef.view(fr.shape[0], fr.shape[1], 5, h, w)
        c0, c1 = c[:, :-1].reshape(-1, 5, h, w).contiguous(), c[:, 1:].reshape(-1, 5, h, w).contiguous()
        g = torch.Generator(device=dev).manual_seed(w)
        fin = torch.randn((pairs, 2, h, w), device=dev, generator=g) * 1.5
        fout = torch.empty_like(fin)
        for (tw, th) in TILES:
            p = _ffi.default_farneback_params(**dict(DEFAULTS, pass_tile_w=tw, pass_tile_h=th))

            def one_pass():
                _ffi.check(L.va_farneback_pass(ctx, _ffi.ptr(c0), _ffi.ptr(c1), _ffi.ptr(fin), _ffi.ptr(fout), pairs, w, h, ctypes.byref(p),
                                               _ffi.stream_ptr(dev)))
            ms = [timed(one_pass)[1] for _ in range(args.warmup + args.reps)][args.warmup:]
            med = statistics.median(ms)
            print(json.dumps(dict(metric="farneback_pass_ms", width=w, height=h, pairs=pairs, tile=[tw, th], winsize=DEFAULTS["winsize"],
                                  ms=round(med, 4), ms_all=[round(t, 4) for t in ms], gpixels_per_s=round(pairs * w * h / med / 1e6, 2),
                                  finite=bool(torch.isfinite(fout).all().item()))), flush=True)


if __name__ == "__main__":
    main()
