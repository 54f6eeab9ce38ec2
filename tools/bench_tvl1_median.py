"""The cost of the median option of TV-L1 on one MI355X.  Prints one JSON line per measurement.

    python tools/bench_tvl1_median.py [--clips 32] [--reps 5] [--warmup 1] [--fields 320]

  tvl1_median_flow_ms    ``flow.tvl1_flow_concurrent`` (two streams, the benchmark's way) of --clips clips x 11 frames at
                         224x224, fixed 5 x 5 x 300, with the option off and with (median, median_every) = (5, 30) -- the
                         defaults of OpenCV's CPU class --, (5, 0) and (3, 30).  The variants are interleaved in one process;
                         HIP events around the whole call, median of --reps.
  flow_median_alone_ms   ``flow.median_filter`` (va_flow_median) alone on --fields fields of 224x224, both sizes, with the
                         bytes it moves (every plane read once and written once) and the rate they give.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = (("off", 0, 0), ("m5_e30", 5, 30), ("m5_e0", 5, 0), ("m3_e30", 3, 30))


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


def medians(times):
    row = {}
    for name, ms in times.items():
        row[name + "_ms"] = round(statistics.median(ms), 3)
        row[name + "_ms_all"] = [round(t, 3) for t in ms]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--fields", type=int, default=320)
    args = ap.parse_args()
    import torch
    from video_analytics_amd import _ffi, synth
    from video_analytics_amd import flow as vflow
    dev = torch.device("cuda", 0)
    gray = synth.synth_clips(args.clips, seed=0)[1].to(dev)
    params = {name: _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5, median=m, median_every=e)
              for name, m, e in VARIANTS}
    out = torch.empty((args.clips * (gray.shape[1] - 1), 2, 224, 224), dtype=torch.float32, device=dev)
    times = {name: [] for name, _, _ in VARIANTS}
    for i in range(args.warmup + args.reps):  # interleaved: off, (5,30), (5,0), (3,30), off, ...
        for name, _, _ in VARIANTS:
            _, ms = timed(lambda: vflow.tvl1_flow_concurrent(gray, params[name], 2, out=out))
            if i >= args.warmup:
                times[name].append(ms)
    row = medians(times)
    for name, _, _ in VARIANTS[1:]:
        row[name + "_over_off"] = round(statistics.median(times[name]) / statistics.median(times["off"]), 4)
    print(json.dumps(dict(metric="tvl1_median_flow_ms", clips=args.clips, pairs=out.shape[0], reps=args.reps,
                          tvl1="300 iters x 5 warps x 5 scales, exact math, two streams", finite=bool(torch.isfinite(out).all().item()),
                          **row)), flush=True)

    field = torch.randn((args.fields, 2, 224, 224), dtype=torch.float32, device=dev)
    dst = torch.empty_like(field)
    times = {"k3": [], "k5": []}
    for i in range(args.warmup + args.reps):
        for name, k in (("k3", 3), ("k5", 5)):
            _, ms = timed(lambda: vflow.median_filter(field, k, out=dst))
            if i >= args.warmup:
                times[name].append(ms)
    row = medians(times)
    nbytes = 2 * field.numel() * 4
    for name in times:
        row[name + "_GBps"] = round(nbytes / statistics.median(times[name]) / 1e6, 1)
    print(json.dumps(dict(metric="flow_median_alone_ms", fields=args.fields, height=224, width=224, reps=args.reps,
                          bytes_moved=nbytes, **row)), flush=True)


if __name__ == "__main__":
    main()
