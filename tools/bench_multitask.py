"""Step time of multi-task training: ``train_step_multitask`` with the heads (51, 101) next to
``train_step_consensus`` on the same model of 152 classes, interleaved in one process, both streams.  Prints one JSON line
per stream.

    python tools/bench_multitask.py [--videos 8] [--segments 3] [--heads 51 101] [--reps 5]

The two steps differ in one single-workgroup launch (``k_ce_multitask_fwd_bwd`` against ``k_ce_consensus_fwd_bwd``); HIP-event
time per step, median over the repetitions.  For the kernels' own times run it under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_multitask.py
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _med(xs):
    return round(statistics.median(xs), 4)


def step(args):
    import torch
    from video_analytics_amd import pipeline, vgg
    from video_analytics_amd.parameters import VIDEO_DESCRIPTOR_DIM, VIDEO_INPUT_FLOW_COUNT as L
    dev = torch.device("cuda", 0)
    n, k, heads = args.videos, args.segments, tuple(args.heads)
    B, C = n * k, sum(heads)
    for c_in, name in ((3, "spatial"), (2 * L, "temporal")):
        w = pipeline.build_stream_weights(c_in, 1, dev, C)
        m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], C, VIDEO_DESCRIPTOR_DIM)
        g = torch.Generator(device=dev).manual_seed(c_in)
        x = torch.randn((B, c_in, 224, 224), generator=g, device=dev)
        tasks = (torch.arange(n, device=dev) % len(heads)).int()
        y_local = (torch.arange(n, device=dev) % min(heads)).long()
        y_all = (torch.arange(n, device=dev) % C).long()
        multi, cons = [], []
        for i in range(args.warmup + args.reps):  # interleaved; lr = 0 keeps the weights where they are
            dt, out_m = _event_ms(lambda: m.train_step_multitask(x, y_local, tasks, heads, k, 0.0, 0.9, i))
            if i >= args.warmup:
                multi.append(dt)
            dt, out_c = _event_ms(lambda: m.train_step_consensus(x, y_all, k, 0.0, 0.9, i))
            if i >= args.warmup:
                cons.append(dt)
        print(json.dumps(dict(metric="train_step_ms", stream=name, batch=B, videos=n, segments=k, heads=list(heads), classes=C,
                              reps=args.reps, multitask_ms=_med(multi), multitask_ms_min=round(min(multi), 4),
                              multitask_ms_max=round(max(multi), 4), consensus_ms=_med(cons), consensus_ms_min=round(min(cons), 4),
                              consensus_ms_max=round(max(cons), 4),
                              finite=bool(torch.isfinite(out_m[0]).all().item() and torch.isfinite(out_c[0]).all().item()))),
              flush=True)
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--heads", type=int, nargs="+", default=[51, 101])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_multitask.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    step(args)


if __name__ == "__main__":
    main()
