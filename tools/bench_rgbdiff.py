"""Timings of the RGB-difference input.  Prints one JSON line per measurement.

    python tools/bench_rgbdiff.py gather [--items 250 24 63] [--reps 20]
    python tools/bench_rgbdiff.py video  [--frames 150] [--dtypes f32 bf16] [--reps 3]
    python tools/bench_rgbdiff.py train  [--videos 8] [--segments 3] [--frames 150] [--reps 3]

``gather``: ``va_rgbdiff_to_stack`` (kernel ``k_rgbdiff_stack``) per item count n at 320x240 and D = 5, beside
``va_flow_to_stack_crop`` (kernel ``k_flow_crop_stack``) writing the same number of output bytes, interleaved in one
process; HIP-event time per call, median over the repetitions.  250 items are the 25 snippets x ten views of
``run_video`` (a view table over one 150-frame video, read in place); the other counts are training batches
(scale-jitter crops over the windows' frames laid out one after the other).  For the kernels' own times run it under the
profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_rgbdiff.py gather
and read the rows of ``k_rgbdiff_stack`` and ``k_flow_crop_stack``.
``video``: ``run_video`` (25 snippets, ten views, full 5 x 5 x 300 TV-L1 schedule) of a pipeline with the third stream and of
one without, interleaved.  ``train``: one ``train_videos`` step of n videos, with and without, interleaved.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _wall_s(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _stats(prefix, xs, digits=4):
    return {prefix: round(statistics.median(xs), digits), prefix + "_min": round(min(xs), digits),
            prefix + "_max": round(max(xs), digits)}


def gather(args):
    import torch
    from video_analytics_amd import augment, rgbdiff, video
    from video_analytics_amd import flow as vflow
    from video_analytics_amd.parameters import VIDEO_INPUT_FLOW_COUNT as L
    H, W, D = args.height, args.width, args.diffs
    dev = torch.device("cuda", 0)
    for n in args.items:
        rng = random.Random(n)
        g = torch.Generator(device=dev).manual_seed(n)
        if n == 250:  # the video path: 25 snippets x ten views of one 150-frame video
            frames = torch.randint(0, 256, (150, 3, H, W), generator=g, dtype=torch.uint8, device=dev)
            table = rgbdiff.view_table(video.snippetStarts(150, L, 25), augment.ten_crop_views(H, W))
        else:         # the training path: n windows of D + 1 frames, one scale-jitter crop each
            frames = torch.randint(0, 256, (n * (D + 1), 3, H, W), generator=g, dtype=torch.uint8, device=dev)
            table = rgbdiff.window_table([i * (D + 1) for i in range(n)], augment.draw_scale_jitter_crops(n, H, W, rng))
        planes = n * 3 * D
        pairs = (planes + 1) // 2  # the flow gather writes whole pairs: one plane more when the count is odd
        fl = torch.randn((pairs, 2, H, W), generator=g, device=dev) * 12.0
        crops = augment.draw_flow_crops(1, pairs, H, W, rng=rng)
        out_d = torch.empty((n, 3 * D, 224, 224), device=dev)
        out_f = torch.empty((2 * pairs, 224, 224), device=dev)
        runs = dict(rgbdiff=lambda: rgbdiff.rgb_diff_stack(frames, table, D, out=out_d),
                    flow_crop=lambda: vflow.crop_flow_to_stack(fl, crops, out=out_f))
        ms = dict((k, []) for k in runs)
        for i in range(args.warmup + args.reps):  # interleaved
            for k, fn in runs.items():
                dt, _ = _event_ms(fn)
                if i >= args.warmup:
                    ms[k].append(dt)
        row = dict(metric="gather_ms_per_call", items=n, diffs=D, height=H, width=W, reps=args.reps,
                   rgbdiff_out_mb=round(out_d.numel() * 4 / 1e6, 1), flow_crop_out_mb=round(out_f.numel() * 4 / 1e6, 1),
                   kernels=["k_rgbdiff_stack", "k_flow_crop_stack"])
        for k, v in ms.items():
            row.update(_stats(k + "_ms", v))
        row["rgbdiff_write_gb_per_s"] = round(out_d.numel() * 4 / 1e6 / statistics.median(ms["rgbdiff"]), 1)
        row["flow_crop_write_gb_per_s"] = round(out_f.numel() * 4 / 1e6 / statistics.median(ms["flow_crop"]), 1)
        print(json.dumps(row), flush=True)


def video_mode(args):
    import torch
    from video_analytics_amd import _ffi, augment, pipeline, synth
    H, W, T = args.height, args.width, args.frames
    dev = torch.device("cuda", 0)
    params = _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)
    views = augment.ten_crop_views(H, W)
    _, gray, _ = synth.synth_clips(1, seed=T, H=H, W=W, n_gray=T, device="cuda")
    gray = gray[0].contiguous()
    rgb = torch.randint(0, 256, (T, 3, H, W), generator=torch.Generator(device=dev).manual_seed(T), dtype=torch.uint8, device=dev)
    for dtype in args.dtypes:
        pipes = dict(with_diff=pipeline.TwoStreamPipeline(device=0, tvl1_params=params, cnn_dtype=dtype, rgb_diff=True,
                                                          rgb_diff_count=args.diffs),
                     without=pipeline.TwoStreamPipeline(device=0, tvl1_params=params, cnn_dtype=dtype))
        s = dict((k, []) for k in pipes)
        for i in range(args.warmup + args.reps):  # interleaved
            for k, pipe in pipes.items():
                dt, out = _wall_s(lambda: pipe.run_video(rgb, gray, n_snippets=args.snippets, views=(views, views)))
                if i >= args.warmup:
                    s[k].append(dt)
        row = dict(metric="run_video_s", frames=T, height=H, width=W, snippets=args.snippets, views=10, cnn_dtype=dtype,
                   diffs=args.diffs, reps=args.reps, finite=bool(torch.isfinite(out["scores"]).all().item()),
                   tvl1="300 iters x 5 warps x 5 scales, exact math")
        for k, v in s.items():
            row.update(_stats(k + "_s", v))
        row["ratio"] = round(statistics.median(s["with_diff"]) / statistics.median(s["without"]), 4)
        print(json.dumps(row), flush=True)
        for pipe in pipes.values():
            pipe.close()


def train_mode(args):
    import torch
    from video_analytics_amd import _ffi, pipeline, synth
    H, W, T, n, k = args.height, args.width, args.frames, args.videos, args.segments
    dev = torch.device("cuda", 0)
    params = _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)
    vids = []
    for v in range(n):
        _, gray, _ = synth.synth_clips(1, seed=100 + v, H=H, W=W, n_gray=T, device="cuda")
        rgb = torch.randint(0, 256, (T, 3, H, W), generator=torch.Generator(device=dev).manual_seed(v), dtype=torch.uint8,
                            device=dev)
        vids.append((rgb, gray[0].contiguous()))
    labels = torch.arange(n) % 101
    pipes = dict(with_diff=pipeline.TwoStreamPipeline(device=0, tvl1_params=params, rgb_diff=True, rgb_diff_count=args.diffs),
                 without=pipeline.TwoStreamPipeline(device=0, tvl1_params=params))
    s = dict((key, []) for key in pipes)
    for i in range(args.warmup + args.reps):  # interleaved; both draw the same starts and crops
        for key, pipe in pipes.items():
            dt, out = _wall_s(lambda: pipe.train_videos(vids, labels, k=k, lr=1e-4, rng=random.Random(i)))
            if i >= args.warmup:
                s[key].append(dt)
    row = dict(metric="train_videos_s", videos=n, segments=k, frames=T, height=H, width=W, diffs=args.diffs, reps=args.reps,
               finite=bool(torch.isfinite(out["stats_s"]).all().item()), tvl1="300 iters x 5 warps x 5 scales, exact math")
    for key, v in s.items():
        row.update(_stats(key + "_s", v))
    row["ratio"] = round(statistics.median(s["with_diff"]) / statistics.median(s["without"]), 4)
    print(json.dumps(row), flush=True)
    for pipe in pipes.values():
        pipe.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gather", "video", "train"])
    ap.add_argument("--items", type=int, nargs="+", default=[250, 24, 63])
    ap.add_argument("--diffs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--snippets", type=int, default=25)
    ap.add_argument("--dtypes", nargs="+", choices=["f32", "bf16"], default=["f32", "bf16"])
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 20 if args.mode == "gather" else 3
    if args.warmup is None:
        args.warmup = 3 if args.mode == "gather" else 1

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_rgbdiff.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    dict(gather=gather, video=video_mode, train=train_mode)[args.mode](args)


if __name__ == "__main__":
    main()
