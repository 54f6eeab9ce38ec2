"""Timings of TSN training: the crop-resize gathers next to the plain crop gathers, the consensus step
next to the plain step, and videos/s of ``TwoStreamPipeline.train_videos``.  Prints one JSON line per measurement.

    python tools/bench_train_tsn.py gathers [--snippets 24 63] [--reps 20]
    python tools/bench_train_tsn.py step    [--videos 8] [--segments 3] [--reps 5]
    python tools/bench_train_tsn.py videos  [--videos 8] [--segments 3] [--frames 150] [--reps 3]

``gathers``: per snippet count n, ``va_flow_to_stack_resize`` (n x 2L planes) and ``va_resize_images_u8`` (n images) with drawn
scale-jitter crops of 320x240 frames, interleaved with ``va_flow_to_stack_crop`` and ``va_crop_images_u8`` at the same output
size; HIP-event time per call, median over the repetitions.  For the kernels' own times run it under the profiler, in a run
of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_train_tsn.py gathers
``step``: ``train_step_consensus`` (n videos x k snippets) and ``train_step`` at the same batch, interleaved, both streams.
``videos``: one ``train_videos`` step of n videos of T frames at 320x240, k segments, full 5 x 5 x 300 TV-L1 schedule.
"""
import argparse
import json
import os
import random
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


def gathers(args):
    import torch
    from video_analytics_amd import augment
    from video_analytics_amd import flow as vflow
    from video_analytics_amd.parameters import VIDEO_INPUT_FLOW_COUNT as L
    H, W = args.height, args.width
    dev = torch.device("cuda", 0)
    for n in args.snippets:
        rng = random.Random(n)
        g = torch.Generator(device=dev).manual_seed(n)
        fl = torch.randn((n * L, 2, H, W), generator=g, device=dev) * 12.0
        rgb = torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8, device=dev)
        crops = augment.draw_scale_jitter_crops(n, H, W, rng)
        rgb_table, flow_table = augment.snippet_tables(crops, list(range(n)), [i * L for i in range(n)], L)
        flow_crops = augment.draw_flow_crops(n, L, H, W, mode="shared", rng=rng)
        rgb_crops = augment.draw_image_crops(n, H, W, rng=rng)
        out_f = torch.empty((n * 2 * L, 224, 224), device=dev)
        runs = dict(flow_resize=lambda: vflow.resize_flow_to_stack(fl, flow_table, out=out_f),
                    flow_crop=lambda: vflow.crop_flow_to_stack(fl, flow_crops, out=out_f),
                    images_resize=lambda: augment.resize_images(rgb, rgb_table),
                    images_crop=lambda: augment.crop_images(rgb, rgb_crops))
        ms = dict((k, []) for k in runs)
        for i in range(args.warmup + args.reps):  # interleaved
            for k, fn in runs.items():
                dt, _ = _event_ms(fn)
                if i >= args.warmup:
                    ms[k].append(dt)
        row = dict(metric="gather_ms_per_call", snippets=n, height=H, width=W, flow_planes=n * 2 * L, reps=args.reps,
                   flow_out_mb=round(n * 2 * L * 224 * 224 * 4 / 1e6, 1))
        row.update(dict((k + "_ms", _med(v)) for k, v in ms.items()))
        row.update(dict((k + "_ms_min", round(min(v), 4)) for k, v in ms.items()))
        print(json.dumps(row), flush=True)


def step(args):
    import torch
    from video_analytics_amd import pipeline, vgg
    from video_analytics_amd.parameters import NACTION_CLASSES, VIDEO_DESCRIPTOR_DIM, VIDEO_INPUT_FLOW_COUNT as L
    dev = torch.device("cuda", 0)
    n, k = args.videos, args.segments
    B = n * k
    for c_in, name in ((3, "spatial"), (2 * L, "temporal")):
        w = pipeline.build_stream_weights(c_in, 1, dev)
        m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], NACTION_CLASSES, VIDEO_DESCRIPTOR_DIM)
        g = torch.Generator(device=dev).manual_seed(c_in)
        x = torch.randn((B, c_in, 224, 224), generator=g, device=dev)
        y_img = (torch.arange(B, device=dev) % NACTION_CLASSES).long()
        y_vid = (torch.arange(n, device=dev) % NACTION_CLASSES).long()
        plain, cons = [], []
        for i in range(args.warmup + args.reps):  # interleaved; lr = 0 keeps the weights where they are
            dt, _ = _event_ms(lambda: m.train_step(x, y_img, 0.0, 0.9, i))
            if i >= args.warmup:
                plain.append(dt)
            dt, out = _event_ms(lambda: m.train_step_consensus(x, y_vid, k, 0.0, 0.9, i))
            if i >= args.warmup:
                cons.append(dt)
        print(json.dumps(dict(metric="train_step_ms", stream=name, batch=B, videos=n, segments=k, reps=args.reps,
                              plain_ms=_med(plain), plain_ms_min=round(min(plain), 4), plain_ms_max=round(max(plain), 4),
                              consensus_ms=_med(cons), consensus_ms_min=round(min(cons), 4),
                              consensus_ms_max=round(max(cons), 4), finite=bool(torch.isfinite(out[0]).all().item()))),
              flush=True)
        m.close()


def videos(args):
    import time
    import torch
    from video_analytics_amd import _ffi, pipeline, synth
    dev = torch.device("cuda", 0)
    n, k, T, H, W = args.videos, args.segments, args.frames, args.height, args.width
    params = _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    vids = []
    for v in range(n):
        _, gray, _ = synth.synth_clips(1, seed=100 + v, H=H, W=W, n_gray=T, device="cuda")
        g = torch.Generator(device=dev).manual_seed(v)
        vids.append((torch.randint(0, 256, (T, 3, H, W), generator=g, dtype=torch.uint8, device=dev), gray[0].contiguous()))
    labels = [v % 101 for v in range(n)]
    rng = random.Random(0)
    ts, pairs = [], 0
    for i in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe.train_videos(vids, labels, k=k, lr=1e-5, dropout_seed=i, rng=rng)
        torch.cuda.synchronize()
        if i >= args.warmup:
            ts.append(time.perf_counter() - t0)
        pairs = sum(p.pair_computations for p in out["plans"])
    print(json.dumps(dict(metric="train_videos_per_s", videos=n, segments=k, frames=T, height=H, width=W, tvl1_pairs=pairs,
                          reps=args.reps, step_s=_med(ts), step_s_min=round(min(ts), 4), step_s_max=round(max(ts), 4),
                          videos_per_s=round(n / statistics.median(ts), 3),
                          finite=bool(torch.isfinite(out["stats_s"]).all().item() and torch.isfinite(out["stats_t"]).all().item()),
                          tvl1="300 iters x 5 warps x 5 scales, exact math")), flush=True)
    pipe.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gathers", "step", "videos"])
    ap.add_argument("--snippets", type=int, nargs="+", default=[24, 63])
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.reps is None:
        args.reps = dict(gathers=20, step=5, videos=3)[args.mode]
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_train_tsn.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    dict(gathers=gathers, step=step, videos=videos)[args.mode](args)


if __name__ == "__main__":
    main()
