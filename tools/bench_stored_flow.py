"""Timings of stored optical flow.  Prints one JSON line per measurement.

    python tools/bench_stored_flow.py [--frames 150] [--videos 8] [--segments 3] [--reps 5] [--only video train extract kernels]

Everything runs in one process; the variants of a measurement are interleaved call by call, every call is timed with HIP
events on the current stream (``run_video`` and ``train_videos`` end ordered on it), and the median of ``--reps`` calls is
reported beside the smallest and the largest.  TV-L1 runs its full schedule (300 iterations x 5 warps x 5 scales, exact math).

``video``: ``run_video`` of a 150-frame 320x240 video, 25 snippets x ten views, live against ``flow=`` uint8 and float32.
``train``: one ``train_videos`` step of 8 videos x 3 snippets, live against ``flows=`` uint8 and float32 (same starts, crops).
``extract``: ``extract_flow`` of one video, uint8 and float32.
``kernels``: ``va_flow_quantize_u8`` alone, and the two uint8 gathers beside their float32 counterparts at the shapes of
the two paths above (250 items of ten-view evaluation; 24 snippets of scale-jitter training).
The stored calls launch a strict subset of the live calls' work: a ratio above 1 is a defect, not a result.
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


def _interleaved(runs, warmup, reps):
    """runs: name -> callable; -> name -> list of ms, the variants called in turn."""
    ms = dict((k, []) for k in runs)
    for i in range(warmup + reps):
        for k, fn in runs.items():
            dt, _ = _event_ms(fn)
            if i >= warmup:
                ms[k].append(dt)
    return ms


def _row(metric, ms, base, **extra):
    row = dict(metric=metric, **extra)
    for k, v in ms.items():
        row[k + "_ms"] = round(statistics.median(v), 4)
        row[k + "_ms_min"], row[k + "_ms_max"] = round(min(v), 4), round(max(v), 4)
    if base is not None:
        for k, v in ms.items():
            if k != base:
                row[k + "_over_" + base] = round(statistics.median(v) / statistics.median(ms[base]), 4)
    print(json.dumps(row), flush=True)


def _video(T, H, W, seed):
    import torch
    from video_analytics_amd import synth
    dev = torch.device("cuda", 0)
    _, gray, _ = synth.synth_clips(1, seed=seed, H=H, W=W, n_gray=T, device="cuda")
    rgb = torch.randint(0, 256, (T, 3, H, W), generator=torch.Generator(device=dev).manual_seed(seed), dtype=torch.uint8, device=dev)
    return rgb, gray[0].contiguous()


def video_mode(args, pipe):
    import torch
    from video_analytics_amd import augment
    H, W, T = args.height, args.width, args.frames
    views = augment.ten_crop_views(H, W)
    rgb, gray = _video(T, H, W, T)
    stores = dict(u8=pipe.extract_flow(gray), f32=pipe.extract_flow(gray, dtype=torch.float32))
    kw = dict(n_snippets=args.snippets, views=(views, views))
    runs = dict(live=lambda: pipe.run_video(rgb, gray, **kw), stored_u8=lambda: pipe.run_video(rgb, flow=stores["u8"], **kw),
                stored_f32=lambda: pipe.run_video(rgb, flow=stores["f32"], **kw))
    ms = _interleaved(runs, args.warmup, args.reps)
    same = all(torch.equal(runs["live"]()["scores"], runs[k]()["scores"]) for k in ("stored_u8", "stored_f32"))
    _row("run_video_ms", ms, "live", frames=T, height=H, width=W, snippets=args.snippets, views=10, reps=args.reps,
         same_scores=bool(same), store_mb=dict((k, round(v.numel() * v.element_size() / 1e6, 1)) for k, v in stores.items()))


def train_mode(args, pipe):
    import torch
    H, W, T, n, k = args.height, args.width, args.frames, args.videos, args.segments
    vids = [_video(T, H, W, 100 + v) for v in range(n)]
    rgbs = [r for r, _ in vids]
    labels = torch.arange(n) % 101
    u8 = [pipe.extract_flow(g) for _, g in vids]
    f32 = [pipe.extract_flow(g, dtype=torch.float32) for _, g in vids]
    step = [0]

    def call(**kw):  # the variants of one round draw the same starts and crops
        return pipe.train_videos(kw.pop("videos"), labels, k=k, lr=1e-4, rng=random.Random(step[0]), **kw)
    runs = dict(live=lambda: call(videos=vids), stored_u8=lambda: call(videos=rgbs, flows=u8),
                stored_f32=lambda: call(videos=rgbs, flows=f32))
    ms = dict((key, []) for key in runs)
    for i in range(args.warmup + args.reps):
        step[0] = i
        for key, fn in runs.items():
            dt, out = _event_ms(fn)
            if i >= args.warmup:
                ms[key].append(dt)
    _row("train_videos_ms", ms, "live", videos=n, segments=k, frames=T, height=H, width=W, reps=args.reps,
         finite=bool(torch.isfinite(out["stats_t"]).all().item()))


def extract_mode(args, pipe):
    import torch
    H, W, T = args.height, args.width, args.frames
    _, gray = _video(T, H, W, T)
    runs = dict(u8=lambda: pipe.extract_flow(gray), f32=lambda: pipe.extract_flow(gray, dtype=torch.float32))
    ms = _interleaved(runs, args.warmup, args.reps)
    _row("extract_flow_ms_per_video", ms, None, frames=T, height=H, width=W, flow_streams=pipe.flow_streams, reps=args.reps)


def kernels_mode(args):
    import torch
    from video_analytics_amd import augment, video
    from video_analytics_amd import flow as vflow
    from video_analytics_amd.parameters import VIDEO_INPUT_FLOW_COUNT as L
    H, W, T = args.height, args.width, args.frames
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    fl = torch.randn((T - 1, 2, H, W), generator=g, device=dev) * 12.0
    q = vflow.quantize_flow(fl)
    out_q = torch.empty_like(q)
    ms = _interleaved(dict(quantize=lambda: vflow.quantize_flow(fl, out=out_q)), 3, 20)
    _row("flow_quantize_ms", ms, None, pairs=T - 1, height=H, width=W, in_mb=round(fl.numel() * 4 / 1e6, 1),
         out_mb=round(q.numel() / 1e6, 1), reps=20)
    # the evaluation shape: 25 snippets x ten views of the video
    views = augment.ten_crop_views(H, W)
    starts = video.snippetStarts(T, L, args.snippets)
    out = torch.empty((len(starts), 10, 2 * L, 224, 224), device=dev)
    ms = _interleaved(dict(f32=lambda: vflow.crop_flow_to_stack_snippets(fl, starts, views, L, out=out),
                           u8=lambda: vflow.flowq_to_stack_snippets(q, starts, views, L, out=out)), 3, 20)
    _row("snippets_gather_ms", ms, "f32", snippets=len(starts), views=10, out_mb=round(out.numel() * 4 / 1e6, 1), reps=20,
         kernels=["k_flow_crop_stack<true, float>", "k_flow_crop_stack<true, unsigned char>"])
    # the training shape: n*k snippets, one scale-jitter crop each, windows drawn over the video's fields
    n = args.videos * args.segments
    rng = random.Random(n)
    first = [rng.randrange(T - 1 - L + 1) for _ in range(n)]
    _, table = augment.snippet_tables(augment.draw_scale_jitter_crops(n, H, W, rng), list(range(n)), first, L)
    out = torch.empty((n * 2 * L, 224, 224), device=dev)
    ms = _interleaved(dict(f32=lambda: vflow.resize_flow_to_stack(fl, table, out=out),
                           u8=lambda: vflow.resize_flowq_to_stack(q, table, out=out)), 3, 20)
    _row("resize_gather_ms", ms, "f32", snippets=n, out_mb=round(out.numel() * 4 / 1e6, 1), reps=20,
         kernels=["k_flow_resize_stack<float>", "k_flow_resize_stack<unsigned char>"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="+", choices=["video", "train", "extract", "kernels"], default=["kernels", "extract", "video", "train"])
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--snippets", type=int, default=25)
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_stored_flow.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    from video_analytics_amd import _ffi, pipeline
    if "kernels" in args.only:
        kernels_mode(args)
    if set(args.only) - {"kernels"}:
        params = _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)
        pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
        for mode, fn in (("extract", extract_mode), ("video", video_mode), ("train", train_mode)):
            if mode in args.only:
                fn(args, pipe)
        pipe.close()


if __name__ == "__main__":
    main()
