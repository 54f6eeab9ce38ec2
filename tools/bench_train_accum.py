"""Timings of gradient accumulation.  Prints one JSON line per measurement.

    python tools/bench_train_accum.py step   [--batch 32] [--reps 7]
    python tools/bench_train_accum.py videos [--videos 64] [--segments 3] [--micro 8] [--frames 150] [--reps 3]

``step``: per stream, the fused step (``train_step``) against ``train_accumulate`` + ``train_apply`` without and with
clipping at the same batch, interleaved in one process; HIP-event time per call, median over the repetitions.  The apply
launch is also timed on its own: its bytes (read G, V, W; write V, W: 20 bytes per parameter) over its time is the achieved
bandwidth, and the difference of the two apply forms is the cost of the clipping pass (4 bytes per parameter read once more).
``videos``: one ``train_videos`` step of n videos of T frames at 320x240, k segments, ``micro_videos=m``, full 5 x 5 x 300
TV-L1 schedule: videos/s, beside the fused step at m videos.
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


def step(args):
    import torch
    from video_analytics_amd import pipeline, vgg
    from video_analytics_amd.parameters import NACTION_CLASSES, VIDEO_DESCRIPTOR_DIM, VIDEO_INPUT_FLOW_COUNT as L
    dev = torch.device("cuda", 0)
    B = args.batch
    for c_in, name in ((3, "spatial"), (2 * L, "temporal")):
        w = pipeline.build_stream_weights(c_in, 1, dev)
        m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], NACTION_CLASSES, VIDEO_DESCRIPTOR_DIM)
        g = torch.Generator(device=dev).manual_seed(c_in)
        x = torch.randn((B, c_in, 224, 224), generator=g, device=dev)
        y = (torch.arange(B, device=dev) % NACTION_CLASSES).long()
        params = sum(m.grad_layout()[1])

        def two(clip, i):
            m.train_accumulate(x, y, first=True, dropout_seed=i)
            return m.train_apply(0.0, 0.9, clip)
        runs = dict(fused=lambda i: m.train_step(x, y, 0.0, 0.9, i),  # lr = 0 keeps the weights where they are
                    accumulate_apply=lambda i: two(None, i), accumulate_apply_clip=lambda i: two(1.0, i),
                    accumulate=lambda i: m.train_accumulate(x, y, first=True, dropout_seed=i),
                    accumulate_add=lambda i: m.train_accumulate(x, y, first=False, dropout_seed=i),
                    apply=lambda i: m.train_apply(0.0, 0.9), apply_clip=lambda i: m.train_apply(0.0, 0.9, 1.0))
        ms = dict((k, []) for k in runs)
        for i in range(args.warmup + args.reps):  # interleaved
            for k, fn in runs.items():
                dt, _ = _event_ms(lambda: fn(i))
                if i >= args.warmup:
                    ms[k].append(dt)
        row = dict(metric="train_accumulate_ms", stream=name, batch=B, reps=args.reps, parameters=params,
                   grad_mb=round(m.grad().numel() * 4 / 1e6, 1))
        for k, v in ms.items():
            row.update({k + "_ms": _med(v), k + "_ms_min": round(min(v), 4), k + "_ms_max": round(max(v), 4)})
        row["apply_gb_per_s"] = round(20.0 * params / (statistics.median(ms["apply"]) * 1e-3) / 1e9, 1)
        row["clip_pass_ms"] = round(statistics.median(ms["apply_clip"]) - statistics.median(ms["apply"]), 4)
        row["clip_pass_gb_per_s"] = round(4.0 * params / (max(row["clip_pass_ms"], 1e-6) * 1e-3) / 1e9, 1)
        row["extra_ms_over_fused"] = round(statistics.median(ms["accumulate_apply"]) - statistics.median(ms["fused"]), 4)
        print(json.dumps(row), flush=True)
        m.close()


def videos(args):
    import time
    import torch
    from video_analytics_amd import _ffi, pipeline, synth
    dev = torch.device("cuda", 0)
    n, k, T, H, W, micro = args.videos, args.segments, args.frames, args.height, args.width, args.micro
    params = _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    vids = []
    for v in range(n):
        _, gray, _ = synth.synth_clips(1, seed=100 + v, H=H, W=W, n_gray=T, device="cuda")
        g = torch.Generator(device=dev).manual_seed(v)
        vids.append((torch.randint(0, 256, (T, 3, H, W), generator=g, dtype=torch.uint8, device=dev), gray[0].contiguous()))
    labels = [v % 101 for v in range(n)]
    for what, sub, kw in (("fused", vids[:micro], {}), ("micro", vids, dict(micro_videos=micro)),
                          ("micro_clip", vids, dict(micro_videos=micro, clip_norm=1.0))):
        rng = random.Random(0)
        ts, pairs = [], 0
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe.train_videos(sub, labels[:len(sub)], k=k, lr=1e-5, dropout_seed=i, rng=rng, **kw)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(time.perf_counter() - t0)
            pairs = sum(p.pair_computations for p in out["plans"])
        print(json.dumps(dict(metric="train_videos_per_s", form=what, videos=len(sub), segments=k, micro_videos=kw.get("micro_videos"),
                              clip_norm=kw.get("clip_norm"), frames=T, height=H, width=W, tvl1_pairs=pairs, reps=args.reps,
                              step_s=_med(ts), step_s_min=round(min(ts), 4), step_s_max=round(max(ts), 4),
                              videos_per_s=round(len(sub) / statistics.median(ts), 3),
                              finite=bool(torch.isfinite(out["stats_s"]).all().item() and torch.isfinite(out["stats_t"]).all().item()),
                              tvl1="300 iters x 5 warps x 5 scales, exact math")), flush=True)
    pipe.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["step", "videos"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--micro", type=int, default=8)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.reps is None:
        args.reps = dict(step=7, videos=3)[args.mode]
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_train_accum.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    dict(step=step, videos=videos)[args.mode](args)


if __name__ == "__main__":
    main()
