"""Timings of the colour jitter.  Prints one JSON line per measurement.

    python tools/bench_color_jitter.py call  [--images 24 64] [--reps 50]
    python tools/bench_color_jitter.py train [--videos 8] [--segments 3] [--frames 150] [--reps 3]

``call``: ``va_color_jitter_u8`` (kernels ``k_color_jitter_sums`` and ``k_color_jitter_apply``) in place on n images of
224x224, every image with all four ops in a drawn order, beside the same rows without contrast (three ops, one launch) and
beside ``va_crop_images_u8`` (kernel ``k_crop_images_u8``) writing the same bytes, interleaved in one process; HIP-event time
per call, table upload included, median over the repetitions.  For the kernels' own times run it under the profiler, in a
run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_color_jitter.py call
``train``: one ``train_videos`` step of n videos x k snippets with ``color_jitter=(.4, .4, .4, .1)`` and without, interleaved
on one pipeline with the same draws of starts and crops, the step without jitter at two places of the cycle
(``without_again``: what two runs of the same thing differ by); wall time around a device synchronise.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

JITTER = (.4, .4, .4, .1)


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


def call_mode(args):
    import torch
    from video_analytics_amd import augment
    dev = torch.device("cuda", 0)
    for n in args.images:
        g = torch.Generator(device=dev).manual_seed(n)
        frames = torch.randint(0, 256, (n, 3, 240, 320), generator=g, dtype=torch.uint8, device=dev)
        x = torch.randint(0, 256, (n, 3, 224, 224), generator=g, dtype=torch.uint8, device=dev)
        four = augment.draw_color_jitter(n, *JITTER, rng=random.Random(n))
        three = augment.draw_color_jitter(n, JITTER[0], 0, JITTER[2], JITTER[3], rng=random.Random(n))
        crops = augment.draw_image_crops(n, 240, 320, rng=random.Random(n))
        bufs = dict((k, x.clone()) for k in ("four_ops", "without_contrast"))
        runs = dict(four_ops=lambda: augment.color_jitter(bufs["four_ops"], four, out=bufs["four_ops"]),
                    without_contrast=lambda: augment.color_jitter(bufs["without_contrast"], three, out=bufs["without_contrast"]),
                    crop=lambda: augment.crop_images(frames, crops))
        ms = dict((k, []) for k in runs)
        host = dict((k, []) for k in runs)  # the host's share: the time the call takes to return (checks, uploads, launches)
        for i in range(args.warmup + args.reps):  # interleaved
            for k, fn in runs.items():
                dt, _ = _event_ms(fn)
                if i >= args.warmup:
                    ms[k].append(dt)
            for k, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if i >= args.warmup:
                    host[k].append((time.perf_counter() - t0) * 1e3)
        mb = x.numel() * 2 / 1e6  # read once, written once (launch one reads the images a second time)
        row = dict(metric="color_jitter_ms_per_call", images=n, height=224, width=224, reps=args.reps, moved_mb=round(mb, 1),
                   kernels=["k_color_jitter_sums", "k_color_jitter_apply", "k_crop_images_u8"])
        for k, v in ms.items():
            row.update(_stats(k + "_ms", v))
            row[k + "_host_ms"] = round(statistics.median(host[k]), 4)
        row["four_ops_gb_per_s"] = round(mb / statistics.median(ms["four_ops"]), 1)
        print(json.dumps(row), flush=True)


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
    # one pipeline, the calls alternating (two pipelines with the same weights differed by 2 % in either direction, far more
    # than the jitter costs); the step without jitter is timed at two places of the cycle: what two runs of the same thing
    # differ by, to hold the difference against
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    runs = dict(without=dict(), with_jitter=dict(color_jitter=JITTER), without_again=dict())
    s = dict((key, []) for key in runs)
    for i in range(args.warmup + args.reps):  # every call of a cycle draws the same starts and crops (the jitter is drawn after them)
        for key, kw in runs.items():
            dt, out = _wall_s(lambda: pipe.train_videos(vids, labels, k=k, lr=1e-4, rng=random.Random(i), **kw))
            if i >= args.warmup:
                s[key].append(dt)
    row = dict(metric="train_videos_s", videos=n, segments=k, frames=T, height=H, width=W, jitter=list(JITTER), reps=args.reps,
               finite=bool(torch.isfinite(out["stats_s"]).all().item()), tvl1="300 iters x 5 warps x 5 scales, exact math")
    for key, v in s.items():
        row.update(_stats(key + "_s", v))
    row["ratio"] = round(statistics.median(s["with_jitter"]) / statistics.median(s["without"]), 4)
    row["ratio_same"] = round(statistics.median(s["without_again"]) / statistics.median(s["without"]), 4)
    print(json.dumps(row), flush=True)
    pipe.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["call", "train"])
    ap.add_argument("--images", type=int, nargs="+", default=[24, 64])
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--segments", type=int, default=3)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 50 if args.mode == "call" else 5
    if args.warmup is None:
        args.warmup = 5 if args.mode == "call" else 1

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_color_jitter.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    dict(call=call_mode, train=train_mode)[args.mode](args)


if __name__ == "__main__":
    main()
