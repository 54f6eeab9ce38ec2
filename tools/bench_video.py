"""Videos/s of whole-video evaluation at native resolution, next to the same videos cut into
independent clips.

Per video length T and CNN dtype, interleaved in one process: ``TwoStreamPipeline.run_video`` (25 snippets, ten views,
TV-L1 once per planned frame pair) and the path a caller had before it: the 25 eleven-frame clips cut out on the device and
run through ``run_batch(views=)``, which computes TV-L1 for every window (250 pairs) and leaves consensus and fusion to the
caller.  Both use the full 5 x 5 x 300 schedule.  ``pipelined`` is ``submit_video`` for all repetitions, then one wait.
Prints one JSON line per (T, dtype).

    python tools/bench_video.py [--frames 37 150 300] [--dtypes f32 bf16] [--reps 3] [--warmup 1] [--height 240 --width 320]
                                [--snippets 25] [--skip-clips]

For the kernel times of the three video kernels run it under the profiler, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_video.py --frames 150 --dtypes f32 --skip-clips
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[37, 150, 300])
    ap.add_argument("--dtypes", nargs="+", choices=["f32", "bf16"], default=["f32", "bf16"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--snippets", type=int, default=25)
    ap.add_argument("--skip-clips", action="store_true", help="video mode only (for a kernel trace)")
    args = ap.parse_args()

    import torch
    from video_analytics_amd import _ffi, augment, pipeline, synth, video
    from video_analytics_amd.parameters import VIDEO_INPUT_FLOW_COUNT as L

    if not torch.cuda.is_available():
        sys.stderr.write("bench_video.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    H, W, n = args.height, args.width, args.snippets
    params = _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)
    views = augment.ten_crop_views(H, W)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for dtype in args.dtypes:
        pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params, cnn_dtype=dtype)
        for T in args.frames:
            _, gray, _ = synth.synth_clips(1, seed=T, H=H, W=W, n_gray=T, device="cuda")
            gray = gray[0].contiguous()
            g = torch.Generator(device=dev).manual_seed(T)
            rgb = torch.randint(0, 256, (T, 3, H, W), generator=g, dtype=torch.uint8, device=dev)
            plan = video.snippetPlan(T, L, n)
            starts = torch.tensor(plan.starts, device=dev)
            clip_gray = gray[starts[:, None] + torch.arange(L + 1, device=dev)[None]].contiguous()  # [n,L+1,H,W]
            clip_rgb = rgb[starts].contiguous()

            def run_video():
                return pipe.run_video(rgb, gray, n_snippets=n, views=(views, views))

            def run_clips():
                return pipe.run_batch(clip_rgb, clip_gray, views=(views, views))

            def run_pipelined():
                outs = [pipe.submit_video(rgb, gray, n_snippets=n, views=(views, views)) for _ in range(args.reps)]
                pipe.wait()
                return outs[-1]

            tv, tc = [], []
            for i in range(args.warmup + args.reps):  # interleaved: video, clips, video, clips, ...
                dt, out = timed(run_video)
                if i >= args.warmup:
                    tv.append(dt)
                if not args.skip_clips:
                    dt, _ = timed(run_clips)
                    if i >= args.warmup:
                        tc.append(dt)
            tp, _ = timed(run_pipelined)
            finite = bool(torch.isfinite(out["scores"]).all().item())
            row = dict(metric="videos_per_s", frames=T, height=H, width=W, snippets=n, views=10, cnn_dtype=dtype,
                       pairs_video=plan.pair_computations, pairs_clips=n * L, reps=args.reps,
                       video_s=round(statistics.median(tv), 4), video_s_min=round(min(tv), 4), video_s_max=round(max(tv), 4),
                       videos_per_s=round(1.0 / statistics.median(tv), 3),
                       pipelined_videos_per_s=round(args.reps / tp, 3), finite=finite,
                       tvl1="300 iters x 5 warps x 5 scales, exact math")
            if tc:
                row.update(clips_s=round(statistics.median(tc), 4), clips_s_min=round(min(tc), 4), clips_s_max=round(max(tc), 4),
                           clips_videos_per_s=round(1.0 / statistics.median(tc), 3),
                           speedup=round(statistics.median(tc) / statistics.median(tv), 3))
            print(json.dumps(row), flush=True)
        pipe.close()


if __name__ == "__main__":
    main()
