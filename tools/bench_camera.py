"""The cost of warped optical flow on one MI355X.  Prints one JSON line per measurement.

    python tools/bench_camera.py --mode kernels [--fields 320 1490] [--reps 5] [--height 240 --width 320]
        va_flow_homography and va_flow_compensate (in place) on device-resident fields: the flow of a homography per field,
        an outlier box of 15 % and 0.05 px noise.  Times are HIP events around each call; for the kernels' own times run it
        under the profiler, in a run of its own:
            rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_camera.py --mode kernels
    python tools/bench_camera.py --mode pipeline [--batch 32] [--reps 5] [--warmup 1] [--cnn-dtype f32|bf16]
        clips/s of TwoStreamPipeline.run_batch on 320x240 clips with one random crop per image and the full 5 x 5 x 300
        schedule, camera="homography" against camera="none", interleaved in one process, median of --reps.
    python tools/bench_camera.py --mode headline --other-tree PATH [--rounds 3] [--steps 10 --warmup 3]
        bench.py of this tree and of another built checkout (the parent commit), alternating, each run a fresh process.
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_fields(N, H, W, dev):
    """[N,2,H,W] float32 on the device: per field the flow of a homography near the identity, a box of 15 % of the frame
    that moves by another (+6, -4) px, and 0.05 px noise."""
    import torch
    g = torch.Generator(device=dev).manual_seed(N)
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                          indexing="ij")
    flow = torch.empty((N, 2, H, W), dtype=torch.float32, device=dev)
    r = torch.rand((N, 8), generator=g, device=dev, dtype=torch.float64) * 2.0 - 1.0
    bh, bw = int(H * 0.15 ** 0.5), int(W * 0.15 ** 0.5)
    for n in range(N):
        a = r[n] * torch.tensor([0.01, 0.01, 3.0, 0.01, 0.01, 3.0, 2e-5, 2e-5], device=dev, dtype=torch.float64)
        D = a[6] * x + a[7] * y + 1.0
        flow[n, 0] = (((1.0 + a[0]) * x + a[1] * y + a[2]) / D - x).float()
        flow[n, 1] = ((a[3] * x + (1.0 + a[4]) * y + a[5]) / D - y).float()
        top, left = (n * 37) % (H - bh + 1), (n * 53) % (W - bw + 1)
        flow[n, 0, top:top + bh, left:left + bw] += 6.0
        flow[n, 1, top:top + bh, left:left + bw] -= 4.0
    flow += torch.randn(flow.shape, generator=g, device=dev) * 0.05
    return flow


def bench_kernels(args):
    import torch
    from video_analytics_amd import flow as vflow
    dev = torch.device("cuda", 0)
    H, W = args.height, args.width
    for N in args.fields:
        flow = synthetic_fields(N, H, W, dev)
        work = flow.clone()
        fit_ms, comp_ms = [], []
        for i in range(args.warmup + args.reps):
            work.copy_(flow)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            Hm, stats = vflow.fit_homography(work)
            e[1].record()
            vflow.compensate_camera(work, Hm, out=work)
            e[2].record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                fit_ms.append(e[0].elapsed_time(e[1]))
                comp_ms.append(e[1].elapsed_time(e[2]))
        px = N * H * W
        print(json.dumps(dict(metric="camera_kernels_ms", fields=N, height=H, width=W, reps=args.reps,
                              fit_ms=round(statistics.median(fit_ms), 4), fit_ms_min=round(min(fit_ms), 4),
                              fit_ms_max=round(max(fit_ms), 4), compensate_ms=round(statistics.median(comp_ms), 4),
                              compensate_ms_min=round(min(comp_ms), 4), compensate_ms_max=round(max(comp_ms), 4),
                              compensate_gb_per_s=round(16.0 * px / (1e6 * statistics.median(comp_ms)), 1),
                              degenerate=int(stats[:, 1].sum().item()), mean_share=round(float(stats[:, 0].mean().item()), 4))),
              flush=True)


def bench_pipeline(args):
    import torch
    from video_analytics_amd import _ffi, augment, pipeline, synth
    from video_analytics_amd.parameters import VIDEO_INPUT_FLOW_COUNT as L
    dev = torch.device("cuda", 0)
    B, H, W = args.batch, args.height, args.width
    params = _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)
    cams = ("none", "homography")
    pipes = {c: pipeline.TwoStreamPipeline(device=0, tvl1_params=params, cnn_dtype=args.cnn_dtype, camera=c) for c in cams}
    rgb, gray, _ = synth.synth_clips(B, seed=0, H=H, W=W)
    rgb, gray = rgb.to(dev), gray.to(dev)
    random.seed(0)
    times = {c: [] for c in cams}
    for i in range(args.warmup + args.reps):  # interleaved: none, homography, none, homography, ...
        crops = augment.draw_clip_crops(B, L, (H, W), (H, W))
        for c in cams:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipes[c].run_batch(rgb, gray, crops=crops)
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[c].append(time.perf_counter() - t0)
    finite = bool(torch.isfinite(out["logits_t"]).all().item())
    for p in pipes.values():
        p.close()
    row = dict(metric="camera_clips_per_s", batch=B, height=H, width=W, reps=args.reps, cnn_dtype=args.cnn_dtype, finite=finite,
               tvl1="300 iters x 5 warps x 5 scales, exact math")
    for c in cams:
        row[c + "_clips_per_s"] = round(B / statistics.median(times[c]), 2)
        row[c + "_step_ms"] = [round(1e3 * t, 2) for t in times[c]]
    row["ratio"] = round(statistics.median(times["none"]) / statistics.median(times["homography"]), 4)
    print(json.dumps(row), flush=True)


def bench_headline(args):
    trees = (("this", ROOT), ("other", os.path.abspath(args.other_tree)))
    values = {name: [] for name, _ in trees}
    for _ in range(args.rounds):
        for name, tree in trees:
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup)],
                               cwd=tree, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(r.returncode)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
            values[name].append(json.loads(line)["value"])
    print(json.dumps(dict(metric="headline_this_against_other", steps=args.steps, warmup=args.warmup, rounds=args.rounds,
                          this=values["this"], other=values["other"], this_median=statistics.median(values["this"]),
                          other_median=statistics.median(values["other"]))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernels", "pipeline", "headline"], required=True)
    ap.add_argument("--fields", type=int, nargs="+", default=[320, 1490])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--cnn-dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--other-tree", help="headline mode: a built checkout of the commit to compare with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    if args.mode == "headline":
        if not args.other_tree:
            ap.error("--mode headline needs --other-tree")
        if args.warmup == 1:
            args.warmup = 3
        return bench_headline(args)
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_camera.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    (bench_kernels if args.mode == "kernels" else bench_pipeline)(args)


if __name__ == "__main__":
    main()
