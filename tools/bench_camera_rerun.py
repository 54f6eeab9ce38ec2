"""The cost of the two-pass warped optical flow on one MI355X, beside the subtract form (S22) and no camera
step at all.  The three variants are interleaved in one process; times are HIP events, median of --reps.  Prints one JSON line
per measurement.

    python tools/bench_camera_rerun.py --mode step [--batch 32] [--reps 5] [--warmup 1] [--cnn-dtype f32|bf16]
        TwoStreamPipeline.run_batch on 320x240 clips with one random crop per image and the full 5 x 5 x 300 schedule.
    python tools/bench_camera_rerun.py --mode extract [--frames 150] [--reps 5]
        TwoStreamPipeline.extract_flow of one video (uint8 store), the same schedule.
    python tools/bench_camera_rerun.py --mode warp [--fields 320 1490] [--reps 5]
        va_frames_warp_pairs alone on uint8 and float32 frames, with the bytes it moves (per pair: two frame planes and the
        homography read, two float planes written) and the rate they give.  For the kernel's own time run it under the
        profiler, in a run of its own:
            rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_camera_rerun.py --mode warp
    python tools/bench_camera_rerun.py --mode fields [--height 240 --width 320]
        How far the two forms' fields are apart on a synthetic scene: a textured background under a planted camera
        homography and a box of 15 % of the frame with a texture of its own that moves by another (+6, -4) px.  Median and
        99th percentile of the distance between the forms, and of each form's distance to the planted residual motion in its
        own sense (subtract: the box's displacement minus the camera's; rerun: where the box's pixel lands once frame 1 is
        warped back, H^-1 (x + d) - x; they differ by the camera's linear part applied to d, about 0.15 px here), per region
        (background, box).  Reported, not asserted.

The headline comparison against the parent commit is tools/bench_camera.py --mode headline.
"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = (("none", dict(camera="none")), ("subtract", dict(camera="homography", camera_form="subtract")),
            ("rerun", dict(camera="homography", camera_form="rerun")))
H_PLANTED = [[1.01 * 0.9998000066665778, -0.01999866669333308, 3.0],   # 1 % zoom, 0.02 rad, (3, -2) px, a little perspective
             [0.01999866669333308, 1.01 * 0.9998000066665778, -2.0],
             [2e-5, -1e-5, 1.0]]


def full_schedule():
    from video_analytics_amd import _ffi
    return _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)


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


def report(metric, times, **row):
    for name, ms in times.items():
        row[name + "_ms"] = round(statistics.median(ms), 3)
        row[name + "_ms_all"] = [round(t, 3) for t in ms]
    for name in ("subtract", "rerun"):
        if name in times and "none" in times:
            row[name + "_over_none"] = round(statistics.median(times[name]) / statistics.median(times["none"]), 4)
    print(json.dumps(dict(metric=metric, **row)), flush=True)


def bench_step(args):
    import torch
    from video_analytics_amd import augment, pipeline, synth
    from video_analytics_amd.parameters import VIDEO_INPUT_FLOW_COUNT as L
    dev = torch.device("cuda", 0)
    B, H, W = args.batch, args.height, args.width
    pipes = {name: pipeline.TwoStreamPipeline(device=0, tvl1_params=full_schedule(), cnn_dtype=args.cnn_dtype, **kw)
             for name, kw in VARIANTS}
    rgb, gray, _ = synth.synth_clips(B, seed=0, H=H, W=W)
    rgb, gray = rgb.to(dev), gray.to(dev)
    random.seed(0)
    times = {name: [] for name, _ in VARIANTS}
    for i in range(args.warmup + args.reps):  # interleaved: none, subtract, rerun, none, ...
        crops = augment.draw_clip_crops(B, L, (H, W), (H, W))
        for name, _ in VARIANTS:
            out, ms = timed(lambda: pipes[name].run_batch(rgb, gray, crops=crops))
            if i >= args.warmup:
                times[name].append(ms)
    finite = bool(torch.isfinite(out["logits_t"]).all().item())
    for p in pipes.values():
        p.close()
    report("camera_rerun_step_ms", times, batch=B, height=H, width=W, reps=args.reps, cnn_dtype=args.cnn_dtype, finite=finite,
           tvl1="300 iters x 5 warps x 5 scales, exact math")


def bench_extract(args):
    import torch
    from video_analytics_amd import pipeline, synth
    dev = torch.device("cuda", 0)
    T, H, W = args.frames, args.height, args.width
    pipes = {name: pipeline.TwoStreamPipeline(device=0, tvl1_params=full_schedule(), **kw) for name, kw in VARIANTS}
    _, gray, _ = synth.synth_clips(1, seed=1, H=H, W=W, n_gray=T)
    gray = gray[0].to(dev)
    times = {name: [] for name, _ in VARIANTS}
    for i in range(args.warmup + args.reps):
        for name, _ in VARIANTS:
            store, ms = timed(lambda: pipes[name].extract_flow(gray))
            if i >= args.warmup:
                times[name].append(ms)
    for p in pipes.values():
        p.close()
    report("camera_rerun_extract_flow_ms", times, frames=T, height=H, width=W, reps=args.reps, store=str(store.dtype),
           tvl1="300 iters x 5 warps x 5 scales, exact math")


def bench_warp(args):
    import torch
    from video_analytics_amd import flow as vflow
    dev = torch.device("cuda", 0)
    H, W = args.height, args.width
    for N in args.fields:
        g = torch.Generator(device=dev).manual_seed(N)
        r = torch.rand((N, 8), generator=g, device=dev, dtype=torch.float64) * 2.0 - 1.0
        Hm = torch.eye(3, dtype=torch.float64, device=dev).repeat(N, 1, 1)
        scale = torch.tensor([0.01, 0.01, 3.0, 0.01, 0.01, 3.0, 2e-5, 2e-5], device=dev, dtype=torch.float64)
        Hm.view(N, 9)[:, :8] += r * scale
        for dtype in (torch.uint8, torch.float32):
            frames = (torch.rand((N, 2, H, W), generator=g, device=dev) * 255.0).to(dtype)
            out = torch.empty((N, 2, H, W), dtype=torch.float32, device=dev)
            ms = []
            for i in range(args.warmup + args.reps):
                _, t = timed(lambda: vflow.warp_pairs(frames, Hm, out=out))
                if i >= args.warmup:
                    ms.append(t)
            moved = N * (2 * H * W * frames.element_size() + 72 + 2 * H * W * 4)
            med = statistics.median(ms)
            print(json.dumps(dict(metric="camera_rerun_warp_ms", pairs=N, height=H, width=W, frames=str(dtype), reps=args.reps,
                                  warp_ms=round(med, 4), warp_ms_min=round(min(ms), 4), warp_ms_max=round(max(ms), 4),
                                  bytes_moved=moved, tb_per_s=round(moved / (1e9 * med), 3))), flush=True)


def synthetic_scene(H, W, dev):
    """-> (gray f32 [1,2,H,W], box mask [H,W] in frame 0, planted residuals [2,H,W] of the subtract and of the rerun form):
    frame 1 holds the background where H_PLANTED^-1 sees it and the box, a texture of its own, moved by (+6, -4) px.  The
    residual motion is zero outside the box; inside it is the box's motion minus the camera's displacement (subtract), or
    H_PLANTED^-1 (x + d) - x, the box's pixel seen in the warped frame (rerun)."""
    import torch
    from video_analytics_amd import synth
    m = 24

    def texture(seed):
        n = synth._uniform_pm(seed, 7, (1, 1, H + 2 * m, W + 2 * m), 1.0).to(dev)
        t = synth._blur(n, 2.0)
        return (t - t.min()) * (255.0 / (t.max() - t.min()))

    def sample(tex, x, y):  # bicubic, pixel coordinates of the unpadded frame
        gx = (x + m + 0.5) * (2.0 / (W + 2 * m)) - 1.0
        gy = (y + m + 0.5) * (2.0 / (H + 2 * m)) - 1.0
        grid = torch.stack([gx, gy], dim=-1)[None].float()
        return torch.nn.functional.grid_sample(tex, grid, mode="bicubic", padding_mode="border", align_corners=False)[0, 0]

    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                          indexing="ij")
    Hm = torch.tensor(H_PLANTED, dtype=torch.float64, device=dev)
    inv = torch.linalg.inv(Hm)
    D = inv[2, 0] * x + inv[2, 1] * y + inv[2, 2]
    bx, by = (inv[0, 0] * x + inv[0, 1] * y + inv[0, 2]) / D, (inv[1, 0] * x + inv[1, 1] * y + inv[1, 2]) / D
    bh, bw = int(H * 0.15 ** 0.5), int(W * 0.15 ** 0.5)
    top, left = (H - bh) // 2, (W - bw) // 2
    dx, dy = 6.0, -4.0
    in_box = lambda u, v: (u >= left) & (u < left + bw) & (v >= top) & (v < top + bh)
    bg, fg = texture(11), texture(12)
    f0 = torch.where(in_box(x, y), sample(fg, x, y), sample(bg, x, y))
    f1 = torch.where(in_box(x - dx, y - dy), sample(fg, x - dx, y - dy), sample(bg, bx, by))
    Dn = Hm[2, 0] * x + Hm[2, 1] * y + Hm[2, 2]
    cx = (Hm[0, 0] * x + Hm[0, 1] * y + Hm[0, 2]) / Dn - x
    cy = (Hm[1, 0] * x + Hm[1, 1] * y + Hm[1, 2]) / Dn - y
    mask = in_box(x, y)
    zero = torch.zeros_like(cx)
    res_sub = torch.stack([torch.where(mask, dx - cx, zero), torch.where(mask, dy - cy, zero)])
    Db = inv[2, 0] * (x + dx) + inv[2, 1] * (y + dy) + inv[2, 2]
    rx = (inv[0, 0] * (x + dx) + inv[0, 1] * (y + dy) + inv[0, 2]) / Db - x
    ry = (inv[1, 0] * (x + dx) + inv[1, 1] * (y + dy) + inv[1, 2]) / Db - y
    res_rerun = torch.stack([torch.where(mask, rx, zero), torch.where(mask, ry, zero)])
    return torch.stack([f0, f1])[None].clamp(0.0, 255.0).float().contiguous(), mask, res_sub.float(), res_rerun.float()


def bench_fields(args):
    import torch
    from video_analytics_amd import flow as vflow
    dev = torch.device("cuda", 0)
    H, W = args.height, args.width
    gray, mask, res_sub, res_rerun = synthetic_scene(H, W, dev)
    params = full_schedule()
    plain = vflow.tvl1_flow(gray, params)
    sub, Hs, share = vflow.apply_camera(plain, "homography")
    rer, _, _ = vflow.rerun_camera(gray, plain, params)
    torch.cuda.synchronize()

    def stats(d, region):
        v = torch.hypot(d[0], d[1])[region].double()
        return dict(median=round(float(v.median()), 4), p99=round(float(torch.quantile(v, 0.99)), 4))
    edge = 8  # the box's rim, where either form sees an occlusion
    inner = torch.zeros_like(mask)
    ys, xs = torch.nonzero(mask, as_tuple=True)
    inner[int(ys.min()) + edge:int(ys.max()) + 1 - edge, int(xs.min()) + edge:int(xs.max()) + 1 - edge] = True
    grown = torch.nn.functional.max_pool2d(mask[None, None].float(), 2 * edge + 1, 1, edge)[0, 0] > 0
    regions = dict(background=~grown, box=inner)
    row = dict(metric="camera_rerun_fields_px", height=H, width=W, tvl1="300 iters x 5 warps x 5 scales, exact math",
               trusted_share=round(float(share[0]), 4),
               fitted_minus_planted=round(float((Hs[0] - torch.tensor(H_PLANTED, dtype=torch.float64, device=dev)).abs().max()), 6))
    for name, region in regions.items():
        row[name] = dict(pixels=int(region.sum()), between_forms=stats(rer[0] - sub[0], region),
                         subtract_to_planted=stats(sub[0] - res_sub, region), rerun_to_planted=stats(rer[0] - res_rerun, region),
                         rerun_above_1px=round(float((torch.hypot(*(rer[0] - res_rerun))[region] > 1.0).double().mean()), 4),
                         subtract_above_1px=round(float((torch.hypot(*(sub[0] - res_sub))[region] > 1.0).double().mean()), 4))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "extract", "warp", "fields"], required=True)
    ap.add_argument("--fields", type=int, nargs="+", default=[320, 1490])
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--cnn-dtype", choices=["f32", "bf16"], default="f32")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_camera_rerun.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    dict(step=bench_step, extract=bench_extract, warp=bench_warp, fields=bench_fields)[args.mode](args)


if __name__ == "__main__":
    main()
