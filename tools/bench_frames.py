"""Timings of the frame preparation.  Prints one JSON line per measurement.

    python tools/bench_frames.py call  [--frames 150] [--height 240 --width 320] [--short-side 256] [--reps 20] [--threads 16]
    python tools/bench_frames.py video [--frames 150] [--height 240 --width 320] [--dtypes f32] [--reps 5]

``call``: ``frames.prepare_frames`` on T decoded frames in two configurations, rescaled to the short side (kernels
``k_frames_hpass`` and ``k_frames_vpass``) and gray only (``k_frames_gray``), interleaved in one process; HIP-event time per
call, median over the repetitions, beside the host's share (the time the call takes to return: checks, the cached tables,
the allocations and the launches) and beside the path a user had before it: PIL ``resize`` + ``convert('L')`` of every frame
on a pool of host threads plus the upload of both results, wall time around a device synchronise.  ``moved_mb`` is what the
kernels read and write, computed from the shapes.  For the kernels' own times run it under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_frames.py call
``video``: ``run_video(rgb)`` against ``run_video(rgb, gray)`` on tools/bench_video.py's configuration (25 snippets, ten
views, the full 5 x 5 x 300 schedule), interleaved on one pipeline, the call with a given gray at two places of the cycle
(``given_again``: what two runs of the same thing differ by); wall time around a device synchronise.
"""
import argparse
import json
import os
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


def call_mode(args):
    import numpy as np
    import torch
    from video_analytics_amd import frames
    try:
        from PIL import Image
    except ImportError:
        Image = None
    from concurrent.futures import ThreadPoolExecutor
    dev = torch.device("cuda", 0)
    T, H, W = args.frames, args.height, args.width
    oh, ow = frames.short_side_size(H, W, args.short_side)
    host = np.random.RandomState(T).randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)  # HWC, as a decoder hands it over
    x = torch.from_numpy(np.ascontiguousarray(host.transpose(0, 3, 1, 2))).to(dev)
    runs = dict(rescale=lambda: frames.prepare_frames(x, args.short_side), gray_only=lambda: frames.prepare_frames(x))
    ms = dict((k, []) for k in runs)
    ret = dict((k, []) for k in runs)
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
                ret[k].append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    frames.resample_table(W, ow)
    frames.resample_table(H, oh)
    tables_ms = (time.perf_counter() - t0) * 1e3  # once per (size, device): the cache holds them afterwards
    moved = dict(rescale=T * (3 * H * W + 2 * 3 * H * ow + 4 * oh * ow) / 1e6,  # frames in, intermediate out and in, rgb + gray out
                 gray_only=T * 4 * H * W / 1e6)
    row = dict(metric="prepare_frames_ms_per_call", frames=T, height=H, width=W, out_height=oh, out_width=ow, reps=args.reps,
               kernels=["k_frames_hpass", "k_frames_vpass", "k_frames_gray"], tables_once_ms=round(tables_ms, 3))
    for k in runs:
        row.update(_stats(k + "_ms", ms[k]))
        row[k + "_host_return_ms"] = round(statistics.median(ret[k]), 4)
        row[k + "_moved_mb"] = round(moved[k], 1)
        row[k + "_gb_per_s"] = round(moved[k] / statistics.median(ms[k]), 1)
    if Image is not None:  # the path users had: PIL on host threads, then two uploads
        def one(f):
            im = Image.fromarray(f).resize((ow, oh), Image.BILINEAR)
            return np.asarray(im), np.asarray(im.convert("L"))

        def one_gray(f):
            return np.asarray(Image.fromarray(f).convert("L"))

        def host_rescale(pool):
            res = list(pool.map(one, host))
            rgb = torch.from_numpy(np.stack([r for r, _ in res])).to(dev)
            gray = torch.from_numpy(np.stack([g for _, g in res])).to(dev)
            return rgb, gray

        def host_gray(pool):
            return torch.from_numpy(np.stack(list(pool.map(one_gray, host)))).to(dev)
        hs = dict(rescale=[], gray_only=[])
        with ThreadPoolExecutor(args.threads) as pool:
            for i in range(1 + max(args.reps // 4, 3)):
                for k, fn in (("rescale", host_rescale), ("gray_only", host_gray)):
                    dt, _ = _wall_s(lambda: fn(pool))
                    if i >= 1:
                        hs[k].append(dt * 1e3)
        for k, v in hs.items():
            row.update(_stats("pil_%d_threads_%s_ms" % (args.threads, k), v, 2))
    print(json.dumps(row), flush=True)


def video_mode(args):
    import torch
    from video_analytics_amd import _ffi, augment, pipeline, synth, utils
    dev = torch.device("cuda", 0)
    T, H, W = args.frames, args.height, args.width
    params = _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)
    views = augment.ten_crop_views(H, W)
    _, tex, _ = synth.synth_clips(1, seed=T, H=H, W=W, n_gray=T, device="cuda")
    g = tex[0]
    rgb = torch.stack([g, torch.roll(g, 5, dims=2), 255 - torch.roll(g, 3, dims=1)], dim=1).contiguous()  # a moving texture
    gray = torch.from_numpy(utils.grayLevel(rgb.permute(0, 2, 3, 1).cpu().numpy())).to(dev)
    for dtype in args.dtypes:
        pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params, cnn_dtype=dtype)
        runs = dict(given=lambda: pipe.run_video(rgb, gray, views=(views, views)),
                    derived=lambda: pipe.run_video(rgb, views=(views, views)),
                    given_again=lambda: pipe.run_video(rgb, gray, views=(views, views)))
        s = dict((k, []) for k in runs)
        outs = {}
        for i in range(args.warmup + args.reps):  # interleaved
            for k, fn in runs.items():
                dt, outs[k] = _wall_s(fn)
                if i >= args.warmup:
                    s[k].append(dt)
        same = all(torch.equal(outs["given"][key], outs["derived"][key]) for key in ("scores", "logits_s_items", "logits_t_items"))
        row = dict(metric="run_video_s", frames=T, height=H, width=W, snippets=25, views=10, cnn_dtype=dtype, reps=args.reps,
                   pairs=outs["derived"]["plan"].pair_computations, same_bits=bool(same),
                   tvl1="300 iters x 5 warps x 5 scales, exact math")
        for k, v in s.items():
            row.update(_stats(k + "_s", v))
        row["ratio"] = round(statistics.median(s["derived"]) / statistics.median(s["given"]), 4)
        row["ratio_same"] = round(statistics.median(s["given_again"]) / statistics.median(s["given"]), 4)
        print(json.dumps(row), flush=True)
        pipe.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["call", "video"])
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--short-side", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dtypes", nargs="+", choices=["f32", "bf16"], default=["f32"])
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 20 if args.mode == "call" else 5
    if args.warmup is None:
        args.warmup = 3 if args.mode == "call" else 1

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_frames.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    dict(call=call_mode, video=video_mode)[args.mode](args)


if __name__ == "__main__":
    main()
