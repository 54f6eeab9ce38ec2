"""Timings of the JPEG decoder.  Prints one JSON line per measurement.

    python tools/bench_jpeg.py call  [--frames 150] [--flow-images 298] [--height 240 --width 320] [--reps 20] [--threads 16]
    python tools/bench_jpeg.py video [--frames 150] [--height 240 --width 320] [--reps 5]

``call``: ``jpeg.decode_jpegs`` taken apart on four workloads -- T textured colour frames at quality 95, 4:2:0, without
restart markers and with one per MCU row, and N gray flow images, the same two ways: the host's parse and pack (wall clock),
the upload (HIP events around the pinned copy), ``va_jpeg_decode`` (events; median over the repetitions; its memsets and
three launches), and the second and third launch alone through their testing entry points (``va_jpeg_idct``,
``va_jpeg_upsample``): what remains of the call is the entropy launch and the two memsets (``entropy_and_memsets_ms``, a
difference, not a measurement of its own; the IDCT alone runs on zero coefficients).
Beside them the path a user had: PIL decoding every file on 1 and on ``--threads`` host threads, the upload of the stacked
``NHWC`` array and its ``NCHW`` copy on the device; wall clock around a device synchronise.  ``bytes_per_image`` is the
mean file size.
``video``: ``run_video(path)`` against PIL-decoding the same AVI, uploading the frames and ``run_video(rgb)`` (the decode
counted), on tools/bench_video.py's configuration (25 snippets, ten views, the full 5 x 5 x 300 schedule), interleaved on one
pipeline; wall time around a device synchronise, median over the repetitions.
"""
import argparse
import io
import json
import os
import statistics
import struct
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


def _wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(prefix, xs, digits=4):
    return {prefix: round(statistics.median(xs), digits), prefix + "_min": round(min(xs), digits),
            prefix + "_max": round(max(xs), digits)}


def textured_frames(T, H, W):
    """u8 [T,H,W,3]: a coarse random texture that drifts two pixels a frame under fine noise -- not flat, so the files carry
    a video's worth of coefficients."""
    import numpy as np
    rs = np.random.RandomState(T)
    coarse = rs.randint(0, 256, size=(H // 8 + 2, W // 8 + 2, 3)).astype(np.float32)
    big = np.kron(coarse, np.ones((8, 8, 1), dtype=np.float32))
    k = np.ones(5, dtype=np.float32) / 5
    for axis in (0, 1):  # soften the block edges
        big = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), axis, big)
    out = np.empty((T, H, W, 3), dtype=np.uint8)
    for t in range(T):
        f = np.roll(big, (t % 8, 2 * t % 16), axis=(0, 1))[:H, :W] + rs.standard_normal((H, W, 3)) * 6
        out[t] = np.clip(f, 0, 255).astype(np.uint8)
    return out


def flow_planes(N, H, W):
    """u8 [N,H,W]: smooth flow-like fields around 128 under fine noise."""
    import numpy as np
    rs = np.random.RandomState(N)
    yy, xx = np.mgrid[:H, :W]
    out = np.empty((N, H, W), dtype=np.uint8)
    for i in range(N):
        f = 128 + 40 * np.sin(xx / 23.0 + i / 5.0) * np.cos(yy / 17.0 - i / 7.0) + rs.standard_normal((H, W)) * 2
        out[i] = np.clip(f, 0, 255).astype(np.uint8)
    return out


def encode(a, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=95, **kw)
    return buf.getvalue()


def write_avi(path, jpegs):
    chunks = b"".join(b"00dc" + struct.pack("<I", len(d)) + d + (b"\0" if len(d) & 1 else b"") for d in jpegs)
    movi = b"LIST" + struct.pack("<I", 4 + len(chunks)) + b"movi" + chunks
    strh = b"strh" + struct.pack("<I", 56) + b"vids" + b"MJPG" + b"\0" * 48
    strl = b"LIST" + struct.pack("<I", 4 + len(strh)) + b"strl" + strh
    hdrl = b"LIST" + struct.pack("<I", 4 + len(strl)) + b"hdrl" + strl
    body = b"AVI " + hdrl + movi
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def call_mode(args):
    import numpy as np
    import torch
    from PIL import Image
    from concurrent.futures import ThreadPoolExecutor
    from video_analytics_amd import jpeg
    dev = torch.device("cuda", 0)
    H, W = args.height, args.width
    rgb, gray = textured_frames(args.frames, H, W), flow_planes(args.flow_images, H, W)
    loads = {
        "frames_420": [encode(f, subsampling=2) for f in rgb],
        "frames_420_restart_per_mcu_row": [encode(f, subsampling=2, restart_marker_blocks=-(-W // 16)) for f in rgb],
        "flow_gray": [encode(f) for f in gray],
        "flow_gray_restart_per_block_row": [encode(f, restart_marker_blocks=-(-W // 8)) for f in gray],
    }
    for name, datas in loads.items():
        n = len(datas)
        hdrs, (w, h, nc, hs, vs) = jpeg.parse_batch(datas, "bench")
        shape = (n, w, h, nc, hs, vs)
        geo = jpeg.layout(w, h, nc, hs, vs)
        parse, pack, up, dec, idct, color, whole = [], [], [], [], [], [], []
        out = torch.empty((n, 3, h, w) if nc == 3 else (n, h, w), dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        coef = torch.zeros((n, geo["blocks"], 64), dtype=torch.int16, device=dev)
        quant = torch.ones((nc, 64), dtype=torch.int16, device=dev)
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            hdrs = [jpeg.parse_jpeg(d) for d in datas]
            t1 = time.perf_counter()
            packed, nseg, nsets = jpeg.pack_jpegs(hdrs)
            t2 = time.perf_counter()
            u, d = _event_ms(lambda: jpeg.upload(packed, dev))
            k, _ = _event_ms(lambda: jpeg.launch(d, shape, nseg, nsets, out, status))
            b, planes = _event_ms(lambda: jpeg.idct_planes(coef, quant, w, h, nc, hs, vs))
            c = _event_ms(lambda: jpeg.upsample_planes(planes, w, h, hs, vs))[0] if nc == 3 else 0.0
            t, _ = _wall_ms(lambda: jpeg.decode_jpegs(datas, dev))
            if i >= args.warmup:
                parse.append((t1 - t0) * 1e3), pack.append((t2 - t1) * 1e3), up.append(u), dec.append(k), idct.append(b)
                color.append(c), whole.append(t)
        assert not status.any()
        row = dict(metric="decode_jpegs_ms_per_call", workload=name, images=n, height=h, width=w, components=nc, segments=nseg,
                   table_sets=nsets, bytes_per_image=round(sum(map(len, datas)) / n), upload_bytes=len(packed), reps=args.reps,
                   kernels=["k_jpeg_entropy", "k_jpeg_idct", "k_jpeg_color"])
        for key, xs in (("host_parse_ms", parse), ("host_pack_ms", pack), ("upload_ms", up), ("va_jpeg_decode_ms", dec),
                        ("idct_ms", idct), ("color_ms", color), ("decode_jpegs_wall_ms", whole)):
            row.update(_stats(key, xs, 3))
        row["entropy_and_memsets_ms"] = round(row["va_jpeg_decode_ms"] - row["idct_ms"] - row["color_ms"], 3)

        def pil_one(d):
            return np.asarray(Image.open(io.BytesIO(d)).convert("RGB" if nc == 3 else "L"))

        def pil_path(pool):
            a = np.stack(list(pool.map(pil_one, datas)) if pool is not None else [pil_one(d) for d in datas])
            t = torch.from_numpy(a).to(dev)
            return t.permute(0, 3, 1, 2).contiguous() if nc == 3 else t
        with ThreadPoolExecutor(args.threads) as pool:
            for label, p in (("pil_1_thread", None), ("pil_%d_threads" % args.threads, pool)):
                xs = [_wall_ms(lambda: pil_path(p))[0] for _ in range(1 + max(args.reps // 4, 3))][1:]
                row.update(_stats(label + "_decode_upload_nchw_ms", xs, 2))
            xs = []
            for _ in range(4):
                t0 = time.perf_counter()
                list(pool.map(pil_one, datas))
                xs.append((time.perf_counter() - t0) * 1e3)
            row.update(_stats("pil_%d_threads_decode_only_ms" % args.threads, xs[1:], 2))
        got = jpeg.decode_jpegs(datas[:4], dev)[0].cpu().numpy()
        want = np.stack([pil_one(d) for d in datas[:4]])
        row["same_bits_as_pil"] = bool(np.array_equal(got, want.transpose(0, 3, 1, 2) if nc == 3 else want))
        print(json.dumps(row), flush=True)


def video_mode(args):
    import tempfile
    import numpy as np
    import torch
    from video_analytics_amd import _ffi, augment, pipeline, utils
    dev = torch.device("cuda", 0)
    T, H, W = args.frames, args.height, args.width
    jpegs = [encode(f, subsampling=2) for f in textured_frames(T, H, W)]
    params = _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)
    views = augment.ten_crop_views(H, W)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "v.avi")
        write_avi(path, jpegs)

        def with_pil():
            a = np.stack([np.asarray(f) for f in utils.iterVideoFrames(path)])
            return torch.from_numpy(a).to(dev).permute(0, 3, 1, 2).contiguous()
        pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
        runs = dict(pil_then_rgb=lambda: pipe.run_video(with_pil(), views=(views, views)),
                    path=lambda: pipe.run_video(path, views=(views, views)),
                    pil_then_rgb_again=lambda: pipe.run_video(with_pil(), views=(views, views)))
        s = dict((k, []) for k in runs)
        outs = {}
        for i in range(args.warmup + args.reps):  # interleaved
            for k, fn in runs.items():
                dt, outs[k] = _wall_ms(fn)
                if i >= args.warmup:
                    s[k].append(dt)
        same = all(torch.equal(outs["path"][key], outs["pil_then_rgb"][key]) for key in ("scores", "logits_s_items", "logits_t_items"))
        row = dict(metric="run_video_from_a_file_ms", frames=T, height=H, width=W, snippets=25, views=10, reps=args.reps,
                   bytes_per_frame=round(sum(map(len, jpegs)) / T), same_bits=bool(same),
                   tvl1="300 iters x 5 warps x 5 scales, exact math")
        for k, v in s.items():
            row.update(_stats(k + "_ms", v, 2))
        row["ratio"] = round(statistics.median(s["path"]) / statistics.median(s["pil_then_rgb"]), 4)
        row["ratio_same"] = round(statistics.median(s["pil_then_rgb_again"]) / statistics.median(s["pil_then_rgb"]), 4)
        print(json.dumps(row), flush=True)
        pipe.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["call", "video"])
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--flow-images", type=int, default=298)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 20 if args.mode == "call" else 5
    if args.warmup is None:
        args.warmup = 3 if args.mode == "call" else 1

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_jpeg.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    dict(call=call_mode, video=video_mode)[args.mode](args)


if __name__ == "__main__":
    main()
