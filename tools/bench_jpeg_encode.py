"""Timings of the JPEG encoder.  Prints one JSON line per workload.

    python tools/bench_jpeg_encode.py [--frames 150] [--height 240 --width 320] [--reps 20] [--warmup 3] [--threads 16]

Three workloads: the ``2 (T - 1)`` gray planes of a real ``extract_flow`` store of a T-frame video at quality 95 without
restart markers, the same planes with ``restartBlocks=40``, and T textured RGB frames at 4:2:0.  For each, interleaved in one
process, the median of ``--reps`` rounds beside the smallest and the largest:
  ``va_jpeg_encode_ms``   the two memsets and four launches alone, HIP events on the current stream, buffers allocated before;
  ``fdct_ms``             the first launch alone through its testing entry point;
  ``encode_jpegs_ms``     the whole call, wall clock: allocation, table upload, kernels, the synchronisation for the lengths,
                          the download of the scans and the headers written around them;
  ``pil_1_thread_ms`` / ``pil_N_threads_ms``   what a user had: the device-to-host copy of the pixels (``d2h_ms`` alone beside
                          it; for RGB the copy includes the NCHW -> NHWC permute on the device) and ``Image.save`` into memory
                          per image, on one host thread and on ``--threads``.
No file is written in any variant.  ``same_bytes_as_pil`` compares every file of one round.
"""
import argparse
import io
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_jpeg import _event_ms, _stats, _wall_ms, textured_frames  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_jpeg_encode.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from video_analytics_amd import _ffi, jpeg, pipeline, synth
    dev = torch.device("cuda", 0)
    T, H, W = args.frames, args.height, args.width
    params = _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    _, gray, _ = synth.synth_clips(1, seed=T, H=H, W=W, n_gray=T, device="cuda")
    store = pipe.extract_flow(gray[0].contiguous())
    pipe.close()
    planes = store.view(2 * store.shape[0], H, W).contiguous()
    frames = torch.from_numpy(textured_frames(T, H, W)).to(dev).permute(0, 3, 1, 2).contiguous()
    workloads = (("flow_gray", planes, None), ("flow_gray_restart_40", planes, 40), ("frames_420", frames, None))

    def pil_one(a, restart):
        buf = io.BytesIO()
        extra = {"subsampling": 2} if a.ndim == 3 else {}  # (on an 'L' image the keyword would change the header's sampling)
        if restart is not None:
            extra["restart_marker_blocks"] = restart
        Image.fromarray(a).save(buf, "JPEG", quality=95, **extra)
        return buf.getvalue()

    with ThreadPoolExecutor(args.threads) as pool:
        for name, images, restart in workloads:
            n, colour = int(images.shape[0]), images.dim() == 4
            shape = (n, W, H, 3, 2, 2) if colour else (n, W, H, 1, 1, 1)
            quant = jpeg.quant_tables(95)
            tables = jpeg.upload(jpeg.encode_tables(quant), dev)
            bufs = jpeg.encode_buffers(shape, restart or 0, dev)
            coef = torch.empty((n, jpeg.layout(*shape[1:])["blocks"], 64), dtype=torch.int16, device=dev)

            def fdct():
                _ffi.check(_ffi.lib().va_jpeg_fdct(_ffi.ctx(0), _ffi.ptr(images), _ffi.ptr(tables), *shape, _ffi.ptr(coef),
                                                   _ffi.stream_ptr(dev)))

            def to_host():
                return (images.permute(0, 2, 3, 1).contiguous() if colour else images).cpu().numpy()
            runs = dict(
                va_jpeg_encode=lambda: _event_ms(lambda: jpeg.encode_launch(images, shape, restart or 0, tables, *bufs)),
                fdct=lambda: _event_ms(fdct),
                encode_jpegs=lambda: _wall_ms(lambda: jpeg.encode_jpegs(images, 95, 2, restart)),
                d2h=lambda: _wall_ms(to_host),
                pil_1_thread=lambda: _wall_ms(lambda: [pil_one(a, restart) for a in to_host()]),
                pil_n_threads=lambda: _wall_ms(lambda: list(pool.map(lambda a: pil_one(a, restart), to_host()))))
            ms, last = dict((k, []) for k in runs), {}
            for i in range(args.warmup + args.reps):
                for k, fn in runs.items():  # interleaved
                    dt, last[k] = fn()
                    if i >= args.warmup:
                        ms[k].append(dt)
            files = last["encode_jpegs"]
            row = dict(metric="encode_jpegs_ms_per_call", workload=name, images=n, height=H, width=W, components=3 if colour else 1,
                       restart=restart or 0, bytes_per_image=round(sum(map(len, files)) / n), reps=args.reps,
                       workspace_bytes=bufs[3].numel(), out_bytes=bufs[0].numel(),
                       kernels=["k_jpeg_fdct", "k_jpeg_entropy_encode", "k_jpeg_stuff<false>", "k_jpeg_stuff<true>"],
                       same_bytes_as_pil=bool(files == last["pil_n_threads"]), status_clear=not bool(bufs[2].any()))
            for k, xs in ms.items():
                row.update(_stats(k.replace("pil_n_threads", "pil_%d_threads" % args.threads) + "_ms", xs, 3))
            row["encode_jpegs_over_pil_%d_threads" % args.threads] = round(
                statistics.median(ms["encode_jpegs"]) / statistics.median(ms["pil_n_threads"]), 4)
            row["encode_jpegs_over_pil_1_thread"] = round(statistics.median(ms["encode_jpegs"]) / statistics.median(ms["pil_1_thread"]), 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
