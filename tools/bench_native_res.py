"""Clips/s of the two-stream pipeline on native-resolution clips (UCF-101: 320x240): TV-L1 on the full frames, the
crop and flip of getTransforms() on the device, both VGG-16 streams on the 224x224 crops.

Same schedule, batch and unpipelined step as bench.py's headline (which stays at 224x224); the crops are drawn on the host
every step, as the reference's data loader draws them.  ``--views ten`` evaluates every clip through the ten views of
``augment.ten_crop_views`` instead (B*10 images per stream, outputs averaged over the views).  ``--motion``
and ``--mean-flow`` choose the temporal input (trajectory stacking, bi-directional flow, mean flow subtraction; DESIGN.md
S11-S13).  Prints one JSON line.

    python tools/bench_native_res.py --steps 3 --warmup 1 [--height 240 --width 320 --batch 32 --flow-crops per_image]
                                     [--views none|ten] [--invert-flow-x] [--cnn-dtype f32|bf16]
                                     [--motion stack|trajectory|bidirectional] [--mean-flow]
"""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--flow-crops", choices=["per_image", "shared", "center"], default="per_image")
    ap.add_argument("--seed", type=int, default=0, help="seed of Python's random (the crop draws)")
    ap.add_argument("--views", choices=["none", "ten"], default="none",
                    help="none: one random crop per image (the reference); ten: ten-crop evaluation")
    ap.add_argument("--invert-flow-x", action="store_true", help="TSN flips: mirrored x-flow images become 255 - q")
    ap.add_argument("--cnn-dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--motion", choices=["stack", "trajectory", "bidirectional"], default="stack",
                    help="the temporal input: optical-flow stacking, trajectory stacking or bi-directional flow")
    ap.add_argument("--mean-flow", action="store_true", help="subtract every flow field's mean vector")
    args = ap.parse_args()

    import torch
    from video_analytics_amd import _ffi, augment, pipeline, synth
    from video_analytics_amd.parameters import VIDEO_INPUT_FLOW_COUNT as L

    if not torch.cuda.is_available():
        sys.stderr.write("bench_native_res.py: no GPU visible; the hot path has no CPU fallback\n")
        sys.exit(2)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    B, H, W = args.batch, args.height, args.width
    params = _ffi.default_tvl1_params(epsilon=0.0, iters=300, warps=5, nscales=5)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params, cnn_dtype=args.cnn_dtype, motion=args.motion,
                                      mean_flow=args.mean_flow)
    rgb, gray, _ = synth.synth_clips(B, seed=0, H=H, W=W)
    rgb, gray = rgb.to(dev), gray.to(dev)
    random.seed(args.seed)
    views = augment.ten_crop_views(H, W)

    def step():
        if args.views == "ten":
            return pipe.run_batch(rgb, gray, views=(views, views), invert_flow_x=args.invert_flow_x)
        crops = augment.draw_clip_crops(B, L, (H, W), (H, W), flow_mode=args.flow_crops)
        out = pipe.run_batch(rgb, gray, crops=crops, invert_flow_x=args.invert_flow_x)
        return out

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    finite = bool(torch.isfinite(out["logits_s"]).all().item() and torch.isfinite(out["logits_t"]).all().item())
    pipe.close()
    print(json.dumps(dict(metric="native_res_clips_per_s", value=round(B * args.steps / elapsed, 2), unit="clips/s",
                          height=H, width=W, batch=B, steps=args.steps, warmup=args.warmup, step_ms=round(1e3 * elapsed / args.steps, 2),
                          flow_crops=args.flow_crops, views=args.views, invert_flow_x=args.invert_flow_x,
                          cnn_dtype=args.cnn_dtype, motion=args.motion, mean_flow=args.mean_flow, tvl1="300 iters x 5 warps x 5 scales, exact math", finite=finite)))


if __name__ == "__main__":
    main()
