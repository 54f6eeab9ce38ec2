"""The cost of space-time interest points on one MI355X.  Prints one JSON line per measurement.

    python tools/bench_stip.py [--frames 150] [--reps 5] [--warmup 1] [--witness-pair 5,1 | --no-witness]

  stip_extract_ms   ``stip.space_time_interest_points`` on --frames frames of 320x240 at the defaults with the flow given:
                    a texture with drifting blobs under a smooth flow.  HIP events around the whole call (workspace and
                    outputs included), median of --reps; the point count beside it.
  stip_pair_ms      per scale pair, through ``va_stip_smooth``: the smoothing of L (three passes), the six integration
                    smoothings (eighteen passes), and ``rest``: the whole call's share of the pair minus both.  Each line
                    carries the bytes its passes move (one volume read and one written per pass) over its time beside the
                    8 TB/s HBM peak, and its float32 operations (one multiply, then an add, a multiply and an add per tap
                    pair) over its time beside the 157.3 TFLOP/s vector peak.
  stip_pass_ms      the widest smoothing (the integration scale of the largest pair) taken apart: x and y alone (tau 0.1 has
                    radius 0, its pass is a copy) and t alone (sigma 0.1 likewise), with the same two ratios and which peak
                    each is closer to.
  stip_witness_s    for scale, not as a race: scipy's float64 ``gaussian_filter`` chain of one scale pair (L and the six
                    products) on this host's CPU, ONE run.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 320, 240
HBM_PEAK_TBS, FP32_PEAK_TFLOPS = 8.0, 157.3


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


def scene(frames, dev):
    """gray uint8 [T,H,W]: a drifting texture with blobs that move and turn; flow float32 [T-1,2,H,W]: smooth, about 1.5 px"""
    import torch
    from video_analytics_amd import synth
    g = torch.Generator().manual_seed(0)
    tex = synth._blur(torch.rand(1, 1, H, W + frames, generator=g), 3.0)[0, 0]
    tex = (tex - tex.amin()) / (tex.amax() - tex.amin())
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    c = torch.rand(40, 4, generator=g)
    gray = torch.empty((frames, H, W), dtype=torch.uint8)
    for t in range(frames):
        f = 90.0 + 60.0 * tex[:, t:t + W]
        for cx, cy, ph, amp in c.tolist():
            x = cx * W + 20.0 * abs(((t / 15.0 + ph) % 2.0) - 1.0)
            f = f + (60.0 + 40.0 * amp) * torch.exp(-((xs - x) ** 2 + (ys - cy * H) ** 2) / 18.0)
        gray[t] = f.clamp(0, 255).round().to(torch.uint8)
    a, b = (synth._blur(torch.randn(2, 1, H, W, generator=g), 12.0)[:, 0] for _ in range(2))
    a, b = a / a.abs().amax() * 2.5, b / b.abs().amax() * 2.5
    tt = torch.linspace(0.0, 1.0, frames - 1).view(-1, 1, 1, 1)
    return gray.to(dev), ((1.0 - tt) * a + tt * b).contiguous().to(dev)


def radius(s):
    return int(4.0 * s + 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--witness-pair", default="5,1")
    ap.add_argument("--no-witness", action="store_true")
    args = ap.parse_args()
    import torch
    from video_analytics_amd import _ffi, stip
    dev = torch.device("cuda", 0)
    T = args.frames
    gray, flow = scene(T, dev)
    p = _ffi.default_stip_params()
    sigmas, taus, s = p.sigma_list, p.tau_list, float(p.integration)
    cap = 1 << 20
    try:
        stip.space_time_interest_points(gray, flow, params=p, max_points=cap)
    except ValueError as e:  # the message states the count found
        cap = int(str(e).split("found ")[1].split(" ")[0])
    ms, out = [], None
    for i in range(args.warmup + args.reps):
        out, t = timed(lambda: stip.space_time_interest_points(gray, flow, params=p, max_points=cap))
        if i >= args.warmup:
            ms.append(t)
    whole = statistics.median(ms)
    pairs = len(sigmas) * len(taus)
    print(json.dumps(dict(metric="stip_extract_ms", frames=T, width=W, height=H, scale_pairs=pairs, flow="given", reps=args.reps,
                          ms=round(whole, 3), ms_all=[round(t, 3) for t in ms], points=out["count"],
                          bound=stip.point_bound(W, H, T, p), finite=bool(torch.isfinite(out["desc"]).all().item()),
                          workspace_bytes=int(_ffi.lib().va_stip_workspace_bytes(W, H, T, cap, ctypes.byref(p))),
                          reference_ms=None, note="the modelled project's Sheet01 (Python 2, cv2) cannot run here: no timing to set beside")),
          flush=True)

    L, ctx, st = _ffi.lib(), _ffi.ctx(0), _ffi.stream_ptr(dev)
    vox = T * H * W
    n = 2 * vox + 2048
    tmp = torch.empty(n, dtype=torch.float32, device=dev)
    vol = torch.rand((T, H, W), dtype=torch.float32, device=dev)
    dst = torch.empty_like(vol)

    def smooth(src, u8, sig, tau):
        _ffi.check(L.va_stip_smooth(ctx, _ffi.ptr(src), u8, T, W, H, float(sig), float(tau), ctypes.byref(p), _ffi.ptr(dst), _ffi.ptr(tmp), n, st))

    def reps(fn):
        return [timed(fn)[1] for _ in range(args.warmup + args.reps)][args.warmup:]

    def ratios(t_ms, passes, rs, first_u8=False):
        """bytes and float32 operations of `passes` passes with radii rs over t_ms"""
        moved = sum(2 * vox * 4 for _ in range(passes)) - (3 * vox if first_u8 else 0)
        flops = sum(vox * (1 + 3 * r) for r in rs)
        tbs, tfl = moved / t_ms / 1e9, flops / t_ms / 1e9
        return dict(bytes_moved=moved, tb_per_s=round(tbs, 3), hbm_peak_tb_per_s=HBM_PEAK_TBS, share_of_hbm_peak=round(tbs / HBM_PEAK_TBS, 4),
                    flops=flops, tflop_per_s=round(tfl, 3), fp32_peak_tflop_per_s=FP32_PEAK_TFLOPS,
                    share_of_fp32_peak=round(tfl / FP32_PEAK_TFLOPS, 4), closer_to="fp32 vector peak" if tfl / FP32_PEAK_TFLOPS > tbs / HBM_PEAK_TBS else "HBM peak")

    total_smooth = 0.0
    for si, sig in enumerate(sigmas):
        for ti, tau in enumerate(taus):
            tl = statistics.median(reps(lambda: smooth(gray, 1, sig, tau)))
            t6 = 6.0 * statistics.median(reps(lambda: smooth(vol, 0, s * sig, s * tau)))
            total_smooth += tl + t6
            rl, ri = [radius(sig)] * 2 + [radius(tau)], [radius(s * sig)] * 2 + [radius(s * tau)]
            print(json.dumps(dict(metric="stip_pair_ms", sigma_index=si, tau_index=ti, sigma=round(sig, 4), tau=round(tau, 4), radii=rl,
                                  integration_radii=ri, smooth_L_ms=round(tl, 3), smooth_L=ratios(tl, 3, rl, True),
                                  integration_6_ms=round(t6, 3), integration_6=ratios(t6, 18, ri * 6))), flush=True)
    print(json.dumps(dict(metric="stip_pair_ms", summary=True, whole_ms=round(whole, 3), smoothing_ms=round(total_smooth, 3),
                          rest_ms=round(whole - total_smooth, 3), rest_per_pair_ms=round((whole - total_smooth) / pairs, 3),
                          note="rest: flow votes once, and per pair derivatives and products, response, maxima, votes, integral planes, "
                               "cuboids; and the workspace and output allocations of the call")), flush=True)

    sig, tau = s * sigmas[-1], s * taus[-1]
    copy = statistics.median(reps(lambda: smooth(vol, 0, 0.1, 0.1)))
    txy = statistics.median(reps(lambda: smooth(vol, 0, sig, 0.1)))
    tt = statistics.median(reps(lambda: smooth(vol, 0, 0.1, tau)))
    print(json.dumps(dict(metric="stip_pass_ms", what="three radius-0 passes (copies)", ms=round(copy, 3), **ratios(copy, 3, [0, 0, 0]))), flush=True)
    print(json.dumps(dict(metric="stip_pass_ms", what="x and y at the widest scale, t a copy", sigma=round(sig, 3), radius=radius(sig), ms=round(txy, 3),
                          less_one_copy_pass_ms=round(txy - copy / 3, 3), **ratios(txy - copy / 3, 2, [radius(sig)] * 2))), flush=True)
    print(json.dumps(dict(metric="stip_pass_ms", what="t at the widest scale, x and y copies", tau=round(tau, 3), radius=radius(tau), ms=round(tt, 3),
                          less_two_copy_passes_ms=round(tt - 2 * copy / 3, 3), **ratios(tt - 2 * copy / 3, 1, [radius(tau)]))), flush=True)

    if not args.no_witness:
        import numpy as np
        from scipy import ndimage
        si, ti = (int(v) for v in args.witness_pair.split(","))
        f = gray.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        Lw = ndimage.gaussian_filter(f, (taus[ti], sigmas[si], sigmas[si]), mode="reflect", truncate=4.0)
        lt, ly, lx = np.gradient(Lw)
        for c in (lx * lx, ly * ly, lt * lt, lx * ly, lx * lt, ly * lt):
            ndimage.gaussian_filter(c, (s * taus[ti], s * sigmas[si], s * sigmas[si]), mode="reflect", truncate=4.0)
        print(json.dumps(dict(metric="stip_witness_s", sigma_index=si, tau_index=ti, seconds=round(time.perf_counter() - t0, 2), runs=1,
                              note="scipy.ndimage.gaussian_filter, float64, one CPU thread, ONE run: for scale only")), flush=True)


if __name__ == "__main__":
    main()
