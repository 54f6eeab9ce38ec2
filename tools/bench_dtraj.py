"""The cost of dense-trajectory extraction on one MI355X.  Prints one JSON line per measurement.

    python tools/bench_dtraj.py [--frames 150] [--reps 5] [--warmup 1]

  dtraj_extract_ms  ``trajectories.dense_trajectories`` on --frames frames of 320x240 at the defaults (named here value by
                    value) with the flow given: a textured scene under a smooth, slowly changing flow of about 1.5 px.  HIP
                    events around the whole call (median filter, workspace and outputs included), median of --reps; the
                    trajectory count and the reject counts beside it.
  dtraj_kernel_ms   every stage alone through its test entry: votes, integral planes and corner response on one chunk of 8
                    frames; sample, step and finish per frame on a track table in its steady state (frames 15-29 of the
                    scene, each call between two events, median over those frames).  The integral's line carries the bytes
                    it moves (votes read, planes written, planes read and written again by the second pass) over its time,
                    beside the 8 TB/s HBM peak and the 6.29 TB/s a copy reaches (MI355X measurements).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULTS = dict(step=5, length=15, patch=32, nxy=2, nt=3, quality=0.001, min_flow=0.4, min_std=1.7320508, max_std=30.0, max_dis=20.0,
                max_dis_share=0.7)
W, H, CHUNK = 320, 240, 8
HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.29


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
    """gray uint8 [T,H,W]: a smooth texture; flow float32 [T-1,2,H,W]: smooth fields of about 1.5 px that change slowly"""
    import torch
    from video_analytics_amd import synth
    g = torch.Generator().manual_seed(0)
    tex = synth._blur(torch.rand(1, 1, H, W, generator=g), 1.0)[0, 0]
    tex = ((tex - tex.amin()) / (tex.amax() - tex.amin()) * 255.0).round().to(torch.uint8)
    gray = tex.unsqueeze(0).repeat(frames, 1, 1).contiguous()
    a, b = (synth._blur(torch.randn(2, 1, H, W, generator=g), 12.0)[:, 0] for _ in range(2))
    a, b = a / a.abs().amax() * 2.5, b / b.abs().amax() * 2.5
    t = torch.linspace(0.0, 1.0, frames - 1).view(-1, 1, 1, 1)
    flow = ((1.0 - t) * a + t * b).contiguous()
    return gray.to(dev), flow.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch
    from video_analytics_amd import _ffi, trajectories
    from video_analytics_amd import flow as vflow
    dev = torch.device("cuda", 0)
    gray, flow = scene(args.frames, dev)
    p = _ffi.default_dense_traj_params(**DEFAULTS)
    ms, out = [], None
    for i in range(args.warmup + args.reps):
        out, t = timed(lambda: trajectories.dense_trajectories(gray, flow, params=p))
        if i >= args.warmup:
            ms.append(t)
    print(json.dumps(dict(metric="dtraj_extract_ms", frames=args.frames, width=W, height=H, params=DEFAULTS, flow="given", reps=args.reps,
                          ms=round(statistics.median(ms), 3), ms_all=[round(t, 3) for t in ms], trajectories=out["count"],
                          rejected=out["rejected"], bound=trajectories.trajectory_bound(W, H, args.frames, p),
                          finite=bool(torch.isfinite(out["desc"]).all().item()),
                          reference_ms=None, note="the modelled project's Sheet02 (Python 2, cv2) cannot run here: no timing to set beside")),
          flush=True)

    L, ctx, st = _ffi.lib(), _ffi.ctx(0), _ffi.stream_ptr(dev)
    med = vflow.median_filter(flow, 3)
    n = CHUNK
    votes = torch.empty((n, 33, H, W), dtype=torch.int32, device=dev)
    integral = torch.empty((n, 33, H + 1, W + 1), dtype=torch.int32, device=dev)
    resp = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    mx = torch.empty((n,), dtype=torch.int32, device=dev)

    def run(name, *a):
        _ffi.check(getattr(L, name)(ctx, *a, st))

    def report(kernel, ms, **more):
        print(json.dumps(dict(metric="dtraj_kernel_ms", kernel=kernel, ms=round(statistics.median(ms), 4), ms_all=[round(t, 4) for t in ms],
                              **more)), flush=True)

    def reps(fn):
        return [timed(fn)[1] for _ in range(args.warmup + args.reps)][args.warmup:]

    t = reps(lambda: run("va_dtraj_votes", _ffi.ptr(gray), 1, _ffi.ptr(flow), n, W, H, ctypes.byref(p), _ffi.ptr(votes)))
    report("votes", t, frames=n, gpixels_per_s=round(n * W * H / statistics.median(t) / 1e6, 2),
           stored_tb_per_s=round(n * 33 * W * H * 4 / statistics.median(t) / 1e9, 3))
    t = reps(lambda: run("va_dtraj_integral", _ffi.ptr(votes), n * 33, W, H, _ffi.ptr(integral)))
    moved = n * 33 * 4 * (W * H + 3 * (W + 1) * (H + 1))
    report("integral", t, planes=n * 33, bytes_moved=moved, tb_per_s=round(moved / statistics.median(t) / 1e9, 3), hbm_peak_tb_per_s=HBM_PEAK_TBS,
           hbm_copy_tb_per_s=HBM_COPY_TBS)
    t = reps(lambda: run("va_dtraj_corner", _ffi.ptr(gray), 1, n, W, H, _ffi.ptr(resp), _ffi.ptr(mx)))
    report("corner", t, frames=n, gpixels_per_s=round(n * W * H / statistics.median(t) / 1e6, 2))

    # the per-frame stages on a table in its steady state: frames 0..29 of the scene, the last 15 are measured
    nbytes, _ = _ffi.dtraj_state_layout(W, H, p)
    state = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    cap = trajectories.trajectory_bound(W, H, 31 + DEFAULTS["length"], p)
    desc = torch.empty((cap, trajectories.descriptor_length(p)), dtype=torch.float32, device=dev)
    pts = torch.empty((cap, DEFAULTS["length"] + 1, 2), dtype=torch.float32, device=dev)
    starts = torch.empty((cap,), dtype=torch.int32, device=dev)
    times = dict(sample=[], step=[], finish=[])
    live = []
    for f in range(min(30, args.frames - 1)):
        run("va_dtraj_votes", _ffi.ptr(gray[f]), 1, _ffi.ptr(flow[f]), 1, W, H, ctypes.byref(p), _ffi.ptr(votes))
        run("va_dtraj_integral", _ffi.ptr(votes), 33, W, H, _ffi.ptr(integral))
        run("va_dtraj_corner", _ffi.ptr(gray[f]), 1, 1, W, H, _ffi.ptr(resp), _ffi.ptr(mx))
        ts = timed(lambda: run("va_dtraj_sample", _ffi.ptr(resp), _ffi.ptr(mx), W, H, f, ctypes.byref(p), _ffi.ptr(state)))[1]
        live.append(int(state[:4].view(torch.int32).item()))
        tp = timed(lambda: run("va_dtraj_step", _ffi.ptr(integral), _ffi.ptr(med[f]), W, H, f, ctypes.byref(p), _ffi.ptr(state)))[1]
        tf = timed(lambda: run("va_dtraj_finish", W, H, ctypes.byref(p), _ffi.ptr(state), _ffi.ptr(desc), _ffi.ptr(pts), _ffi.ptr(starts),
                               cap))[1]
        if f >= 15:
            times["sample"].append(ts), times["step"].append(tp), times["finish"].append(tf)
    for k, v in times.items():
        report(k, v, launches=dict(sample=2, step=1, finish=2)[k], frames_measured=len(v), live_tracks=round(statistics.median(live[15:])))


if __name__ == "__main__":
    main()
