"""Host side of the two-pass warped optical flow: the numpy restatement of the warp that
tests/test_camera_rerun_gpu.py holds the kernel to (beside the S21 / S22 restatements of tests/test_camera_host.py), its
properties and an independent float64 witness, the claim of the form itself -- a pair warped by the exact homography leaves
TV-L1 nothing to find -- on the TV-L1 oracle, the refusal of bad options before anything reaches the GPU, and the stream
order of the second pass with the recorder of tests/test_pipeline_order_host.py."""
import json

import numpy as np
import pytest
import torch

import test_pipeline_order_host as order
from test_camera_host import same_bits

F32 = np.float32

# the planted camera of the form test: 1 % zoom, 0.02 rad rotation, (3, -2) px, a little perspective
H_STAR = np.array([[1.01 * np.cos(0.02), -np.sin(0.02), 3.0],
                   [np.sin(0.02), 1.01 * np.cos(0.02), -2.0],
                   [2e-5, -1e-5, 1.0]])


# ---- S53 restated ----

def warp_positions(Hm, h, w):
    """S53's positions in float64, S22's arithmetic: -> (px, py, inside) [h,w]."""
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        X = Hm[0, 0] * x + Hm[0, 1] * y + Hm[0, 2]
        Y = Hm[1, 0] * x + Hm[1, 1] * y + Hm[1, 2]
        D = Hm[2, 0] * x + Hm[2, 1] * y + Hm[2, 2]
        px, py = X / D, Y / D
        inside = (D > 0.0) & (px >= 0.0) & (px <= w - 1.0) & (py >= 0.0) & (py <= h - 1.0)  # a NaN fails every comparison
    return px, py, inside


def s53_warp_pairs(frames, Hs):
    """S53 restated: frames uint8 or float32 [S,F,h,w] (or [F,h,w]), Hs float64 [S*(F-1),3,3] -> float32 [S*(F-1),2,h,w].
    Double positions, the blend in float32 one rounding per operation (numpy float32 arrays: no fused multiply-add)."""
    frames = np.asarray(frames)
    if frames.ndim == 3:
        frames = frames[None]
    S, F, h, w = frames.shape
    N = S * (F - 1)
    Hs = np.asarray(Hs, dtype=np.float64).reshape(N, 3, 3)
    out = np.empty((N, 2, h, w), dtype=F32)
    for n in range(N):
        s, k = divmod(n, F - 1)
        fa, fb = frames[s, k].astype(F32), frames[s, k + 1].astype(F32)
        px, py, inside = warp_positions(Hs[n], h, w)
        px, py = np.where(inside, px, 0.0), np.where(inside, py, 0.0)
        fx0, fy0 = np.floor(px), np.floor(py)
        ax, ay = (px - fx0).astype(F32), (py - fy0).astype(F32)
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        A, B, C, D = fb[y0, x0], fb[y0, x1], fb[y1, x0], fb[y1, x1]
        t = A + ax * (B - A)
        b = C + ax * (D - C)
        val = t + ay * (b - t)
        assert t.dtype == F32 and val.dtype == F32
        out[n, 0] = fa
        out[n, 1] = np.where(inside, val, fa)
    return out


def near_identity(rs, n):
    """n homographies near the identity: 2 % linear part, 3 px translation, 2e-5 perspective."""
    Hs = np.tile(np.eye(3), (n, 1, 1))
    Hs[:, :2, :2] += rs.uniform(-0.02, 0.02, (n, 2, 2))
    Hs[:, :2, 2] = rs.uniform(-3.0, 3.0, (n, 2))
    Hs[:, 2, :2] = rs.uniform(-2e-5, 2e-5, (n, 2))
    return Hs


def shift_homography(dx, dy):
    return np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])


def crossing_homography(x_zero):
    """D = 1 - x / x_zero: positive left of column x_zero, zero on it, negative beyond."""
    Hm = np.eye(3)
    Hm[2, 0] = -1.0 / x_zero
    return Hm


def gray_frames(rs, shape, dtype):
    """Gray frames of the given dtype: uint8 noise, or float32 with fractional values in [0, 255]."""
    if dtype == np.uint8:
        return rs.randint(0, 256, shape).astype(np.uint8)
    return (rs.uniform(0.0, 255.0, shape)).astype(F32)


@pytest.mark.parametrize("dtype", [np.uint8, F32])
def test_the_identity_returns_both_frames_bits(dtype):
    rs = np.random.RandomState(1)
    fr = gray_frames(rs, (2, 3, 29, 37), dtype)
    out = s53_warp_pairs(fr, np.tile(np.eye(3), (4, 1, 1)))
    f = fr.astype(F32)
    for n in range(4):
        s, k = divmod(n, 2)
        assert same_bits(out[n, 0], f[s, k]) and same_bits(out[n, 1], f[s, k + 1])


@pytest.mark.parametrize("dtype", [np.uint8, F32])
def test_an_integer_shift_returns_the_shifted_frame_inside_and_frame_k_outside(dtype):
    h, w = 29, 37
    fr = gray_frames(np.random.RandomState(2), (1, 2, h, w), dtype)
    out = s53_warp_pairs(fr, shift_homography(3.0, -2.0)[None])
    f = fr.astype(F32)
    want = f[0, 0].copy()
    want[2:, :w - 3] = f[0, 1][:h - 2, 3:]  # pixel (x, y) reads (x + 3, y - 2) of frame k + 1 where that lies in the frame
    assert same_bits(out[0, 0], f[0, 0]) and same_bits(out[0, 1], want)
    assert not same_bits(out[0, 1], f[0, 0])


def test_a_crossing_denominator_and_a_nan_fall_back_to_frame_k():
    h, w = 29, 37
    fr = gray_frames(np.random.RandomState(3), (3, 2, h, w), F32)
    nan_h = np.eye(3)
    nan_h[0, 1] = np.nan
    neg = -np.eye(3)  # the same map as the identity up to sign, but D < 0 everywhere
    out = s53_warp_pairs(fr, np.stack([crossing_homography(18.0), nan_h, neg]))
    assert same_bits(out[0, 1][:, 18:], fr[0, 0][:, 18:])       # D <= 0 from column 18 on
    assert same_bits(out[0, 1][:, 0], fr[0, 1][:, 0])           # x = 0: D = 1, the identity's position
    assert not same_bits(out[0, 1][:, :18], fr[0, 0][:, :18])
    assert same_bits(out[1, 1], fr[1, 0]) and same_bits(out[1, 0], fr[1, 0])   # the pair (f_k, f_k)
    assert same_bits(out[2, 1], fr[2, 0])
    assert np.isfinite(out).all()


@pytest.mark.parametrize("h,w", [(29, 37), (128, 96)])
@pytest.mark.parametrize("dtype", [np.uint8, F32])
def test_restatement_agrees_with_map_coordinates(h, w, dtype):
    """An independent witness: scipy's order-1 spline in float64 at the same double positions.  The restatement rounds to
    float32 eight times on the way to a value: ax and ay themselves, three operations in a row's blend (the two rows enter
    the result with weights that sum to 1, so they count once) and three in the blend between the rows.  Every rounded
    quantity is at most 255, so each rounding is at most 255 * 2^-24 = 1.52e-5 and the eight stay below 2e-4 gray levels."""
    ndimage = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(h)
    fr = gray_frames(rs, (2, 3, h, w), dtype)
    Hs = near_identity(rs, 4)
    out = s53_warp_pairs(fr, Hs)
    worst, n_inside = 0.0, 0
    for n in range(4):
        s, k = divmod(n, 2)
        px, py, inside = warp_positions(Hs[n], h, w)
        wit = ndimage.map_coordinates(fr[s, k + 1].astype(np.float64), [py[inside], px[inside]], order=1, mode="nearest")
        worst = max(worst, float(np.abs(out[n, 1][inside].astype(np.float64) - wit).max()))
        n_inside += int(inside.sum())
        assert same_bits(out[n, 1][~inside], fr[s, k].astype(F32)[~inside])
    print("%dx%d %s: %.3g gray levels over %d inside pixels" % (w, h, np.dtype(dtype).name, worst, n_inside))
    assert n_inside > 0.8 * 4 * h * w
    assert worst <= 2e-4, worst


# ---- the form does what it claims ----

def planted_scene(h=128, w=96, Hm=H_STAR, seed=0, margin=16):
    """Two float64 frames [2,h,w]: a texture (Gaussian-filtered noise, sigma 2, scaled to [0,255], sampled bicubically) and
    the same texture seen by a camera that moved by ``Hm``: frame 1 at q holds what frame 0 holds at Hm^-1 q."""
    ndimage = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(seed)
    tex = ndimage.gaussian_filter(rs.standard_normal((h + 2 * margin, w + 2 * margin)), 2.0)
    tex = (tex - tex.min()) * (255.0 / (tex.max() - tex.min()))
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    inv = np.linalg.inv(Hm)
    p = np.einsum("ij,jhw->ihw", inv, np.stack([x, y, np.ones_like(x)]))
    f0 = ndimage.map_coordinates(tex, [y + margin, x + margin], order=3, mode="nearest")
    f1 = ndimage.map_coordinates(tex, [p[1] / p[2] + margin, p[0] / p[2] + margin], order=3, mode="nearest")
    return np.clip(np.stack([f0, f1]), 0.0, 255.0)


@pytest.mark.parametrize("dtype", [np.uint8, F32])
def test_a_pair_warped_by_the_exact_homography_has_no_flow_left(oracle_tvl1, dtype):
    """96 x 128 (width x height), the oracle's TV-L1 with its default parameters.  Measured with the committed oracle on
    this scene (seed 0): uint8 frames median 0.0139, 99th percentile 0.0467, maximum 0.42 px; float frames 0.0135, 0.0487,
    0.15 px; plain flow median 2.26 px; 95.2 % of the pixels inside.  The bounds, 0.05 and 0.2 px, are the issue's: about 3.5
    times what its own run of such a scene gave (0.014 and 0.056 px)."""
    h, w = 128, 96
    scene = planted_scene(h, w)
    fr = np.rint(scene).astype(np.uint8) if dtype == np.uint8 else scene.astype(F32)
    pairs = s53_warp_pairs(fr, H_STAR[None])
    _, _, inside = warp_positions(H_STAR, h, w)
    plain = oracle_tvl1.tvl1_flow(fr[None], oracle_tvl1.default_params(), nthreads=0)
    left = oracle_tvl1.tvl1_flow(pairs, oracle_tvl1.default_params(), nthreads=0)
    mag = np.hypot(left[0, 0], left[0, 1])[inside]
    plain_mag = np.hypot(plain[0, 0], plain[0, 1])[inside]
    med, p99 = float(np.median(mag)), float(np.percentile(mag, 99))
    print("%s: residual median %.4f, 99th percentile %.4f, maximum %.4f px; plain flow median %.3f px; %.1f %% inside"
          % (np.dtype(dtype).name, med, p99, float(mag.max()), float(np.median(plain_mag)), 100.0 * inside.mean()))
    assert inside.mean() > 0.9 and float(np.median(plain_mag)) > 2.0
    assert med < 0.05, med
    assert p99 < 0.2, p99


# ---- option checks: before anything reaches the GPU ----

@pytest.fixture
def no_gpu_calls(monkeypatch):
    """Every path to the device raises AssertionError: a ValueError seen with it comes from a host check."""
    from video_analytics_amd import _ffi
    from video_analytics_amd import flow as vflow

    def boom(*a, **k):
        raise AssertionError("reached the GPU")
    for mod, name in ((_ffi, "ctx"), (_ffi, "lib"), (vflow, "tvl1_flow"), (vflow, "tvl1_flow_concurrent")):
        monkeypatch.setattr(mod, name, boom)


def test_the_form_names_and_defaults(no_gpu_calls):
    import inspect
    from video_analytics_amd import pipeline
    from video_analytics_amd import flow as vflow
    from video_analytics_amd.temporalModel import flowVolumesFromFrames
    assert vflow.CAMERA_FORMS == ("subtract", "rerun") and vflow.CAMERAS == ("none", "homography")
    for form in vflow.CAMERA_FORMS:
        vflow.check_camera_form(form, "x")
        vflow.check_camera_form(form, "x", "homography")
    vflow.check_camera_form("subtract", "x", "none")
    for f in (vflow.apply_motion, flowVolumesFromFrames, pipeline.TwoStreamPipeline.__init__):
        p = inspect.signature(f).parameters["camera_form"]
        assert p.default == "subtract" and p.kind == inspect.Parameter.KEYWORD_ONLY, f
    assert inspect.signature(vflow.apply_motion).parameters["frames"].kind == inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(vflow.apply_camera).parameters) == ["flow", "camera", "in_place"]
    assert list(inspect.signature(vflow.rerun_camera).parameters) == ["frames", "flow", "params", "out"]
    assert list(inspect.signature(vflow.warp_pairs).parameters) == ["frames", "H", "out"]
    flow = torch.zeros(2, 2, 8, 8)
    assert vflow.apply_motion(flow, 2, camera_form="subtract") is flow  # no camera: no kernel, no buffer, whatever the form


@pytest.mark.parametrize("form", ["Rerun", "twice", None, 1, ("rerun",)])
def test_an_unknown_form_is_refused_on_the_host(no_gpu_calls, form):
    from video_analytics_amd import pipeline
    from video_analytics_amd import flow as vflow
    from video_analytics_amd.temporalModel import flowVolumesFromFrames
    gray = torch.zeros(2, 11, 240, 320, dtype=torch.uint8)
    with pytest.raises(ValueError, match="camera_form"):
        vflow.check_camera_form(form, "x")
    for camera in ("none", "homography"):
        with pytest.raises(ValueError, match="camera_form"):
            flowVolumesFromFrames(gray, camera=camera, camera_form=form)
        with pytest.raises(ValueError, match="camera_form"):
            pipeline.TwoStreamPipeline(device=0, camera=camera, camera_form=form)


def test_rerun_without_a_camera_is_refused_on_the_host(no_gpu_calls):
    from video_analytics_amd import pipeline
    from video_analytics_amd import flow as vflow
    from video_analytics_amd.temporalModel import flowVolumesFromFrames
    gray = torch.zeros(2, 11, 240, 320, dtype=torch.uint8)
    with pytest.raises(ValueError, match="rerun"):
        vflow.check_camera_form("rerun", "x", "none")
    with pytest.raises(ValueError, match="rerun"):
        flowVolumesFromFrames(gray, camera_form="rerun")
    with pytest.raises(ValueError, match="rerun"):
        pipeline.TwoStreamPipeline(device=0, camera_form="rerun")
    with pytest.raises(ValueError, match="rerun"):
        pipeline.TwoStreamPipeline(device=0, camera="none", camera_form="rerun", motion="trajectory")


def test_rerun_helpers_refuse_bad_arguments_on_the_host(no_gpu_calls):
    from video_analytics_amd import flow as vflow
    dev = order.dev
    cpu_flow, cpu_frames = torch.zeros(4, 2, 8, 9), torch.zeros(2, 3, 8, 9, dtype=torch.uint8)
    flow, frames = dev(cpu_flow.clone()), dev(cpu_frames.clone())
    eye = dev(torch.eye(3, dtype=torch.float64).repeat(4, 1, 1))
    bad = [lambda: vflow.apply_motion(flow, 2, camera="homography", camera_form="rerun"),          # no frames
           lambda: vflow.apply_motion(cpu_flow, 2, camera="homography", camera_form="rerun", frames=cpu_frames),
           lambda: vflow.warp_pairs(cpu_frames, eye),                                              # not on the device
           lambda: vflow.warp_pairs(frames.double(), eye), lambda: vflow.warp_pairs(frames[0, 0], eye),
           lambda: vflow.warp_pairs(frames[:, :1], eye[:0]),                                       # one frame: no pair
           lambda: vflow.warp_pairs(frames, eye[:3]), lambda: vflow.warp_pairs(frames, eye.float()),
           lambda: vflow.warp_pairs(frames, eye.as_subclass(torch.Tensor)),                        # H on the host
           lambda: vflow.warp_pairs(frames, eye, out=dev(torch.zeros(3, 2, 8, 9))),
           lambda: vflow.warp_pairs(frames, eye, out=dev(torch.zeros(4, 2, 8, 9, dtype=torch.float64))),
           lambda: vflow.rerun_camera(frames, flow[:3]), lambda: vflow.rerun_camera(cpu_frames, flow),
           lambda: vflow.rerun_camera(frames, cpu_flow), lambda: vflow.rerun_camera(frames, dev(torch.zeros(4, 2, 9, 8)))]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d was accepted" % i)
    f32 = dev(torch.zeros(2, 3, 8, 9))
    buf = dev(torch.zeros(2 * 3 * 8 * 9 + 4 * 2 * 8 * 9))
    with pytest.raises(ValueError, match="overlap"):
        vflow.warp_pairs(buf[:f32.numel()].view(f32.shape), eye, out=buf[8:8 + 4 * 2 * 8 * 9])


def test_a_rerun_pipeline_refuses_what_a_camera_pipeline_refuses(no_gpu_calls):
    """``flow_stack=`` is already quantised: refused before anything is enqueued, whatever the form."""
    from video_analytics_amd import pipeline
    pipe = pipeline.TwoStreamPipeline.__new__(pipeline.TwoStreamPipeline)
    pipe.motion, pipe.mean_flow, pipe.camera, pipe.camera_form, pipe._n = "stack", False, "homography", "rerun", 0
    with pytest.raises(ValueError, match="camera"):
        pipe.submit(torch.zeros(2, 3, 224, 224, dtype=torch.uint8), None, flow_stack=torch.zeros(2, 20, 224, 224))
    assert pipe._n == 0 and pipe._rerun()
    pipe.camera_form = "subtract"
    assert not pipe._rerun()
    del pipe.camera_form  # a pipeline built attribute by attribute before the option existed
    assert not pipe._rerun()


# ---- the stream order ----

def install_rerun(mp):
    """The order test's recorder, with the pairs bank among the named buffers and recording stand-ins for the three steps
    of the second pass -> the Recorder."""
    from video_analytics_amd import flow as vflow
    rec = order.install(mp)
    mp.setattr(order, "BANKS", order.BANKS + ("_pairs",))

    def fit_homography(fl, *a, **k):
        rec.log("fit_homography", rec.current[-1], rec.desc(fl))
        return torch.zeros(fl.shape[0], 3, 3, dtype=torch.float64), torch.zeros(fl.shape[0], 2, dtype=torch.float64)

    def warp_pairs(frames, H, out=None):
        rec.log("warp_pairs", rec.current[-1], rec.desc(frames), rec.desc(out))
        S, F, h, w = frames.shape
        return out if out is not None else torch.empty((S * (F - 1), 2, h, w))

    def tvl1_flow(frames, params=None, ws_slot=0, out=None, **over):
        slot = ws_slot if not isinstance(ws_slot, tuple) else ws_slot[0] + "/own"
        rec.log("tvl1_flow", rec.current[-1], rec.desc(frames), rec.desc(out), slot)
        return out

    mp.setattr(vflow, "fit_homography", fit_homography)
    mp.setattr(vflow, "warp_pairs", warp_pairs)
    mp.setattr(vflow, "tvl1_flow", tvl1_flow)
    return rec


def record_rerun(scenario):
    with pytest.MonkeyPatch.context() as mp:
        rec = install_rerun(mp)
        scenario(rec)
    return rec.trace, rec.n_events


def three_submits(rec, **kw):
    from video_analytics_amd import augment
    import random
    pipe = order.make_pipe(rec, camera="homography", mean_flow=True, **kw)
    rgb, gray = order.batch(2, 240, 320)
    crops = augment.draw_clip_crops(2, order.L, (240, 320), (240, 320), rng=random.Random(3))
    for _ in range(3):  # the third reuses slot 0 and waits for its flow-read event
        pipe.submit(rgb, gray, crops=crops)
    pipe.wait()
    return pipe


def one_video(rec, **kw):
    from video_analytics_amd import augment
    pipe = order.make_pipe(rec, camera="homography", **kw)
    v = augment.ten_crop_views(240, 320)
    pipe.submit_video(*order.clip(20, 240, 320), n_snippets=3, views=(v, v))
    pipe.wait()
    return pipe


SECOND_PASS = ("fit_homography", "warp_pairs", "tvl1_flow")


def _positions(trace, name, stream="cnn"):
    return [i for i, e in enumerate(trace) if e[0] == name and e[1] == stream]


def test_the_second_pass_runs_on_the_cnn_stream_between_the_tvl1_events_and_the_gather():
    trace, n_events = record_rerun(lambda rec: three_submits(rec, camera_form="rerun"))
    fits, warps, passes = (_positions(trace, name) for name in SECOND_PASS)
    gathers = _positions(trace, "crop_flow_to_stack")
    assert len(fits) == len(warps) == len(passes) == len(gathers) == 3
    tv_events = [[e[2] for e in trace[:fits[j]] if e[0] == "record" and e[1].startswith("flow")][-2:] for j in range(3)]
    for j in range(3):
        k = j % 2
        waits = [i for i, e in enumerate(trace) if e[0] == "wait_event" and e[1] == "cnn" and e[2] in tv_events[j]]
        assert len(waits) == 2 and max(waits) < fits[j] < warps[j] < passes[j] < gathers[j], (j, waits)
        assert trace[fits[j]][2] == "flow[%d]:20x2x240x320" % k
        assert trace[warps[j]][2:] == ["2x11x240x320", "pairs[%d]:20x2x240x320" % k]
        # the second pass reads the slot's pairs, writes the slot's flow buffer, and has a workspace of the pipeline's own
        assert trace[passes[j]][2:] == ["pairs[%d]:20x2x240x320" % k, "flow[%d]:20x2x240x320" % k, "rerun/own"]
        # the TV-L1 input is handed to the CNN stream before the warp reads it there
        assert ["record_stream", "cnn", "2x11x240x320", "cnn"] in trace[max(waits):warps[j]]
        # the flow-read event follows the gather, the last reader of the slot's flow buffer ...
        after = trace[gathers[j] + 1]
        assert after[:2] == ["record", "cnn"], after
        if j == 0:  # ... and the TV-L1 of the third batch, which writes slot 0 again, waits for it on both flow streams
            third = [e for e in trace[gathers[1]:] if e[0] == "wait_event" and e[2] == after[2]]
            assert sorted(e[1] for e in third) == ["flow0", "flow1"], third
    # nothing of the second pass runs anywhere but on the CNN stream
    assert all(e[1] == "cnn" for e in trace if e[0] in SECOND_PASS)
    # the default choreography is untouched: no event more than the subtract form's, and the same trace around the step
    base, base_events = record_rerun(lambda rec: three_submits(rec, camera_form="subtract"))
    assert n_events == base_events
    ours = [e for e in trace if e[0] not in SECOND_PASS and e != ["record_stream", "cnn", "2x11x240x320", "cnn"]]
    theirs = [e for e in base if e[0] != "apply_camera"]
    assert ours == theirs
    assert [e for e in base if e[0] == "apply_camera"] == [["apply_camera", "cnn", "flow[%d]:20x2x240x320" % (j % 2), "homography",
                                                            True] for j in range(3)]
    assert not [e for e in base if e[0] in SECOND_PASS or "pairs" in json.dumps(e)]


def test_the_second_pass_of_a_video_and_of_a_training_step():
    trace, _ = record_rerun(lambda rec: one_video(rec, camera_form="rerun"))
    fit, warp, second = (_positions(trace, name)[0] for name in SECOND_PASS)
    gather = _positions(trace, "crop_flow_to_stack_snippets")[0]
    last_wait = max(i for i, e in enumerate(trace[:fit]) if e[0] == "wait_event" and e[1] == "cnn")
    assert last_wait < fit < warp < second < gather
    n_pairs = int(trace[fit][2].split(":")[1].split("x")[0])
    assert trace[warp][2:] == ["%dx2x240x320" % n_pairs, "pairs[0]:%dx2x240x320" % n_pairs]  # one two-frame sequence per planned pair
    assert trace[second][2:] == ["pairs[0]:%dx2x240x320" % n_pairs, "flow[0]:%dx2x240x320" % n_pairs, "rerun/own"]
    assert trace[gather + 1][:2] == ["record", "cnn"]

    def train(rec):
        pipe = order.make_pipe(rec, camera="homography", camera_form="rerun")
        crops = torch.tensor([[0, 0, 224, 224, 0], [0, 0, 224, 224, 1]], dtype=torch.int32)
        pipe.train_videos([order.clip(), order.clip()], [3, 4], k=1, starts=[[2], [5]], crops=crops)
    trace, _ = record_rerun(train)
    steps = [e for e in trace if e[0] in SECOND_PASS]
    assert [e[:2] for e in steps] == [[name, "caller"] for name in SECOND_PASS]  # in order on the current stream
    assert steps[2][4] == "rerun"  # the shared slot of the current-stream callers: not 0, not a flow stream's
    first = [i for i, e in enumerate(trace) if e[0] == "tvl1_flow_concurrent"][0]
    assert first < trace.index(steps[0]) < [i for i, e in enumerate(trace) if e[0] == "resize_flow_to_stack"][0]


def test_subtract_spelled_out_builds_the_default_pipeline():
    """``camera_form="subtract"`` is the default: the same attributes, no pairs buffer, and the committed trace of the camera
    scenario operation for operation."""
    def scenario(rec):
        three_submits(rec, camera_form="subtract")
        assert rec.pipe.camera_form == "subtract" and rec.pipe._pairs == [None, None] and not rec.pipe._rerun()

    def default(rec):
        three_submits(rec)
        assert rec.pipe.camera_form == "subtract" and rec.pipe._pairs == [None, None]
    assert record_rerun(scenario) == record_rerun(default)
    with open(order.GOLDEN) as f:
        golden = json.load(f)

    def s3(rec, **kw):  # tests/test_pipeline_order_host.py: s3_crops_camera_mean_flow
        from video_analytics_amd import augment
        import random
        pipe = order.make_pipe(rec, camera="homography", mean_flow=True, **kw)
        rgb, gray = order.batch(2, 240, 320)
        crops = augment.draw_clip_crops(2, order.L, (240, 320), (240, 320), rng=random.Random(3))
        for _ in range(2):
            pipe.submit(rgb, gray, crops=crops, invert_flow_x=True)
        pipe.wait()
    with pytest.MonkeyPatch.context() as mp:
        rec = order.install(mp)
        s3(rec, camera_form="subtract")
    assert rec.trace == golden["s3_crops_camera_mean_flow"]


def test_the_default_scenarios_still_match_the_golden():
    with open(order.GOLDEN) as f:
        golden = json.load(f)
    for scenario in order.SCENARIOS:
        assert order.record(scenario) == golden[scenario.__name__], scenario.__name__
