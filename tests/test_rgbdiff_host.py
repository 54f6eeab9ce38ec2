"""RGB difference, host side: float32 numpy restatements of the difference volume (S23) and of the fusion
of m streams (S24), each held to an independent witness with a bound derived here; the two test videos and the conditions
they must meet; the table helpers' known answers; and the refusal of every bad argument before anything reaches the GPU.
tests/test_rgbdiff_gpu.py holds the kernels and the pipeline to these restatements bit for bit."""
import math
import types

import numpy as np
import pytest
import torch

from test_tsn_host import s17_images_u8, s17_taps
from test_video_host import fuse_f64, no_gpu_calls, s16_fuse  # noqa: F401  (no_gpu_calls is a fixture)

F32 = np.float32
EPS = 2.0 ** -24  # unit roundoff of float32
OUT = 224
STDS = (0.229, 0.224, 0.225)


# ---- S23 restated ----

def s23_resampled(win, row):
    """win uint8 [F,3,h,w], the frames of one window; row {src, top, left, ch, cw, flip} -> int32 [F,3,224,224]: every frame
    and channel through S17's taps and S12's bilinear form in float32, clamped, rounded to nearest even (the u8 value
    va_resize_images_u8 writes)."""
    _, top, left, ch, cw, flip = (int(v) for v in row)
    x0, x1, ax = s17_taps(cw, bool(flip))[:3]
    y0, y1, ay = s17_taps(ch)[:3]
    f = win.astype(F32)
    ra, rb = f[:, :, top + y0, :], f[:, :, top + y1, :]
    A, B, C, D = ra[..., left + x0], ra[..., left + x1], rb[..., left + x0], rb[..., left + x1]
    t = A + ax * (B - A)
    b = C + ax * (D - C)
    val = t + ay[:, None] * (b - t)
    assert val.dtype == F32
    return np.rint(np.minimum(np.maximum(val, F32(0.0)), F32(255.0))).astype(np.int32)


def s23_den(stds=STDS):
    """den[c] = 255.0f * (float)std[c], rounded to float32 once."""
    return (F32(255.0) * np.asarray(stds, dtype=F32)).astype(F32)


def s23_stack(frames, table, D, stds=STDS, layout="NCHW", want_int=False):
    """frames uint8 [T,3,h,w] (or [T,h,w,3]), table int [n_out,6] -> float32 [n_out,3D,224,224]: plane 3j + c =
    (float)(r[j+1,c] - r[j,c]) / den[c], one float32 division (va_rgbdiff_to_stack).  ``want_int``: also the integer
    differences int32 [n_out,D,3,224,224]."""
    if layout == "NHWC":
        frames = frames.transpose(0, 3, 1, 2)
    den = s23_den(stds)
    out = np.empty((len(table), 3 * D, OUT, OUT), dtype=F32)
    ints = np.empty((len(table), D, 3, OUT, OUT), dtype=np.int32) if want_int else None
    for o, row in enumerate(np.asarray(table).tolist()):
        q = s23_resampled(frames[row[0]:row[0] + D + 1], row)
        d = q[1:] - q[:-1]                                       # [D,3,224,224], exact integers
        out[o] = (d.astype(F32) / den[None, :, None, None]).reshape(3 * D, OUT, OUT)
        if want_int:
            ints[o] = d
    assert out.dtype == F32
    return (out, ints) if want_int else out


# ---- the two test videos ----

def noise_video(T, h, w, seed):
    """uint8 [T,3,h,w]: independent uniform noise in every frame."""
    return np.random.RandomState(seed).randint(0, 256, size=(T, 3, h, w)).astype(np.uint8)


def moving_video(T, h, w, seed):
    """uint8 [T,3,h,w]: one texture of 5-pixel-wide columns of constant value, moved left by one pixel per frame, so that a
    pixel's difference is zero inside a column and the step between two columns at its edge."""
    rs = np.random.RandomState(seed)
    tex = np.repeat(rs.randint(0, 256, size=(3, h, (w + T) // 5 + 2)), 5, axis=2).astype(np.uint8)
    return np.stack([tex[:, :, t:t + w] for t in range(T)])


def jitter_rows(h, w, n_first, offsets=(0, 9)):
    """The table rows of the tests: every scale-jitter size pair x the fixed offsets ``offsets`` x both flips, two rows of
    the network's own size where the frame holds them (one mirrored), a 1x1 and a 3x2 rectangle; ``src`` cycles through the
    ``n_first`` possible first frames, so that windows repeat and overlap."""
    from video_analytics_amd import augment
    rows = []
    _, pairs = augment.scale_jitter_sizes(h, w)
    for cw, ch in pairs:
        if cw > w or ch > h:
            continue
        offs = augment.fixed_offsets(h, w, ch, cw)
        for i in offsets:
            for flip in (0, 1):
                rows.append((offs[i][1], offs[i][0], ch, cw, flip))
    if h >= OUT and w >= OUT:
        rows += [(h - OUT, w - OUT, OUT, OUT, 0), ((h - OUT) // 2, 1, OUT, OUT, 1)]
    rows += [(h - 1, w - 1, 1, 1, 0), (h // 2, w // 3, 2, 3, 1)]   # {top, left, ch, cw, flip}: 1x1, and 3 wide x 2 high
    return np.array([(i % n_first,) + r for i, r in enumerate(rows)], dtype=np.int32)


@pytest.mark.parametrize("h,w,D", [(37, 29, 3), (60, 81, 1), (240, 320, 2)])
def test_s23_restatement_is_the_difference_of_resized_images_and_within_three_roundings_of_float64(h, w, D):
    T = D + 3
    frames = noise_video(T, h, w, seed=h + D)
    table = jitter_rows(h, w, T - D)
    if h == 240:
        table = table[[0, 7, 21, 38, 40, 41, 42, 43]]  # a few of each kind: the full set runs on the device
    for layout in ("NCHW", "NHWC"):
        x = frames if layout == "NCHW" else np.ascontiguousarray(frames.transpose(0, 2, 3, 1))
        got, ints = s23_stack(x, table, D, layout=layout, want_int=True)
        # the D + 1 frames of each row through the S17 restatement of va_resize_images_u8, then subtracted as integers
        for j in range(D + 1):
            tj = table.copy()
            tj[:, 0] += j
            r = s17_images_u8(x, tj, layout).astype(np.int32)
            if j > 0:
                assert np.array_equal(ints[:, j - 1], r - prev), (layout, j)
            prev = r
        # The float64 witness w = (a - b) / (255 * std_c).  The float32 value differs from it by three roundings: std_c to
        # float32, the product 255 * std_c (together "den"), and the one division; a - b is an exact integer.  Each moves the
        # value by at most 2^-24 of its size: |got - w| <= 3 * 2^-24 * |w|.
        wit = ints.astype(np.float64) / (255.0 * np.asarray(STDS, dtype=np.float64))[None, None, :, None, None]
        wit = wit.reshape(got.shape)
        err = np.abs(got.astype(np.float64) - wit)
        print("S23 %dx%d D=%d %s: worst |restatement - witness| / |witness| = %.3g (bound %.3g)"
              % (w, h, D, layout, float((err[wit != 0] / np.abs(wit[wit != 0])).max()), 3 * EPS))
        assert (err <= 3 * EPS * np.abs(wit)).all()
        assert (got[wit == 0] == 0).all()


def test_the_test_videos_meet_their_conditions():
    """What tests/test_rgbdiff_gpu.py relies on: noise gives differences of both signs up to the ends of the range; the
    moving texture gives exact zeros and both signs."""
    h, w, D = 60, 81, 2
    table = jitter_rows(h, w, 3)
    _, d = s23_stack(noise_video(D + 3, h, w, 1), table, D, want_int=True)
    assert d.min() < 0 < d.max() and np.abs(d).max() >= 200
    _, d = s23_stack(moving_video(D + 3, h, w, 2), table, D, want_int=True)
    assert d.min() < 0 < d.max() and (d == 0).any()
    assert (d == 0).mean() > 0.3                      # inside the columns nothing changes
    full = moving_video(8, 240, 320, 3)
    assert np.array_equal(full[1][:, :, :-1], full[0][:, :, 1:])  # one pixel per frame


# ---- the tables ----

def test_view_table_and_window_table_known_answers():
    from video_analytics_amd import rgbdiff
    views = torch.tensor([[0, 0, 0], [16, 96, 1]], dtype=torch.int32)
    t = rgbdiff.view_table([3, 7, 3], views)
    assert t.dtype == torch.int32 and t.tolist() == [
        [3, 0, 0, 224, 224, 0], [3, 16, 96, 224, 224, 1],      # snippet-major: both views of snippet 0, then snippet 1
        [7, 0, 0, 224, 224, 0], [7, 16, 96, 224, 224, 1],
        [3, 0, 0, 224, 224, 0], [3, 16, 96, 224, 224, 1]]
    crops = torch.tensor([[1, 2, 210, 180, 1], [0, 5, 224, 224, 0]], dtype=torch.int32)
    t = rgbdiff.window_table([0, 6], crops)
    assert t.dtype == torch.int32 and t.tolist() == [[0, 1, 2, 210, 180, 1], [6, 0, 5, 224, 224, 0]]
    assert rgbdiff.RGB_DIFF_COUNT == 5
    for f in (lambda: rgbdiff.view_table([1, 2], views.long()), lambda: rgbdiff.view_table([], views),
              lambda: rgbdiff.view_table([0], views[:0]), lambda: rgbdiff.view_table(3, views),
              lambda: rgbdiff.window_table([0], crops), lambda: rgbdiff.window_table([0, 1], crops[:, :3]),
              lambda: rgbdiff.window_table(["a", 1], crops)):
        with pytest.raises(ValueError):
            f()


def test_rows_of_the_networks_size_are_the_plain_crop():
    from video_analytics_amd import augment, rgbdiff
    T, h, w, D = 9, 240, 320, 2
    frames = noise_video(T, h, w, seed=5)
    views = augment.ten_crop_views(h, w)[[1, 9]]
    starts = [0, 4, 6]
    table = rgbdiff.view_table(starts, views).numpy()
    got, ints = s23_stack(frames, table, D, want_int=True)
    for s, st in enumerate(starts):
        for v, (top, left, flip) in enumerate(views.tolist()):
            win = frames[st:st + D + 1, :, top:top + OUT, left:left + OUT].astype(np.int32)
            if flip:
                win = win[..., ::-1]
            assert np.array_equal(ints[s * 2 + v], win[1:] - win[:-1])   # row s*V + v: snippet-major


# ---- S24 restated ----

def s24_fuse(scores, weights):
    """S24 restated: (((w0*a0 + w1*a1) + w2*a2) + ...) / (((w0 + w1) + w2) + ...), every operation rounded to float32 in
    stream order; the arg-max's first maximum."""
    ws = [F32(w) for w in weights]
    acc = ws[0] * np.asarray(scores[0], F32)
    wsum = ws[0]
    for w, a in zip(ws[1:], scores[1:]):
        acc = acc + w * np.asarray(a, F32)
        wsum = F32(wsum + w)
    f = (acc / wsum).astype(np.float32)
    assert acc.dtype == F32
    return f, np.argmax(f, axis=-1).astype(np.int32)


def fuse_n_f64(scores, weights):
    """The float64 witness: exact products (float32 x float32 fits float64), math.fsum of them and of the weights."""
    a = np.stack([np.asarray(s, dtype=np.float64) for s in scores])
    w = [float(F32(x)) for x in weights]
    num = np.array([math.fsum(w[k] * a[k].flat[i] for k in range(len(w))) for i in range(a[0].size)]).reshape(a[0].shape)
    return num / math.fsum(w)


def test_s24_restatement_at_two_streams_is_s16():
    rs = np.random.RandomState(24)
    for wa, wb in ((1.0, 1.0), (1.0, 1.5), (0.0, 2.0), (3.0, 0.0), (0.3, 0.7)):
        a = rs.dirichlet(np.ones(101), size=9).astype(np.float32)
        b = rs.dirichlet(np.ones(101), size=9).astype(np.float32)
        f, p = s24_fuse([a, b], (wa, wb))
        rf, rp = s16_fuse(a, b, wa, wb)
        assert np.array_equal(f, rf) and np.array_equal(p, rp)
        assert np.abs(f - fuse_f64(a, b, float(F32(wa)), float(F32(wb)))).max() <= 4 * EPS


@pytest.mark.parametrize("m", [3, 5])
def test_s24_restatement_agrees_with_the_float64_witness(m):
    """The bound.  With u = 2^-24 and A = max |a|: the numerator's term k is rounded once as a product and once by every
    addition it passes through, m roundings at the most (terms 0 and 1: the product and m - 1 additions), so the computed
    numerator is within m*u*sum(w_k |a_k|) <= m*u*W*A of the exact one (first order), i.e. m*u*A after the division by W.
    The weights used here are small dyadic rationals whose running sums are exact in float32, so W carries no error; the
    division rounds once more, u*|f| <= u*A.  That is (m + 1)*u*A; the bound (m + 2)*u*A leaves one u*A for the
    second-order terms, which are below m^2 * u^2 * A."""
    rs = np.random.RandomState(m)
    weights = [(1.0, 1.5, 0.5), (1.0, 1.0, 1.0), (0.0, 2.0, 0.25)] if m == 3 else [(1.0, 1.5, 0.5, 2.0, 0.25), (1.0,) * 5,
                                                                                     (4.0, 0.0, 0.0, 0.5, 1.0)]
    worst = 0.0
    for ws in weights:
        run = F32(0.0)
        for w in ws:  # the premise of the bound: the running sums of the weights are exact
            assert float(F32(run + F32(w))) == float(run) + w
            run = F32(run + F32(w))
        scores = [rs.dirichlet(np.ones(101), size=7).astype(np.float32) for _ in range(m)]
        scores[1] = (scores[1] * F32(-3.0)).astype(np.float32)  # not only probabilities: both signs, A = 3 max p
        f, pred = s24_fuse(scores, ws)
        ref = fuse_n_f64(scores, ws)
        A = max(float(np.abs(s).max()) for s in scores)
        err = float(np.abs(f.astype(np.float64) - ref).max())
        worst = max(worst, err / A)
        assert err <= (m + 2) * EPS * A, (ws, err)
        top = np.sort(ref, axis=1)
        clear = (top[:, -1] - top[:, -2]) > 2 * (m + 2) * EPS * A
        assert np.array_equal(pred[clear], np.argmax(ref, axis=1)[clear])
    print("S24 m=%d: worst |restatement - witness| / max|a| = %.3g (bound %.3g)" % (m, worst, (m + 2) * EPS))


def test_s24_ties_and_nan():
    a = np.zeros((2, 7), dtype=np.float32)
    a[0, [2, 5]] = 0.5
    a[1, [6, 1]] = 0.25
    f, pred = s24_fuse([a, a, a], (1.0, 1.5, 0.5))
    assert pred.tolist() == [2, 1] and f[0, 2] == f[0, 5] == F32(0.5)
    b = a.copy()
    b[1, 3] = np.nan
    f, _ = s24_fuse([a, b, a], (1.0, 1.0, 1.0))
    assert np.isnan(f[1, 3]) and not np.isnan(f[0]).any() and np.isnan(f[1]).sum() == 1
    f, _ = s24_fuse([a, b, a], (1.0, 0.0, 1.0))   # a zero weight does not hide a NaN: 0 * NaN = NaN
    assert np.isnan(f[1, 3])


# ---- bad arguments: before anything reaches the GPU ----

def _good():
    frames = torch.zeros(8, 3, 240, 320, dtype=torch.uint8)
    table = torch.tensor([[0, 0, 0, 224, 224, 0], [2, 16, 96, 210, 180, 1]], dtype=torch.int32)
    return frames, table


def test_rgb_diff_stack_refuses_bad_arguments_on_the_host(no_gpu_calls):
    from video_analytics_amd import rgbdiff
    frames, table = _good()

    def t(r, c, v):
        x = table.clone()
        x[r, c] = v
        return x
    big = table[:1].repeat(65536, 1)
    cases = dict(
        host_frames=dict(),                                   # everything else is right: the frames are not on the device
        dtype=dict(frames_u8=frames.float()), dim=dict(frames_u8=frames[0]), channels=dict(frames_u8=frames[:, :2]),
        not_a_tensor=dict(frames_u8=frames.numpy()),
        layout=dict(layout="NCWH"), nhwc_channels=dict(layout="NHWC"),
        d_zero=dict(n_diff=0), d_large=dict(n_diff=22), d_bool=dict(n_diff=True), d_float=dict(n_diff=2.0),
        d_window=dict(n_diff=8),                              # 8 frames hold at most 7 differences
        src_last=dict(table=t(1, 0, 3)),                      # first frame 3 + 5 differences needs frame 8
        src_negative=dict(table=t(0, 0, -1)), rect=dict(table=t(1, 2, 141)), size=dict(table=t(0, 3, 0)),
        flip=dict(table=t(0, 5, 2)), table_dtype=dict(table=table.long()), table_shape=dict(table=table[:, :5]),
        table_empty=dict(table=table[:0]), too_many=dict(table=big),
        stds_zero=dict(stds=(0.229, 0.0, 0.225)), stds_nan=dict(stds=(0.229, float("nan"), 0.225)),
        stds_two=dict(stds=(0.229, 0.224)), stds_negative=dict(stds=(-1.0, 1.0, 1.0)), stds_text=dict(stds="abc"),
        out_size=dict(out=torch.zeros(2, 15, 224, 223)), out_dtype=dict(out=torch.zeros(2, 15, 224, 224, dtype=torch.float64)),
    )
    for name, kw in cases.items():
        args = dict(dict(frames_u8=frames, table=table), **kw)
        with pytest.raises(ValueError):
            rgbdiff.rgb_diff_stack(**args)
            pytest.fail(name)
    # the good call passes every rule but the last: where the frames live
    with pytest.raises(ValueError, match="CUDA"):
        rgbdiff.rgb_diff_stack(frames, table, out=torch.zeros(2, 15, 224, 224))
    with pytest.raises(ValueError, match="window of 8"):
        rgbdiff.rgb_diff_stack(frames, table, n_diff=8)
    assert rgbdiff.denominators((0.229, 0.224, 0.225)).tolist() == s23_den().tolist()


def test_check_diff_count_and_fusion_weights(no_gpu_calls):
    from video_analytics_amd import fusion, rgbdiff
    assert rgbdiff.check_diff_count(5, 10, "x") == 5 and rgbdiff.check_diff_count(1, 1, "x") == 1
    assert rgbdiff.check_diff_count(21, 30, "x") == 21 and rgbdiff.check_diff_count(np.int64(10), 10, "x") == 10
    for D, L in ((0, 10), (11, 10), (22, 30), (-1, 10), (True, 10), (2.0, 10), ("5", 10), (None, 10)):
        with pytest.raises(ValueError):
            rgbdiff.check_diff_count(D, L, "x")
    assert fusion.check_fusion_weights_n((1, 1.5, 0.5), 3, "x") == (1.0, 1.5, 0.5)
    assert fusion.check_fusion_weights_n([0, 0, 2], 3, "x") == (0.0, 0.0, 2.0)
    for w, m in (((1.0, 1.0), 3), ((1.0, 1.0, 1.0), 2), ((1.0, -0.5, 1.0), 3), ((0.0, 0.0, 0.0), 3),
                 ((1.0, float("nan"), 1.0), 3), ((1.0, float("inf"), 1.0), 3), ((1e39, 1.0), 2), ((3e38, 3e38), 2),
                 (None, 2), (1.0, 2), (("a", 1.0), 2), ((1.0,), 1), ((1.0,) * 9, 9)):
        with pytest.raises(ValueError):
            fusion.check_fusion_weights_n(w, m, "x")
    cpu = torch.zeros(2, 101)
    for f in (lambda: fusion.fuse_scores_n([cpu, cpu, cpu]), lambda: fusion.fuse_scores_n(cpu),
              lambda: fusion.fuse_scores_n([cpu]), lambda: fusion.fuse_scores_n([cpu, cpu], (1.0, 1.0, 1.0))):
        with pytest.raises(ValueError):
            f()


def test_the_constructor_refuses_bad_difference_arguments_on_the_host(no_gpu_calls, monkeypatch):
    from video_analytics_amd import pipeline
    import inspect

    def boom(*a, **k):
        raise AssertionError("reached the GPU")
    monkeypatch.setattr(pipeline, "build_stream_weights", boom)
    monkeypatch.setattr(pipeline.vgg, "Vgg16Stream", boom)
    for kw in (dict(rgb_diff_count=0), dict(rgb_diff_count=11), dict(rgb_diff_count=22, flow_count=30),
               dict(rgb_diff_count=5, flow_count=4), dict(rgb_diff_count=2.5), dict(rgb_diff_count=None)):
        with pytest.raises(ValueError, match="RGB differences"):
            pipeline.TwoStreamPipeline(device=0, rgb_diff=True, **kw)
    with pytest.raises(ValueError, match="third entry"):
        pipeline.TwoStreamPipeline(device=0, weights=[{}, {}, {}])
    with pytest.raises(ValueError, match="third entry"):
        pipeline.TwoStreamPipeline(device=0, rgb_diff=True, weights=[{}, {}, {}, {}])
    p = inspect.signature(pipeline.TwoStreamPipeline.__init__).parameters
    assert (p["rgb_diff"].default, p["rgb_diff_count"].default, p["diff_seed"].default) == (False, 5, 3)
    for f in (pipeline.TwoStreamPipeline.submit_video, pipeline.TwoStreamPipeline.run_video):
        assert inspect.signature(f).parameters["fusion_weights"].default is None


def _bare_pipeline(diff, dtype="f32"):
    """A pipeline object without a device behind it: only what the host checks read."""
    from video_analytics_amd import pipeline
    pipe = pipeline.TwoStreamPipeline.__new__(pipeline.TwoStreamPipeline)
    pipe.L, pipe.D, pipe.motion, pipe.mean_flow, pipe.camera, pipe._n = 10, 5, "stack", False, "none", 0
    pipe.device = torch.device("cpu")
    pipe.diff = types.SimpleNamespace(dtype=dtype) if diff else None
    pipe.spatial = pipe.temporal = types.SimpleNamespace(dtype=dtype, n_classes=101)
    return pipe


def test_submit_video_and_train_videos_refuse_bad_combinations_on_the_host(no_gpu_calls):
    from video_analytics_amd import augment
    rgb, gray = torch.zeros(37, 3, 240, 320, dtype=torch.uint8), torch.zeros(37, 240, 320, dtype=torch.uint8)
    v = augment.ten_crop_views(240, 320)
    third, plain = _bare_pipeline(True), _bare_pipeline(False)
    with pytest.raises(ValueError, match="fuses 3 streams"):
        third.submit_video(rgb, gray, views=(v, v), fusion_weights=(1.0, 1.5))
    with pytest.raises(ValueError, match="fuses 2 streams"):
        plain.submit_video(rgb, gray, views=(v, v), fusion_weights=(1.0, 1.5, 0.5))
    with pytest.raises(ValueError, match="fuses 2 streams"):
        plain.run_video(rgb, gray, views=(v, v), fusion_weights=(1.0,))
    for bad in ((1.0, -1.0, 1.0), (0.0, 0.0, 0.0), (1.0, float("nan"), 1.0)):
        with pytest.raises(ValueError, match="positive sum"):
            third.submit_video(rgb, gray, views=(v, v), fusion_weights=bad)
    with pytest.raises(ValueError, match="fusion weights must be 3 numbers"):
        third.submit_video(rgb, gray, views=(v, v), fusion_weights=1.5)
    # good weights (and the default None) pass the weight rules on either pipeline and stop at the next one: host tensors
    for pipe, ws in ((third, (1.0, 1.5, 0.5)), (third, None), (plain, (1.0, 1.5)), (plain, None)):
        with pytest.raises(ValueError, match="must be on"):
            pipe.submit_video(rgb, gray, views=(v, v), fusion_weights=ws)
    assert third._n == 0 and plain._n == 0
    with pytest.raises(ValueError, match="fp32 only"):
        _bare_pipeline(True, "bf16").train_videos([(rgb, gray)], [3], k=3)
