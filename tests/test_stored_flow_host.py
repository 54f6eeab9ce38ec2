"""Stored optical flow, host side: numpy float32 restatements of the quantisation, the u8 snippets
gather and the u8 crop-resize gather, each held to an independent witness (utils.flowToImages, an index-by-index gather, a
float64 bilinear with the rounding decided away from ties); every ValueError of the flow= / flows= arguments, raised with all
paths to the device blocked; and utils.loadFlowImages against PIL on files utils.saveFlowImages wrote.
tests/test_stored_flow_gpu.py holds the kernels and the pipeline to these restatements bit for bit."""
import os

import numpy as np
import pytest
import torch

from test_tsn_host import s17_cases, s17_resize, s9_quantise, value_tolerance, witness
from test_video_host import no_gpu_calls, s15_source_planes  # noqa: F401  (no_gpu_calls: a fixture)

F32 = np.float32
MEAN, STD = F32(0.485), F32(0.229)


# ---- S39-S41 restated ----

def s39_quantise(flow, bound=20.0):
    """S39 in its written order on float32 values -> uint8; fmax / fmin return the other operand for a NaN, as fmaxf does."""
    bound = F32(bound)
    with np.errstate(invalid="ignore"):
        t = (F32(255.0) * (np.asarray(flow, F32) + bound)) / (F32(2.0) * bound)
        return np.rint(np.fmin(np.fmax(t, F32(0.0)), F32(255.0))).astype(np.uint8)


def s40_normalise(q, invert=False):
    """The tail of S40 / S41: q (integers 0..255 in any type) -> ((float)q' / 255 - mean) / std in float32."""
    q = np.asarray(q).astype(F32)
    if invert:
        q = F32(255.0) - q
    return (q / F32(255.0) - MEAN) / STD


def s40_snippets(flowq, starts, views, L, invert_x=False, size=224):
    """flowq uint8 [N,2,h,w], starts [n], views int [V,3] -> float32 [n*V*2L,size,size]: va_flowq_to_stack_snippets."""
    N, _, h, w = flowq.shape
    planes = flowq.reshape(2 * N, h, w)
    views = np.asarray(views)
    V = views.shape[0]
    src = s15_source_planes(starts, L, V)
    out = np.empty((len(src), size, size), dtype=F32)
    for o, p in enumerate(src.tolist()):
        top, left, flip = views[(o // (2 * L)) % V].tolist()
        win = planes[p, top:top + size, left:left + size]
        out[o] = s40_normalise(win[:, ::-1] if flip else win, bool(invert_x) and bool(flip) and p % 2 == 0)
    return out


def s41_images(flowq, table):
    """The resampled 8-bit image of every table row: uint8 [n_out,224,224], what va_resize_images_u8 writes for the plane."""
    planes = flowq.reshape((-1,) + flowq.shape[2:])
    out = np.empty((len(table), 224, 224), dtype=np.uint8)
    for o, row in enumerate(np.asarray(table).tolist()):
        val = s17_resize(planes[row[0]].astype(F32), row)
        out[o] = np.rint(np.minimum(np.maximum(val, F32(0.0)), F32(255.0))).astype(np.uint8)
    return out


def s41_resize(flowq, table, invert_x=False, images=None):
    """flowq uint8 [N,2,h,w], table int [n_out,6] -> float32 [n_out,224,224]: va_flowq_to_stack_resize.  ``images``: the
    resampled images when they come from elsewhere (the device's resize_images)."""
    qr = s41_images(flowq, table) if images is None else images
    out = np.empty(qr.shape, dtype=F32)
    for o, row in enumerate(np.asarray(table).tolist()):
        out[o] = s40_normalise(qr[o], bool(invert_x) and bool(row[5]) and row[0] % 2 == 0)
    return out


def hard_flow(rs, n, h, w):
    """sigma 12 px (both clamps at +-20 are hit) with planted NaN and +-inf."""
    fl = (rs.standard_normal((n, 2, h, w)) * 12.0).astype(F32)
    fl[0, 0, 3, 5], fl[1, 1, h - 1, w - 1], fl[2 % n, 0, 0, 0] = np.nan, np.inf, -np.inf
    fl[0, 1, h // 2, 4:8] = np.nan
    return fl


# ---- the restatements against their witnesses ----

@pytest.mark.parametrize("bound", [20.0, 127.5, 7.25])
def test_s39_restatement_equals_flow_to_images(bound):
    from video_analytics_amd import utils
    rs = np.random.RandomState(39)
    fl = (rs.standard_normal((3, 2, 33, 47)) * 12.0).astype(F32)
    fl[0, 0, :4, :4] = [[-1e9, -20.0, 20.0, 1e9]] * 4   # far beyond +-bound, and the bound itself
    if bound == 127.5:  # integer values: t = v + 127.5, every one an exact tie; rint rounds it to even
        fl = np.rint(fl)
        q = s39_quantise(fl, bound)
        inside = np.abs(fl) < 127
        assert (q[inside] % 2 == 0).all() and np.array_equal(q[inside], (2 * np.rint((fl[inside] + 127.5) / 2)).astype(np.uint8))
    q = s39_quantise(fl, bound)
    assert q.dtype == np.uint8 and np.array_equal(q, utils.flowToImages(fl, bound))
    assert q.min() == 0 and q.max() == 255
    # what numpy's clip does not specify: a NaN becomes 0, the infinities the ends
    assert s39_quantise(np.array([np.nan, np.inf, -np.inf], F32)).tolist() == [0, 255, 0]


def test_s39_then_normalise_is_s9():
    """Storing q and normalising later gives S9's bits: the stored path's whole claim, on the host."""
    rs = np.random.RandomState(9)
    fl = hard_flow(rs, 3, 20, 31)
    ok = np.isfinite(fl)
    for inv in (False, True):
        with np.errstate(invalid="ignore"):
            assert np.array_equal(s40_normalise(s39_quantise(fl), inv)[ok], s9_quantise(fl, invert=inv)[ok])


@pytest.mark.parametrize("invert", [False, True])
def test_s40_restatement_equals_an_index_by_index_gather(invert):
    rs = np.random.RandomState(40)
    N, h, w, L, size = 6, 9, 11, 2, 4
    q = rs.randint(0, 256, size=(N, 2, h, w)).astype(np.uint8)
    starts = [0, 1, 1, 4]
    views = np.array([[0, 0, 0], [5, 7, 1], [2, 3, 1]])
    got = s40_snippets(q, starts, views, L, invert, size).reshape(len(starts), len(views), 2 * L, size, size)
    for s, st in enumerate(starts):
        for v, (top, left, flip) in enumerate(views.tolist()):
            for c in range(2 * L):
                for y in range(size):
                    for x in range(size):
                        val = int(q[st + c // 2, c % 2, top + y, left + (size - 1 - x if flip else x)])
                        if invert and flip and c % 2 == 0:
                            val = 255 - val
                        want = F32(F32(F32(val) / F32(255.0)) - MEAN) / STD
                        assert got[s, v, c, y, x] == want, (s, v, c, y, x)


@pytest.mark.parametrize("h,w", [(240, 320), (241, 321)])
def test_s41_restatement_rounds_as_the_float64_witness_away_from_ties(h, w):
    """Where the float64 bilinear value is farther from a tie (k + 1/2) than the value tolerance, the restatement's resampled
    image must be rint of the witness, and its output the normalisation of that; elsewhere either neighbour may come out."""
    rs = np.random.RandomState(h)
    q = rs.randint(0, 256, size=(1, 2, h, w)).astype(np.uint8)
    for (top, left, ch, cw) in s17_cases(h, w):
        for flip in (0, 1):
            for src in (0, 1):
                row = (src, top, left, ch, cw, flip)
                ref = witness(q[0, src], row)
                tol = value_tolerance(q[0, src, top:top + ch, left:left + cw], ch, cw, bool(flip))
                near = np.abs(ref - np.floor(ref) - 0.5) <= tol
                want = np.rint(np.clip(ref, 0.0, 255.0)).astype(np.int64)
                img = s41_images(q, [row])[0].astype(np.int64)
                assert np.array_equal(img[~near], want[~near]) and int(np.abs(img - want).max()) <= 1, row
                assert near.mean() <= 0.02, (row, float(near.mean()))
                for inv in (False, True):
                    got = s41_resize(q, [row], inv)[0]
                    flipped_x = inv and flip and src == 0
                    w64 = ((255 - want if flipped_x else want) / 255.0 - 0.485) / 0.229
                    # float32 against float64: q / 255 in [0, 1] rounds by <= 2^-25, the constant 0.485 by <= 2^-26, the
                    # difference (magnitude <= 0.515) by <= 2^-25: 1.25 * 2^-24 in all, 5.5 * 2^-24 after the division by 0.229;
                    # the constant 0.229 and the division add 2^-24 each relative to a quotient below 2.25: 10 * 2^-24
                    assert float(np.abs(got.astype(np.float64) - w64)[~near].max()) <= 10 * 2.0 ** -24, row


def test_s41_at_224_is_the_s40_crop():
    rs = np.random.RandomState(41)
    h, w, L = 240, 320, 2
    q = rs.randint(0, 256, size=(3, 2, h, w)).astype(np.uint8)
    views = np.array([[0, 0, 0], [16, 96, 1], [7, 5, 1]])
    for inv in (False, True):
        a = s40_snippets(q, [1], views, L, inv)
        table = [[2 * 1 + c, int(t), int(l), 224, 224, int(f)] for (t, l, f) in views.tolist() for c in range(2 * L)]
        assert np.array_equal(s41_resize(q, table, inv), a)


def test_s41_is_not_the_float_resize_away_from_224():
    """TSN's order (resample the image) against the live path's (resample the field, quantise once): equal at 224, different
    in a visible share of the pixels for a resampling crop.  DESIGN.md S41 records this; nothing treats them as equal."""
    from test_tsn_host import s17_flow_stack
    rs = np.random.RandomState(4)
    fl = (rs.standard_normal((1, 2, 240, 320)) * 12.0).astype(F32)
    q = s39_quantise(fl)
    same = [[0, 3, 5, 224, 224, 1]]
    assert np.array_equal(s41_resize(q, same, True), s17_flow_stack(fl, same, True))
    other = [[0, 0, 0, 168, 210, 0]]
    assert (s41_resize(q, other) != s17_flow_stack(fl, other)).mean() > 0.01


# ---- bad arguments: before anything reaches the GPU ----
#
# The frames and stores live on the host and the pipeline object has no device behind it, so a call that passes every shape
# and type rule stops at the last rule, "must be on <device>"; a bad store must be refused by its own rule before that.

def _video(T=37, H=240, W=320):
    return torch.zeros(T, 3, H, W, dtype=torch.uint8)


def _pipe(motion="stack", mean_flow=False, camera="none"):
    """A TwoStreamPipeline without a device behind it: only what the host checks read."""
    import types
    from video_analytics_amd import pipeline
    p = pipeline.TwoStreamPipeline.__new__(pipeline.TwoStreamPipeline)
    p.L, p.D, p.motion, p.mean_flow, p.camera, p._n = 10, 0, motion, mean_flow, camera, 0
    p.device = torch.device("cuda", 0)
    p.heads, p.diff = None, None
    p.spatial = p.temporal = types.SimpleNamespace(dtype="f32", n_classes=101)
    p.flow_streams, p.tvl1_params = 2, None
    return p


def _store(T=37, H=240, W=320, dtype=torch.uint8):
    return torch.zeros(T - 1, 2, H, W, dtype=dtype)


VIDEO_CASES = [("with_gray", "replaces the gray frames"), ("dtype", "uint8 or float32"), ("rank", "uint8 or float32"),
               ("planes", "uint8 or float32"), ("not_a_tensor", "uint8 or float32"), ("count", "stored flow fields"),
               ("size", "but the frames are"), ("size_after_rescale", "but the frames are"), ("strided", "contiguous"),
               ("u8_mean_flow", "act on the float field"), ("f32_bidirectional", "not offered for whole videos"),
               ("u8_trajectory", "not offered for whole videos")]


@pytest.mark.parametrize("case,msg", VIDEO_CASES, ids=[c for c, _ in VIDEO_CASES])
def test_submit_video_refuses_bad_stored_flow_on_the_host(no_gpu_calls, case, msg):
    from video_analytics_amd import augment
    rgb, gray, flow, kw, pk = _video(), None, _store(), {}, {}
    if case == "with_gray":
        gray = torch.zeros(37, 240, 320, dtype=torch.uint8)
    elif case == "dtype":
        flow = _store(dtype=torch.float16)
    elif case == "rank":
        flow = flow[0]
    elif case == "planes":
        flow = torch.zeros(36, 3, 240, 320, dtype=torch.uint8)
    elif case == "not_a_tensor":
        flow = flow.numpy()
    elif case == "count":
        flow = _store(T=36)
    elif case == "size":
        flow = _store(H=224, W=224)
    elif case == "size_after_rescale":
        kw["rescale"] = (256, 341)  # the store has the decoded size, the prepared frames do not
    elif case == "strided":
        flow = _store(W=640)[:, :, :, ::2]
    elif case == "u8_mean_flow":
        pk["mean_flow"] = True
    elif case == "f32_bidirectional":
        flow, pk["motion"] = _store(dtype=torch.float32), "bidirectional"
    elif case == "u8_trajectory":
        pk["motion"] = "trajectory"
    pipe = _pipe(**pk)
    h, w = kw.get("rescale", (240, 320))
    v = augment.ten_crop_views(h, w)
    for call in (pipe.submit_video, pipe.run_video):
        with pytest.raises(ValueError, match=msg):
            call(rgb, gray, views=(v, v), flow=flow, **kw)
    assert pipe._n == 0


def test_submit_video_passes_good_stored_flow_to_the_last_rule(no_gpu_calls):
    from video_analytics_amd import augment
    v = augment.ten_crop_views(240, 320)
    for dtype, pk in ((torch.uint8, {}), (torch.float32, {}), (torch.float32, dict(mean_flow=True)),
                      (torch.uint8, dict(camera="homography"))):
        with pytest.raises(ValueError, match="must be on"):
            _pipe(**pk).submit_video(_video(), None, views=(v, v), flow=_store(dtype=dtype))
    v = augment.ten_crop_views(256, 341)
    with pytest.raises(ValueError, match="must be on"):
        _pipe().submit_video(_video(), None, views=(v, v), flow=_store(H=256, W=341), rescale=(256, 341))


TRAIN_CASES = [("with_gray", "replaces the gray frames"), ("count", "2 videos but 1 stored flows"), ("not_a_list", "must be a list"),
               ("mixed_types", "share their type"), ("dtype", "uint8 or float32"), ("fields", "stored flow fields"),
               ("size", "but the frames are"), ("strided", "contiguous"), ("u8_mean_flow", "act on the float field"),
               ("u8_trajectory", "act on the float field"), ("f32_bidirectional", "bi-directional")]


@pytest.mark.parametrize("case,msg", TRAIN_CASES, ids=[c for c, _ in TRAIN_CASES])
def test_train_videos_refuses_bad_stored_flows_on_the_host(no_gpu_calls, case, msg):
    import random
    videos = [_video(37), _video(41)]
    flows, pk = [_store(37), _store(41)], {}
    if case == "with_gray":
        videos[1] = (videos[1], torch.zeros(41, 240, 320, dtype=torch.uint8))
    elif case == "count":
        flows = flows[:1]
    elif case == "not_a_list":
        flows = 5
    elif case == "mixed_types":
        flows[1] = _store(41, dtype=torch.float32)
    elif case == "dtype":
        flows = [_store(37, dtype=torch.float64), _store(41, dtype=torch.float64)]
    elif case == "fields":
        flows[1] = _store(37)
    elif case == "size":
        flows[0] = _store(37, H=224, W=224)
    elif case == "strided":
        flows[0] = _store(37, W=640)[:, :, :, ::2]
    elif case == "u8_mean_flow":
        pk["mean_flow"] = True
    elif case == "u8_trajectory":
        pk["motion"] = "trajectory"
    elif case == "f32_bidirectional":
        flows, pk["motion"] = [_store(37, dtype=torch.float32), _store(41, dtype=torch.float32)], "bidirectional"
    with pytest.raises(ValueError, match=msg):
        _pipe(**pk).train_videos(videos, [3, 4], k=3, rng=random.Random(1), flows=flows)


def test_train_videos_passes_good_stored_flows_to_the_last_rule(no_gpu_calls):
    import random
    for dtype, pk in ((torch.uint8, {}), (torch.uint8, dict(camera="homography")), (torch.float32, dict(mean_flow=True)),
                      (torch.float32, dict(motion="trajectory", mean_flow=True))):
        with pytest.raises(ValueError, match="and the stored flows must be on"):
            _pipe(**pk).train_videos([_video(37), (_video(41), None)], [3, 4], k=3, rng=random.Random(1),
                                     flows=[_store(37, dtype=dtype), _store(41, dtype=dtype)])


@pytest.mark.parametrize("case", ["bidirectional", "dtype", "rank", "gray_dtype", "gray_rescale", "one_frame", "device"])
def test_extract_flow_refuses_bad_arguments_on_the_host(no_gpu_calls, case):
    frames, kw, pk = torch.zeros(12, 240, 320, dtype=torch.uint8), {}, {}
    if case == "bidirectional":
        pk["motion"] = "bidirectional"
    elif case == "dtype":
        kw["dtype"] = torch.float16
    elif case == "rank":
        frames = frames[0]
    elif case == "gray_dtype":
        frames = frames.double()
    elif case == "gray_rescale":
        kw["rescale"] = 256
    elif case == "one_frame":
        frames = frames[:1]
    msg = dict(bidirectional="bi-directional", dtype="dtype must be", rank="frames must be gray", gray_dtype="uint8 or float32",
               gray_rescale="acts on rgb frames", one_frame="no frame pair", device="must be on")[case]
    with pytest.raises(ValueError, match=msg):
        _pipe(**pk).extract_flow(frames, **kw)
    if case == "device":  # good rgb frames, with and without rescale=, reach the last rule too
        for kw in ({}, dict(rescale=256), dict(dtype=torch.float32, return_camera=True)):
            with pytest.raises(ValueError, match="must be on"):
                _pipe().extract_flow(_video(12), **kw)


def test_flow_wrappers_refuse_bad_arguments_on_the_host(no_gpu_calls):
    from video_analytics_amd import augment
    from video_analytics_amd import flow as vflow
    v = augment.ten_crop_views(240, 320)
    f32, u8 = torch.zeros(12, 2, 240, 320), torch.zeros(12, 2, 240, 320, dtype=torch.uint8)
    table = torch.tensor([[0, 0, 0, 224, 224, 0]], dtype=torch.int32)
    vflow.check_stored_flow(u8, 13, 240, 320, "x")
    vflow.check_stored_flow(f32, 13, 240, 320, "x")
    for f in (lambda: vflow.quantize_flow(f32), lambda: vflow.quantize_flow(u8),              # host tensors
              lambda: vflow.flowq_to_stack_snippets(u8, [0], v, 10), lambda: vflow.resize_flowq_to_stack(u8, table),
              # the existing wrappers keep rejecting u8 flow
              lambda: vflow.crop_flow_to_stack_snippets(u8, [0], v, 10), lambda: vflow.resize_flow_to_stack(u8, table),
              lambda: vflow.check_stored_flow(u8, 14, 240, 320, "x"), lambda: vflow.check_stored_flow(u8, 13, 240, 322, "x")):
        with pytest.raises(ValueError):
            f()


def test_evaluate_videos_needs_one_stored_flow_per_video():
    from video_analytics_amd import video

    class Pipe(object):
        diff = None

        def __init__(self):
            self.seen = []

        def submit_video(self, rgb, gray, flow=None, **kw):
            self.seen.append((rgb, gray, flow))
            z = torch.zeros(3)

            class Done(object):
                def synchronize(self):
                    pass
            return dict(scores_s=z, scores_t=z, pred=torch.tensor(0), desc_s=z, desc_t=z, done=Done())

        def wait(self):
            pass
    p = Pipe()
    video.evaluateVideos(p, ["a", ("b", None)], [0, 0], flows=iter(["fa", "fb"]))
    assert p.seen == [("a", None, "fa"), ("b", None, "fb")]
    for flows in (["fa"], ["fa", "fb", "fc"]):
        with pytest.raises(ValueError):
            video.evaluateVideos(Pipe(), ["a", "b"], [0, 0], flows=flows)
    p = Pipe()
    video.evaluateVideos(p, ["a"], [0])  # flows=None: submit_video is called as before, without flow=
    assert p.seen == [("a", None, None)]


# ---- loadFlowImages ----

def test_load_flow_images_reads_what_save_flow_images_wrote(tmp_path):
    from PIL import Image
    from video_analytics_amd import utils
    rs = np.random.RandomState(5)
    fl = (rs.standard_normal((4, 2, 24, 32)) * 8.0).astype(F32)
    d = str(tmp_path / "v_flow")
    assert utils.saveFlowImages(fl, d) == 8
    got = utils.loadFlowImages(d)
    assert got.dtype == np.uint8 and got.shape == (4, 2, 24, 32)
    for k in range(4):
        for plane, prefix in enumerate(("flow_x_", "flow_y_")):
            ref = np.asarray(Image.open(os.path.join(d, "%s%04d.jpg" % (prefix, k + 1))))
            assert np.array_equal(got[k, plane], ref)
    assert np.abs(got.astype(int) - utils.flowToImages(fl).astype(int)).max() <= 24  # JPEG of noise, quality 95: close
    assert np.array_equal(utils.loadFlowImages(d, first=2, count=2), got[1:3])
    assert np.array_equal(utils.loadFlowImages(d, first=3), got[2:])
    # a missing file: asked for by count, in the middle of a pair, at the start
    with pytest.raises(ValueError):
        utils.loadFlowImages(d, count=5)
    with pytest.raises(ValueError):
        utils.loadFlowImages(d, first=6)
    with pytest.raises(ValueError):
        utils.loadFlowImages(d, count=0)
    os.remove(os.path.join(d, "flow_y_0003.jpg"))
    with pytest.raises(ValueError):
        utils.loadFlowImages(d)
    assert utils.loadFlowImages(d, count=2).shape == (2, 2, 24, 32)
    # a size mismatch and a colour image
    Image.fromarray(np.zeros((24, 30), np.uint8), mode="L").save(os.path.join(d, "flow_y_0003.jpg"))
    with pytest.raises(ValueError):
        utils.loadFlowImages(d)
    Image.fromarray(np.zeros((24, 32, 3), np.uint8), mode="RGB").save(os.path.join(d, "flow_y_0003.jpg"))
    with pytest.raises(ValueError):
        utils.loadFlowImages(d)
