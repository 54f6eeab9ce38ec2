"""Decoded frames -> the pipeline's inputs, host side: the numpy restatement of PIL's bilinear resize and
gray level against the golden PIL made (tests/golden/make_frames_golden.py) and against PIL itself, the tap tables'
properties, the Resize rule, and every argument error of the new entry points before anything reaches a device."""
import math
import os
import types

import numpy as np
import pytest
import torch

from test_video_host import no_gpu_calls  # noqa: F401  (a fixture)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames_small.npz")
# (h, w) -> (oh, ow): the cases the golden holds
CASES = (((37, 53), (16, 23)), ((30, 40), (64, 85)), ((50, 50), (50, 31)), ((24, 32), (24, 32)), ((64, 66), (4, 5)),
         ((9, 7), (1, 1)))


def case_name(case):
    (h, w), (oh, ow) = case
    return "%dx%d_to_%dx%d" % (h, w, oh, ow)


@pytest.fixture(scope="module")
def golden():
    assert os.path.getsize(GOLDEN) < 200 * 1024
    return np.load(GOLDEN)


# ---- the restatement against PIL ----

def test_the_golden_holds_the_cases(golden):
    assert sorted(golden.files) == sorted(p + case_name(c) for c in CASES for p in ("in_", "rgb_", "gray_"))
    for case in CASES:
        (h, w), (oh, ow) = case
        nm = case_name(case)
        assert golden["in_" + nm].shape == (2, h, w, 3) and golden["in_" + nm].dtype == np.uint8
        assert golden["rgb_" + nm].shape == (2, oh, ow, 3) and golden["gray_" + nm].shape == (2, oh, ow)


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_restatement_equals_the_golden(golden, case):
    from video_analytics_amd import frames, utils
    (h, w), (oh, ow) = case
    nm = case_name(case)
    a = golden["in_" + nm]
    rgb, gray = frames.prepareFrames(a, (oh, ow))
    assert rgb.dtype == np.uint8 and gray.dtype == np.uint8
    assert np.array_equal(rgb, golden["rgb_" + nm]) and np.array_equal(gray, golden["gray_" + nm])
    assert np.array_equal(frames.resizeBilinear(a, oh, ow), rgb) and np.array_equal(utils.grayLevel(rgb), gray)
    one, g1 = frames.prepareFrames(a[1], (oh, ow))  # a single frame, no leading axis
    assert np.array_equal(one, rgb[1]) and np.array_equal(g1, gray[1])
    if (oh, ow) == (h, w):
        same, g = frames.prepareFrames(a)  # size=None keeps the size
        assert np.array_equal(same, a) and np.array_equal(g, gray)


LIVE = CASES + (((240, 320), (256, 341)), ((480, 640), (256, 341)), ((17, 300), (256, 4518)), ((240, 320), (240, 320)),
                ((64, 64), (41, 23)), ((120, 160), (240, 320)))


@pytest.mark.parametrize("case", LIVE, ids=case_name)
def test_restatement_equals_pil_live(case):
    Image = pytest.importorskip("PIL.Image")
    from video_analytics_amd import frames
    (h, w), (oh, ow) = case
    a = np.random.RandomState(h * 1000 + ow).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    a[h // 3:h // 3 + 2] = 255
    a[:, w // 2:w // 2 + 2] = 0
    im = Image.fromarray(a).resize((ow, oh), Image.BILINEAR)
    rgb, gray = frames.prepareFrames(a, (oh, ow))
    assert np.array_equal(rgb, np.asarray(im)) and np.array_equal(gray, np.asarray(im.convert("L")))


def test_gray_level_of_every_colour_is_pils():
    Image = pytest.importorskip("PIL.Image")
    from video_analytics_amd import frames
    v = np.arange(256, dtype=np.uint8)
    for r in range(256):  # the colour cube, one red plane at a time: all 2**24 colours
        a = np.stack([np.full((256, 256), r, dtype=np.uint8), np.repeat(v[:, None], 256, 1), np.repeat(v[None, :], 256, 0)], axis=-1)
        _, gray = frames.prepareFrames(a)
        assert np.array_equal(gray, np.asarray(Image.fromarray(a).convert("L")))


# ---- the tap tables ----

@pytest.mark.parametrize("n_in,n_out", [(53, 23), (37, 16), (40, 85), (30, 64), (50, 31), (66, 5), (64, 4), (7, 1), (9, 1),
                                        (320, 341), (240, 256), (640, 341), (300, 4518), (1, 5), (5, 1), (16, 1)])
def test_resample_table_properties(n_in, n_out):
    from video_analytics_amd import frames
    bounds, taps = frames.resample_table(n_in, n_out)
    ksize = 2 * int(math.ceil(max(n_in / n_out, 1.0))) + 1
    assert frames.kernel_size(n_in, n_out) == ksize <= frames.MAX_KSIZE
    assert bounds.dtype == np.int32 and taps.dtype == np.int32
    assert bounds.shape == (n_out, 2) and taps.shape == (n_out, ksize)
    lo, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (lo >= 0).all() and (n >= 1).all() and (n <= ksize).all() and (lo + n <= n_in).all()  # inside the input
    assert (taps >= 0).all()
    for i in range(n_out):
        assert (taps[i, n[i]:] == 0).all()
        assert abs(int(taps[i].sum()) - (1 << 22)) <= ksize / 2.0  # each tap is rounded once: at most half a unit each
    assert (np.diff(lo) >= 0).all()  # the windows move with the output sample
    # int32 suffices: the largest sum the device forms
    assert 255 * int(taps.sum(axis=1).max()) + (1 << 21) < 2 ** 31


def test_resample_table_known_taps():
    from video_analytics_amd import frames
    # 2 -> 1: both samples, half each; 1 -> 2: the one sample, whole; 4 -> 2: the triangle of half-width 2 cut at the edge,
    # 3/7 3/7 1/7 and its mirror
    b, t = frames.resample_table(2, 1)
    assert b.tolist() == [[0, 2]] and t[0, :2].tolist() == [1 << 21, 1 << 21]
    b, t = frames.resample_table(1, 2)
    assert b.tolist() == [[0, 1], [0, 1]] and t[:, 0].tolist() == [1 << 22, 1 << 22]
    b, t = frames.resample_table(4, 2)
    assert b.tolist() == [[0, 3], [1, 3]]
    three, one = int(0.5 + 3.0 / 7.0 * (1 << 22)), int(0.5 + 1.0 / 7.0 * (1 << 22))
    assert t[0, :3].tolist() == [three, three, one] and t[1, :3].tolist() == [one, three, three]
    for bad in ((0, 4), (4, 0), (-1, 2)):
        with pytest.raises(ValueError):
            frames.resample_table(*bad)


def test_short_side_size_known_answers():
    from video_analytics_amd import frames
    assert frames.short_side_size(240, 320, 256) == (256, 341)
    assert frames.short_side_size(320, 240, 256) == (341, 256)
    assert frames.short_side_size(256, 256, 256) == (256, 256)
    assert frames.short_side_size(480, 640, 256) == (256, 341)
    assert frames.short_side_size(240, 320, 240) == (240, 320)
    for bad in ((0, 320, 256), (240, 0, 256), (240, 320, 0)):
        with pytest.raises(ValueError):
            frames.short_side_size(*bad)
    assert frames.output_size(240, 320, None) == (240, 320)
    assert frames.output_size(240, 320, 256) == (256, 341)
    assert frames.output_size(240, 320, (100, 90)) == (100, 90)
    assert frames.output_size(64, 66, (4, 5)) == (4, 5)       # factor 16 exactly
    with pytest.raises(ValueError, match="more than 16"):
        frames.output_size(65, 66, (4, 5))                    # 16.25
    with pytest.raises(ValueError, match="more than 16"):
        frames.output_size(240, 320, 14)                      # 240 / 14 = 17.1


# ---- bad arguments: before anything reaches the GPU ----

def _rgb(T=37, H=240, W=320):
    return torch.zeros(T, 3, H, W, dtype=torch.uint8)


BAD_PREPARE = [
    ("dtype", lambda: dict(rgb=_rgb(2).float())),
    ("rank", lambda: dict(rgb=_rgb(2)[0])),
    ("not_a_tensor", lambda: dict(rgb=np.zeros((2, 3, 8, 8), dtype=np.uint8))),
    ("channels", lambda: dict(rgb=torch.zeros(2, 4, 8, 8, dtype=torch.uint8))),
    ("channels_nhwc", lambda: dict(rgb=_rgb(2), layout="NHWC")),
    ("layout", lambda: dict(rgb=_rgb(2), layout="CHW")),
    ("no_frames", lambda: dict(rgb=torch.zeros(0, 3, 8, 8, dtype=torch.uint8))),
    ("empty_frame", lambda: dict(rgb=torch.zeros(2, 3, 0, 8, dtype=torch.uint8))),
    ("size_zero", lambda: dict(rgb=_rgb(2), size=0)),
    ("size_negative", lambda: dict(rgb=_rgb(2), size=(-1, 10))),
    ("size_float", lambda: dict(rgb=_rgb(2), size=256.0)),
    ("size_bool", lambda: dict(rgb=_rgb(2), size=True)),
    ("size_triple", lambda: dict(rgb=_rgb(2), size=(1, 2, 3))),
    ("size_side_below_one", lambda: dict(rgb=torch.zeros(2, 3, 8, 200, dtype=torch.uint8), size=(8, 0))),
    ("factor_17", lambda: dict(rgb=_rgb(2), size=(14, 320))),
    ("factor_17_short_side", lambda: dict(rgb=_rgb(2), size=14)),
    ("host_tensor", lambda: dict(rgb=_rgb(2), size=256)),  # everything right but the device
]


@pytest.mark.parametrize("name,make", BAD_PREPARE, ids=[n for n, _ in BAD_PREPARE])
def test_prepare_frames_refuses_bad_arguments_on_the_host(no_gpu_calls, name, make):
    from video_analytics_amd import frames
    with pytest.raises(ValueError, match="prepare_frames"):
        frames.prepare_frames(**make())


def test_check_frames_accepts_good_calls(no_gpu_calls):
    from video_analytics_amd import frames
    assert frames.check_frames(_rgb(2), 256) == (2, 240, 320, 256, 341)
    assert frames.check_frames(torch.zeros(5, 24, 32, 3, dtype=torch.uint8), None, "NHWC") == (5, 24, 32, 24, 32)
    assert frames.check_frames(_rgb(1, 64, 66), (4, 5)) == (1, 64, 66, 4, 5)


def _bare_pipeline(diff=False):
    """A pipeline object without a device behind it: only what the host checks read."""
    from video_analytics_amd import pipeline
    pipe = pipeline.TwoStreamPipeline.__new__(pipeline.TwoStreamPipeline)
    pipe.L, pipe.D, pipe.motion, pipe.mean_flow, pipe.camera, pipe._n = 10, 5, "stack", False, "none", 0
    pipe.device = torch.device("cpu")
    pipe.heads = None
    pipe.diff = types.SimpleNamespace(dtype="f32", n_classes=101) if diff else None
    pipe.spatial = pipe.temporal = types.SimpleNamespace(dtype="f32", n_classes=101)
    return pipe


@pytest.mark.parametrize("diff", [False, True])
def test_run_video_refuses_bad_frames_on_the_host(no_gpu_calls, diff):
    from video_analytics_amd import augment
    pipe = _bare_pipeline(diff)
    rgb, gray = _rgb(), torch.zeros(37, 240, 320, dtype=torch.uint8)
    v240, v256 = augment.ten_crop_views(240, 320), augment.ten_crop_views(256, 341)
    for call in (pipe.run_video, pipe.submit_video):
        with pytest.raises(ValueError, match="rescale= derives gray"):
            call(rgb, gray, views=(v256, v256), rescale=256)
        for bad in (0, -3, 2.5, True, (1, 2, 3), "256", (256.0, 341)):
            with pytest.raises(ValueError, match="submit_video"):
                call(rgb, views=(v256, v256), rescale=bad)
        with pytest.raises(ValueError, match="more than 16"):
            call(rgb, views=(v256, v256), rescale=14)
        with pytest.raises(ValueError, match="submit_video"):
            call(rgb.float(), views=(v240, v240))                 # gray=None: rgb is all there is to check
        with pytest.raises(ValueError, match="submit_video"):
            call(rgb[0], views=(v240, v240))
        with pytest.raises(ValueError, match="submit_video"):
            call(rgb, views=(v256, v256))                         # the views are checked against the size the frames end with
        with pytest.raises(ValueError, match="need views="):
            call(rgb, rescale=256)                                # 341x256 frames need views
        with pytest.raises(ValueError, match="submit_video"):
            call(rgb[:10], views=(v240, v240))                    # 9 pairs < L
        # good frames pass every new rule and stop at the last one: the frames are on the host
        for kw in (dict(views=(v240, v240)), dict(views=(v256, v256), rescale=256), dict(views=(v256, v256), rescale=(256, 341)),
                   dict(rescale=(224, 224))):
            with pytest.raises(ValueError, match="rgb must be on"):
                call(rgb, **kw)
    assert pipe._n == 0


@pytest.mark.parametrize("diff", [False, True])
def test_train_videos_refuses_bad_frames_on_the_host(no_gpu_calls, diff):
    pipe = _bare_pipeline(diff)
    rgb, gray = _rgb(25), torch.zeros(25, 240, 320, dtype=torch.uint8)
    with pytest.raises(ValueError, match="rescale= derives gray"):
        pipe.train_videos([(rgb, gray), (rgb, gray)], [1, 2], k=3, rescale=256)
    with pytest.raises(ValueError, match="rescale= derives gray"):
        pipe.train_videos([(rgb, gray), (rgb, None)], [1, 2], k=3, rescale=256)  # one entry brings its own gray
    for bad in (0, -3, 2.5, True, (1, 2, 3), "256"):
        with pytest.raises(ValueError, match="train_videos"):
            pipe.train_videos([rgb, rgb], [1, 2], k=3, rescale=bad)
    with pytest.raises(ValueError, match="more than 16"):
        pipe.train_videos([rgb, rgb], [1, 2], k=3, rescale=14)
    with pytest.raises(ValueError, match="rgb must be a uint8"):
        pipe.train_videos([(rgb.float(), None), rgb], [1, 2], k=3)
    with pytest.raises(ValueError, match="videos must be a list"):
        pipe.train_videos([(rgb, None, None), rgb], [1, 2], k=3)
    with pytest.raises(ValueError, match="share their frame size"):
        pipe.train_videos([rgb, _rgb(25, 224, 320)], [1, 2], k=3)
    with pytest.raises(ValueError, match="share their frame size"):
        pipe.train_videos([rgb, (rgb, gray.float())], [1, 2], k=3)   # derived gray is uint8
    with pytest.raises(ValueError, match="share their frame size"):
        pipe.train_videos([rgb, _rgb(25, 320, 240)], [1, 2], k=3, rescale=256)  # 256x341 and 341x256
    with pytest.raises(ValueError, match="train_videos"):
        pipe.train_videos([rgb, rgb[:10]], [1, 2], k=3)              # a video shorter than one snippet
    # good entries in every spelling pass the new rules and stop at the last one: the frames are on the host
    for vids, kw in (([rgb, rgb], {}), ([(rgb, None), rgb], {}), ([(rgb, None), (rgb, gray)], {}), ([rgb, rgb], dict(rescale=256)),
                     ([rgb, (rgb, None)], dict(rescale=(256, 341)))):
        with pytest.raises(ValueError, match="must be on"):
            pipe.train_videos(vids, [1, 2], k=3, **kw)


def test_the_new_arguments_default_to_the_old_behaviour():
    import inspect
    from video_analytics_amd import pipeline
    for f in (pipeline.TwoStreamPipeline.submit_video, pipeline.TwoStreamPipeline.run_video):
        p = inspect.signature(f).parameters
        assert list(p)[:3] == ["self", "rgb", "gray"] and p["gray"].default is None and p["rescale"].default is None
        assert list(p)[3:11] == ["n_snippets", "views", "invert_flow_x", "consensus", "fusion_weights", "crops", "task", "rescale"]
    assert inspect.signature(pipeline.TwoStreamPipeline.train_videos).parameters["rescale"].default is None
    assert list(inspect.signature(pipeline.check_video).parameters) == ["rgb", "gray", "flow_count", "motion", "n_snippets", "views",
                                                                       "consensus", "fusion_weights", "crops"]
