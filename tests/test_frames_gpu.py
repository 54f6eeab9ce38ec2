"""Decoded frames -> the pipeline's inputs on the device: va_frames_prepare against the golden PIL made
and against the numpy restatement, bit for bit, through both layouts, byte-aligned buffers and guard bands; the ABI's
refusals; and TwoStreamPipeline.run_video / submit_video / train_videos with gray=None and rescale= against the same calls on
frames prepared on the host.  Every comparison is exact."""
import random

import numpy as np
import pytest
import torch

from test_frames_host import CASES, GOLDEN, case_name
from test_video_gpu import SCHEDULE

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 256


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _at_offset(nbytes, off, fill=FILL):
    """-> (flat, view): ``view`` the ``nbytes`` bytes that start ``off`` bytes past a 4-byte boundary of ``flat``, which is
    filled with ``fill`` and extends ``GUARD`` bytes beyond the view."""
    flat = torch.full((off + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 4 == 0
    view = flat[off:off + nbytes]
    assert view.data_ptr() % 4 == off % 4
    return flat, view


def _guards_intact(flat, off, nbytes):
    return bool((flat[:off] == FILL).all()) and bool((flat[off + nbytes:] == FILL).all()) and flat.numel() == off + nbytes + GUARD


# ---- the kernels against PIL's golden ----

@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_prepare_frames_equals_the_golden(golden, case, n):
    from video_analytics_amd import frames
    (h, w), (oh, ow) = case
    nm = case_name(case)
    pick = [0] if n == 1 else [0, 1, 1, 0, 1]  # the golden's two frames, in an order that tells the frames apart
    a = golden["in_" + nm][pick]
    want_rgb = torch.from_numpy(np.ascontiguousarray(golden["rgb_" + nm][pick].transpose(0, 3, 1, 2))).cuda()
    want_gray = torch.from_numpy(golden["gray_" + nm][pick]).cuda()
    size = None if (oh, ow) == (h, w) else (oh, ow)
    for layout in ("NCHW", "NHWC"):
        host = torch.from_numpy(a if layout == "NHWC" else np.ascontiguousarray(a.transpose(0, 3, 1, 2)))
        for off in (0, 1, 3):
            _, src = _at_offset(host.numel(), off, 0)
            src.copy_(host.reshape(-1).cuda())
            x = src.view(host.shape)
            assert x.data_ptr() % 4 == off
            rflat, rview = _at_offset(want_rgb.numel(), off)
            gflat, gview = _at_offset(want_gray.numel(), off)
            rgb, gray = frames.prepare_frames(x, size, layout, out_rgb=rview, out_gray=gview)
            torch.cuda.synchronize()
            assert rgb.data_ptr() == rview.data_ptr() and gray.data_ptr() == gview.data_ptr()
            assert tuple(rgb.shape) == (n, 3, oh, ow) and tuple(gray.shape) == (n, oh, ow)
            assert torch.equal(rgb, want_rgb), (layout, off)
            assert torch.equal(gray, want_gray), (layout, off)
            assert _guards_intact(rflat, off, want_rgb.numel()) and _guards_intact(gflat, off, want_gray.numel()), (layout, off)
        # outputs of the call's own
        x = host.cuda()
        rgb, gray = frames.prepare_frames(x, size, layout)
        assert torch.equal(rgb, want_rgb) and torch.equal(gray, want_gray), layout
        if size is None and layout == "NCHW":
            assert rgb.data_ptr() == x.data_ptr()  # planar frames that keep their size are their own result


@pytest.mark.parametrize("h,w,size,oh,ow", [(120, 160, (240, 320), 240, 320), (240, 320, 256, 256, 341)])
def test_prepare_frames_equals_the_restatement_and_repeats_its_bits(h, w, size, oh, ow):
    from video_analytics_amd import frames
    n = 3
    a = np.random.RandomState(h + ow).randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    a[1, 40:60] = 255
    a[2, :, 100:130] = 0
    want_rgb, want_gray = frames.prepareFrames(a, size)
    assert want_rgb.shape == (n, oh, ow, 3)
    want_rgb = torch.from_numpy(np.ascontiguousarray(want_rgb.transpose(0, 3, 1, 2))).cuda()
    want_gray = torch.from_numpy(want_gray).cuda()
    nchw = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2))).cuda()
    nhwc = torch.from_numpy(a).cuda()
    first = frames.prepare_frames(nchw, size)
    again = frames.prepare_frames(nchw, size)
    other = frames.prepare_frames(nhwc, size, "NHWC")
    torch.cuda.synchronize()
    for rgb, gray in (first, again, other):
        assert torch.equal(rgb, want_rgb) and torch.equal(gray, want_gray)
    assert first[0].data_ptr() != again[0].data_ptr()


def test_the_abi_refuses_bad_arguments_without_launching():
    from video_analytics_amd import _ffi, frames
    L, c = _ffi.lib(), _ffi.ctx(0)
    n, h, w, oh, ow = 2, 64, 66, 4, 5
    dev = torch.device("cuda", 0)
    src = torch.zeros(n, 3, h, w, dtype=torch.uint8, device=dev)
    xb, xt = frames.device_table(w, ow, dev)
    yb, yt = frames.device_table(h, oh, dev)
    rgb = torch.full((n, 3, oh, ow), FILL, dtype=torch.uint8, device=dev)
    gray = torch.full((n, oh, ow), FILL, dtype=torch.uint8, device=dev)
    nbytes = L.va_frames_prepare_workspace_bytes(n, w, h, ow, oh)
    assert nbytes == n * 3 * h * ow
    assert L.va_frames_prepare_workspace_bytes(n, w, h, w, oh) == 0 and L.va_frames_prepare_workspace_bytes(n, w, h, ow, h) == 0
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(src=src, n=n, w=w, h=h, nhwc=0, ow=ow, oh=oh, xb=xb, xt=xt, yb=yb, yt=yt, rgb=rgb, gray=gray, work=work, nbytes=nbytes):
        return L.va_frames_prepare(c, _ffi.ptr(src), n, w, h, nhwc, ow, oh, _ffi.ptr(xb), _ffi.ptr(xt), _ffi.ptr(yb), _ffi.ptr(yt),
                                   _ffi.ptr(rgb), _ffi.ptr(gray), _ffi.ptr(work), nbytes, _ffi.stream_ptr(dev))
    bad = (dict(h=65), dict(w=81), dict(h=1000, w=1000),      # factors 16.25, 16.2 and 250
           dict(src=None), dict(gray=None), dict(rgb=None), dict(xb=None), dict(xt=None), dict(yb=None), dict(yt=None),
           dict(n=0), dict(w=0), dict(h=0), dict(ow=0), dict(oh=0), dict(ow=-1), dict(nhwc=2))
    for kw in bad:
        assert call(**kw) == _ffi.VA_ERR_INVALID, kw
    assert call(h=65) == _ffi.VA_ERR_INVALID and b"more than 16" in L.va_last_error()
    for kw in (dict(work=None), dict(nbytes=nbytes - 1)):
        assert call(**kw) == _ffi.VA_ERR_WORKSPACE, kw
    # rgb_out may be missing only for planar frames that keep their size
    assert call(ow=w, oh=h, xb=None, xt=None, yb=None, yt=None, rgb=None, nhwc=1, gray=torch.empty(n, h, w, dtype=torch.uint8, device=dev)) \
        == _ffi.VA_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((rgb == FILL).all()) and bool((gray == FILL).all())  # nothing was launched
    assert call() == _ffi.VA_OK
    torch.cuda.synchronize()
    want_rgb, want_gray = frames.prepareFrames(np.zeros((n, h, w, 3), dtype=np.uint8), (oh, ow))
    assert not bool(rgb.any()) and not bool(gray.any()) and not want_rgb.any() and not want_gray.any()
    with pytest.raises(ValueError):
        frames.prepare_frames(src, (3, 5))  # the wrapper refuses the same factor itself


# ---- the pipeline ----

def _decoded_video(T, H, W, seed):
    """RGB u8 [T,3,H,W] as a decoder hands it over: one moving texture seen through three channels that differ."""
    from video_analytics_amd import synth
    _, gray, _ = synth.synth_clips(1, seed=seed, H=H, W=W, n_gray=T)
    g = gray[0]
    return torch.stack([g, torch.roll(g, 5, dims=2), 255 - torch.roll(g, 3, dims=1)], dim=1).contiguous()


def _host_gray(rgb):
    """utils.grayLevel of rgb u8 [T,3,H,W] on the host -> u8 [T,H,W]."""
    from video_analytics_amd import utils
    return torch.from_numpy(utils.grayLevel(rgb.permute(0, 2, 3, 1).numpy()))


def _host_prepared(rgb, size):
    """frames.prepareFrames of rgb u8 [T,3,H,W] on the host -> (rgb u8 [T,3,oh,ow], gray u8 [T,oh,ow])."""
    from video_analytics_amd import frames
    r, g = frames.prepareFrames(np.ascontiguousarray(rgb.permute(0, 2, 3, 1).numpy()), size)
    return torch.from_numpy(np.ascontiguousarray(r.transpose(0, 3, 1, 2))), torch.from_numpy(g)


KEYS = ("scores_s", "scores_t", "scores", "pred", "desc_s", "desc_t", "logits_s_items", "logits_t_items")


def _kept(out):
    return {key: out[key].clone() for key in KEYS}


def _assert_same(a, b):
    for key in KEYS:
        assert torch.equal(a[key], b[key]), key


@pytest.fixture(scope="module")
def pipe():
    from video_analytics_amd import _ffi, pipeline
    p = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(**SCHEDULE))
    yield p
    p.close()


def test_run_video_derives_gray_and_pipelines_it(pipe):
    from video_analytics_amd import augment
    H, W = 240, 320
    rgb, rgb2 = _decoded_video(20, H, W, seed=71), _decoded_video(23, H, W, seed=73)
    views = augment.ten_crop_views(H, W)
    kw = dict(views=(views, views))
    with pytest.raises(ValueError):
        pipe.run_video(rgb.cuda(), _host_gray(rgb).cuda(), rescale=256, **kw)
    n0 = pipe._n
    given = pipe.run_video(rgb.cuda(), _host_gray(rgb).cuda(), **kw)
    given = _kept(given)
    out = pipe.run_video(rgb.cuda(), **kw)
    assert out["frame_size"] == (H, W) and tuple(out["logits_s_items"].shape) == (25, 10, 101) and pipe._n == n0 + 2
    one = _kept(out)
    _assert_same(one, given)
    assert float(one["logits_t_items"].std()) > 0 and torch.isfinite(one["scores"]).all()
    two = _kept(pipe.run_video(rgb2.cuda(), **kw))
    assert not torch.equal(two["scores_t"], one["scores_t"])
    # pipelined: both videos submitted before either is waited for (different lengths: the buffers are re-allocated)
    a = pipe.submit_video(rgb.cuda(), **kw)
    b = pipe.submit_video(rgb2.cuda(), **kw)
    pipe.wait()
    torch.cuda.synchronize()
    _assert_same(a, one)
    _assert_same(b, two)


def test_run_video_rescales_on_the_device(pipe):
    from video_analytics_amd import augment
    from video_analytics_amd.video import evaluateVideos
    rgb = _decoded_video(20, 120, 160, seed=75)
    views = augment.ten_crop_views(240, 320)
    kw = dict(views=(views, views))
    big, gray = _host_prepared(rgb, 240)
    assert tuple(big.shape) == (20, 3, 240, 320) and tuple(gray.shape) == (20, 240, 320)
    want = _kept(pipe.run_video(big.cuda(), gray.cuda(), **kw))
    out = pipe.run_video(rgb.cuda(), rescale=240, **kw)
    assert out["frame_size"] == (240, 320)
    _assert_same(_kept(out), want)
    _assert_same(_kept(pipe.run_video(rgb.cuda(), rescale=(240, 320), **kw)), want)
    # evaluateVideos passes both through: bare frames and rescale=
    label = int(want["pred"])
    acc_s, acc_t, acc_f, desc = evaluateVideos(pipe, [rgb.cuda(), (rgb.cuda(), None)], [label, label + 1], rescale=240, **kw)
    assert acc_f == 0.5 and desc.shape == (2, 512)
    assert np.array_equal(desc[0], torch.cat([want["desc_s"], want["desc_t"]]).cpu().numpy()) and np.array_equal(desc[0], desc[1])


def test_train_videos_derives_gray():
    from video_analytics_amd import _ffi, augment, pipeline
    k, lr, mu, seed = 3, 1e-4, 0.9, 5
    vids = [_decoded_video(25, 120, 160, seed=81), _decoded_video(31, 120, 160, seed=83)]
    starts = [[0, 3, 14], [2, 9, 20]]
    crops = augment.draw_scale_jitter_crops(6, 240, 320, random.Random(3))
    labels = torch.tensor([5, 77])
    params = _ffi.default_tvl1_params(**SCHEDULE)
    args = dict(k=k, starts=starts, crops=crops, lr=lr, momentum=mu, dropout_seed=seed)
    outs, first = [], []
    for derive in (True, False):
        p = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
        if derive:  # one entry in each spelling
            out = p.train_videos([(vids[0].cuda(), None), vids[1].cuda()], labels, rescale=240, **args)
        else:
            out = p.train_videos([tuple(t.cuda() for t in _host_prepared(v, 240)) for v in vids], labels, **args)
        torch.cuda.synchronize()
        outs.append(out)
        first.append([m.export_state()["conv_w"][0].cpu() for m in (p.spatial, p.temporal)])
        p.close()
    a, b = outs
    assert tuple(a["flow"].shape[-2:]) == (240, 320) and torch.equal(a["flow"], b["flow"])
    for key in ("stats_s", "stats_t", "desc_s", "desc_t"):
        assert torch.isfinite(a[key]).all() and torch.equal(a[key], b[key]), key
    for x, y in zip(*first):
        assert torch.equal(x, y)
