"""Stored optical flow on the device: va_flow_quantize_u8, va_flowq_to_stack_snippets and
va_flowq_to_stack_resize against the float gathers and the restatements of tests/test_stored_flow_host.py, bit for bit;
TwoStreamPipeline.extract_flow against TV-L1 pair by pair; and run_video(flow=), train_videos(flows=) and
evaluateVideos(flows=) against the live calls they replace, with TV-L1 patched to raise while the stored calls run."""
import random

import numpy as np
import pytest
import torch

from test_stored_flow_host import hard_flow, s40_snippets, s41_resize
from test_tsn_gpu import _full_table, _state, _videos
from test_video_gpu import SCHEDULE, _synthetic_video

pytestmark = pytest.mark.gpu

RESULT_TENSORS = ("scores_s", "scores_t", "scores", "pred", "desc_s", "desc_t", "logits_s_items", "logits_t_items")


def _no_tvl1(monkeypatch):
    """From here on a TV-L1 launch through the flow module raises."""
    from video_analytics_amd import flow as vflow

    def boom(*a, **k):
        raise AssertionError("a stored-flow call launched TV-L1")
    monkeypatch.setattr(vflow, "tvl1_flow", boom)
    monkeypatch.setattr(vflow, "tvl1_flow_concurrent", boom)


def _offset(t, by=1):
    """A copy of ``t`` that starts ``by`` elements past an aligned allocation."""
    flat = torch.empty(t.numel() + by, dtype=t.dtype, device=t.device)
    flat[by:].copy_(t.reshape(-1))
    return flat[by:].view(t.shape)


# ---- S39: the quantisation ----

@pytest.mark.parametrize("w,h", [(320, 240), (321, 241), (17, 300)])
def test_quantize_equals_flow_to_images(w, h):
    from video_analytics_amd import utils
    from video_analytics_amd import flow as vflow
    rs = np.random.RandomState(w)
    fl = (rs.standard_normal((3, 2, h, w)) * 12.0).astype(np.float32)   # sigma 12 px: values beyond +-20 on both sides
    fl[0, 0, 0, :4] = [-1e9, -20.0, 20.0, 1e9]
    assert (fl > 20).any() and (fl < -20).any()
    d = torch.from_numpy(fl).cuda()
    ref = utils.flowToImages(fl)
    got = vflow.quantize_flow(d)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 2, h, w) and got.data_ptr() % 4 == 0 and d.data_ptr() % 16 == 0
    assert np.array_equal(got.cpu().numpy(), ref)
    # a source and a destination one element past the aligned ones: scalar loads, byte stores
    src = _offset(d)
    assert src.data_ptr() % 16 == 4
    assert np.array_equal(vflow.quantize_flow(src).cpu().numpy(), ref)
    dst = torch.full((fl.size + 1,), 7, dtype=torch.uint8, device="cuda")
    out = vflow.quantize_flow(d, out=dst[1:])
    assert out.data_ptr() % 4 == 1 and np.array_equal(out.cpu().numpy(), ref) and int(dst[0]) == 7
    out = vflow.quantize_flow(src, out=dst[1:].zero_())
    assert np.array_equal(out.cpu().numpy(), ref) and int(dst[0]) == 7
    # bound = 127.5 and integer flow: t = v + 127.5, every value an exact tie
    ints = np.rint(fl * 4.0).astype(np.float32)
    ints[0, 0, 0, :4] = [-1e9, -128.0, 127.0, 1e9]
    got = vflow.quantize_flow(torch.from_numpy(ints).cuda(), bound=127.5).cpu().numpy()
    assert np.array_equal(got, utils.flowToImages(ints, 127.5)) and (got[np.abs(ints) < 127] % 2 == 0).all()


def test_quantize_refuses_bad_arguments():
    from video_analytics_amd import _ffi
    from video_analytics_amd import flow as vflow
    fl = torch.zeros(2, 2, 8, 12, device="cuda")
    for bad in (lambda: vflow.quantize_flow(fl, bound=0.0), lambda: vflow.quantize_flow(fl, bound=float("nan")),
                lambda: vflow.quantize_flow(fl, bound="x"), lambda: vflow.quantize_flow(fl[:, :1]),
                lambda: vflow.quantize_flow(fl.to(torch.uint8)), lambda: vflow.quantize_flow(fl, out=torch.zeros(5, device="cuda")),
                lambda: vflow.quantize_flow(fl, out=torch.zeros(2, 2, 8, 12, device="cuda"))):
        with pytest.raises(ValueError):
            bad()
    L, c = _ffi.lib(), _ffi.ctx(0)
    out = torch.zeros(2, 2, 8, 12, dtype=torch.uint8, device="cuda")

    def call(flow=fl, n=2, w=12, h=8, bound=20.0, dst=out):
        return L.va_flow_quantize_u8(c, _ffi.ptr(flow), n, w, h, bound, _ffi.ptr(dst), _ffi.stream_ptr(fl.device))
    assert call() == _ffi.VA_OK
    for kw in (dict(flow=None), dict(dst=None), dict(n=0), dict(w=0), dict(h=-1), dict(bound=0.0), dict(bound=-1.0)):
        assert call(**kw) == _ffi.VA_ERR_INVALID, kw
    torch.cuda.synchronize()


# ---- S40: the snippets gather ----

@pytest.mark.parametrize("h,w", [(240, 320), (241, 321)])
@pytest.mark.parametrize("invert", [False, True])
def test_flowq_snippets_gather_equals_the_float_gather(h, w, invert):
    from video_analytics_amd import augment
    from video_analytics_amd import flow as vflow
    L, N = 10, 14
    fl = hard_flow(np.random.RandomState(h + int(invert)), N, h, w)   # sigma 12 px, planted NaN and +-inf
    views = augment.ten_crop_views(h, w)
    starts = [0, 1, 1, 4, 4]  # overlapping windows, duplicates, the last possible start
    d = torch.from_numpy(fl).cuda()
    q = vflow.quantize_flow(d)
    live = vflow.crop_flow_to_stack_snippets(d, starts, views, L, invert_x_on_flip=invert)
    got = vflow.flowq_to_stack_snippets(q, starts, views, L, invert_x_on_flip=invert)
    assert tuple(got.shape) == (len(starts), 10, 2 * L, 224, 224) and got.dtype == torch.float32
    assert torch.equal(got, live)
    # a numpy gather of the u8 store
    ref = s40_snippets(q.cpu().numpy(), starts, views.numpy(), L, invert)
    assert np.array_equal(got.cpu().numpy().reshape(-1, 224, 224), ref)
    # an unaligned volume (4 bytes past a 16-byte boundary), prefilled with NaN: every element is written, by scalar stores
    flat = torch.full((got.numel() + 1,), float("nan"), dtype=torch.float32, device="cuda")
    assert flat[1:].data_ptr() % 16 == 4
    un = vflow.flowq_to_stack_snippets(q, starts, views, L, invert_x_on_flip=invert, out=flat[1:])
    assert torch.equal(un, live) and bool(torch.isnan(flat[0]))
    # an aligned volume prefilled with NaN, and a store one byte past a 4-byte boundary: byte loads
    pre = torch.full(tuple(got.shape), float("nan"), dtype=torch.float32, device="cuda")
    q1 = _offset(q)
    assert q1.data_ptr() % 4 == 1
    assert torch.equal(vflow.flowq_to_stack_snippets(q1, starts, views, L, invert_x_on_flip=invert, out=pre), live)
    # disjoint windows: the views form of the float gather
    a = vflow.flowq_to_stack_snippets(q[:10], [0], views, L, invert_x_on_flip=invert)
    assert torch.equal(a, vflow.crop_flow_to_stack_views(d[:10], views, L, invert_x_on_flip=invert))


def test_flowq_gathers_refuse_bad_arguments():
    from video_analytics_amd import _ffi, augment
    from video_analytics_amd import flow as vflow
    q = torch.zeros(12, 2, 240, 320, dtype=torch.uint8, device="cuda")
    views = augment.ten_crop_views(240, 320)
    table = torch.tensor([[0, 0, 0, 224, 224, 0]], dtype=torch.int32)
    for bad in (lambda: vflow.flowq_to_stack_snippets(q, [3], views, 10), lambda: vflow.flowq_to_stack_snippets(q, [], views, 10),
                lambda: vflow.flowq_to_stack_snippets(q, [0], views, 13), lambda: vflow.flowq_to_stack_snippets(q.float(), [0], views, 10),
                lambda: vflow.flowq_to_stack_snippets(q, [0], augment.ten_crop_views(480, 640), 10),
                lambda: vflow.resize_flowq_to_stack(q.float(), table), lambda: vflow.resize_flowq_to_stack(q, table[:, :5]),
                lambda: vflow.resize_flowq_to_stack(q, torch.tensor([[24, 0, 0, 224, 224, 0]], dtype=torch.int32)),
                lambda: vflow.resize_flowq_to_stack(q, torch.tensor([[0, 20, 0, 224, 224, 0]], dtype=torch.int32)),
                # the existing wrappers keep rejecting u8 flow
                lambda: vflow.crop_flow_to_stack_snippets(q, [0], views, 10), lambda: vflow.resize_flow_to_stack(q, table),
                lambda: vflow.flow_to_stack(q)):
        with pytest.raises(ValueError):
            bad()
    L, c = _ffi.lib(), _ffi.ctx(0)
    out = torch.zeros(1, 10, 20, 224, 224, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    cr = augment.crops_to_device(augment.expand_views(views, 1, 20), q.device)
    tb = augment.crops_to_device(table, q.device)

    def snip(flow=q, n_pairs=12, starts=st, n=1, flow_count=10, V=10, inv=0, std=0.229, crops=cr, dst=out):
        return L.va_flowq_to_stack_snippets(c, _ffi.ptr(flow), n_pairs, _ffi.ptr(starts), n, flow_count, V, 320, 240, 0.485, std,
                                            _ffi.ptr(crops), inv, 224, 224, _ffi.ptr(dst), _ffi.stream_ptr(q.device))
    assert snip() == _ffi.VA_OK
    for kw in (dict(flow=None), dict(n_pairs=9), dict(starts=None), dict(n=0), dict(flow_count=0), dict(V=0), dict(inv=2),
               dict(n=4000), dict(std=0.0), dict(crops=None), dict(dst=None)):
        assert snip(**kw) == _ffi.VA_ERR_INVALID, kw

    def res(flow=q, n_pairs=12, w=320, std=0.229, tab=tb, n_out=1, inv=0, dst=out):
        return L.va_flowq_to_stack_resize(c, _ffi.ptr(flow), n_pairs, w, 240, 0.485, std, _ffi.ptr(tab), n_out, inv, _ffi.ptr(dst),
                                          _ffi.stream_ptr(q.device))
    assert res() == _ffi.VA_OK
    for kw in (dict(flow=None), dict(n_pairs=0), dict(w=0), dict(std=0.0), dict(tab=None), dict(n_out=0), dict(n_out=70000),
               dict(inv=2), dict(dst=None)):
        assert res(**kw) == _ffi.VA_ERR_INVALID, kw
    torch.cuda.synchronize()


# ---- S41: the crop-resize gather ----

def _resize_rows(h, w, n_planes, seed):
    """Table rows {src, top, left, ch, cw, flip}: crops of 224 x 224, the full frame, 168 x 168, 168 x 210 and 1 x 1, each
    at all four corners, plain and flipped, the source plane alternating between x and y planes."""
    rs = np.random.RandomState(seed)
    rows = []
    for ch, cw in ((224, 224), (h, w), (168, 168), (168, 210), (1, 1)):
        for top in (0, h - ch):
            for left in (0, w - cw):
                for flip in (0, 1):
                    rows.append([int(rs.randint(0, n_planes)), top, left, ch, cw, flip])
    return rows


@pytest.mark.parametrize("h,w", [(240, 320), (256, 341)])
@pytest.mark.parametrize("invert", [False, True])
def test_flowq_resize_gather_is_the_image_resize_then_the_normalisation(h, w, invert):
    from video_analytics_amd import augment
    from video_analytics_amd import flow as vflow
    N = 3
    fl = hard_flow(np.random.RandomState(w + int(invert)), N, h, w)
    q = vflow.quantize_flow(torch.from_numpy(fl).cuda())
    rows = _resize_rows(h, w, 2 * N, seed=h)
    assert any(r[0] % 2 == 0 and r[5] for r in rows) and any(r[0] % 2 == 1 and r[5] for r in rows)
    table = torch.tensor(rows, dtype=torch.int32)
    got = vflow.resize_flowq_to_stack(q, table, invert_x_on_flip=invert)
    assert tuple(got.shape) == (len(rows), 224, 224) and got.dtype == torch.float32
    # the planes as one-channel images through the image gather, then inversion and normalisation restated in float32
    images = augment.resize_images(q.view(2 * N, 1, h, w), table)[:, 0].cpu().numpy()
    assert np.array_equal(got.cpu().numpy(), s41_resize(q.cpu().numpy(), rows, invert, images=images))
    # ... and the whole restatement on the host
    assert np.array_equal(got.cpu().numpy(), s41_resize(q.cpu().numpy(), rows, invert))
    # an unaligned, NaN-prefilled volume
    flat = torch.full((got.numel() + 1,), float("nan"), dtype=torch.float32, device="cuda")
    assert torch.equal(vflow.resize_flowq_to_stack(q, table, invert_x_on_flip=invert, out=flat[1:]), got)


@pytest.mark.parametrize("invert", [False, True])
def test_flowq_resize_gather_at_224_is_the_snippets_gather(invert):
    from video_analytics_amd import augment
    from video_analytics_amd import flow as vflow
    h, w, L, N = 241, 321, 2, 6
    fl = hard_flow(np.random.RandomState(224), N, h, w)
    q = vflow.quantize_flow(torch.from_numpy(fl).cuda())
    views = augment.ten_crop_views(h, w)
    starts = [0, 3, 3, 4]
    a = vflow.flowq_to_stack_snippets(q, starts, views, L, invert_x_on_flip=invert)
    rows = [[2 * s + c, t, l, 224, 224, f] for s in starts for (t, l, f) in views.tolist() for c in range(2 * L)]
    b = vflow.resize_flowq_to_stack(q, torch.tensor(rows, dtype=torch.int32), invert_x_on_flip=invert)
    assert torch.equal(a.view(-1, 224, 224), b)


# ---- extract_flow ----

@pytest.fixture(scope="module")
def params():
    from video_analytics_amd import _ffi
    return _ffi.default_tvl1_params(**SCHEDULE)


@pytest.fixture(scope="module")
def pipe(params):
    from video_analytics_amd import pipeline
    p = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    yield p
    p.close()


@pytest.fixture(scope="module")
def video37(params):
    """A 37-frame 320x240 video on the device and the TV-L1 field of each of its 36 pairs, computed pair by pair."""
    from video_analytics_amd import flow as vflow
    rgb, gray = _synthetic_video(37, 240, 320, seed=41)
    rgb, gray = rgb.cuda(), gray.cuda()
    pairs = torch.stack([gray[:-1], gray[1:]], dim=1)     # [36,2,H,W]: every field from its own two-frame sequence
    fields = vflow.tvl1_flow(pairs, params)
    torch.cuda.synchronize()
    return rgb, gray, fields


@pytest.mark.parametrize("streams", [2, 3])
def test_extract_flow_is_tvl1_of_every_pair(params, video37, streams):
    from video_analytics_amd import pipeline, utils
    rgb, gray, fields = video37
    p = pipeline.TwoStreamPipeline(device=0, tvl1_params=params, flow_streams=streams)
    f32 = p.extract_flow(gray, dtype=torch.float32)
    assert f32.dtype == torch.float32 and tuple(f32.shape) == (36, 2, 240, 320) and f32.is_contiguous()
    assert torch.equal(f32, fields)
    u8 = p.extract_flow(gray)
    assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), utils.flowToImages(f32))
    store, Hm, share = p.extract_flow(gray.float(), dtype=torch.float32, return_camera=True)   # float gray frames: the same flow
    assert torch.equal(store, fields) and Hm is None and share is None
    if streams == 2:  # decoded RGB frames: the gray frames and rescale= as submit_video derives them
        from video_analytics_amd import flow as vflow
        from video_analytics_amd import frames as vframes
        g = vframes.prepare_frames(rgb[:5], (120, 160))[1]
        assert torch.equal(p.extract_flow(rgb[:5], rescale=(120, 160), dtype=torch.float32),
                           vflow.tvl1_flow(torch.stack([g[:-1], g[1:]], dim=1), params))
        for bad in (dict(frames=gray.cpu()), dict(frames=gray[:1]), dict(frames=gray, rescale=120), dict(frames=gray, dtype=torch.float16)):
            with pytest.raises(ValueError):
                p.extract_flow(**bad)
    p.close()


def test_extract_flow_stores_the_warped_flow_of_a_camera_pipeline(params, video37):
    from video_analytics_amd import pipeline, utils
    from video_analytics_amd import flow as vflow
    rgb, gray, fields = video37
    p = pipeline.TwoStreamPipeline(device=0, tvl1_params=params, camera="homography")
    want, Hw, sw = vflow.apply_camera(fields, "homography")
    store, Hm, share = p.extract_flow(gray, dtype=torch.float32, return_camera=True)
    assert torch.equal(store, want) and not torch.equal(store, fields)
    assert torch.equal(Hm, Hw) and torch.equal(share, sw) and tuple(Hm.shape) == (36, 3, 3)
    assert np.array_equal(p.extract_flow(gray).cpu().numpy(), utils.flowToImages(want))
    p.close()
    bi = pipeline.TwoStreamPipeline(device=0, tvl1_params=params, motion="bidirectional")
    with pytest.raises(ValueError):
        bi.extract_flow(gray)
    bi.close()


# ---- run_video(flow=) ----

def _assert_same_result(a, b):
    for key in RESULT_TENSORS:
        assert torch.equal(a[key], b[key]), key
    assert a["starts"] == b["starts"] and a["frame_size"] == b["frame_size"] and a["plan"].pairs == b["plan"].pairs
    assert sorted(a) == sorted(b)


def test_run_video_from_stored_flow_equals_the_live_call(pipe, video37, monkeypatch):
    from video_analytics_amd import augment
    rgb, gray, fields = video37
    views = augment.ten_crop_views(240, 320)
    kw = dict(views=(views, views), invert_flow_x=True, fusion_weights=(1.0, 1.5))
    live = pipe.run_video(rgb, gray, **kw)
    live = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in live.items()}
    f32, u8 = pipe.extract_flow(gray, dtype=torch.float32), pipe.extract_flow(gray)
    with pytest.raises(ValueError):
        pipe.submit_video(rgb, gray, flow=u8, **kw)            # flow= with gray=
    with pytest.raises(ValueError):
        pipe.submit_video(rgb, flow=u8.cpu(), **kw)            # a store on the host
    with pytest.raises(ValueError):
        pipe.submit_video(rgb, flow=u8[:-1], **kw)             # a field short
    n = pipe._n
    _no_tvl1(monkeypatch)
    for store in (f32, u8):
        out = pipe.run_video(rgb, flow=store, **kw)
        torch.cuda.synchronize()
        _assert_same_result(out, live)
        assert "homography" not in out and tuple(out["logits_t_items"].shape) == (25, 10, 101)
    assert pipe._n == n + 2


def test_run_video_from_stored_flow_with_mean_flow(params, video37, monkeypatch):
    from video_analytics_amd import augment, pipeline
    rgb, gray, fields = video37
    p = pipeline.TwoStreamPipeline(device=0, tvl1_params=params, mean_flow=True)
    views = augment.ten_crop_views(240, 320)
    kw = dict(n_snippets=5, views=(views, views))
    live = p.run_video(rgb, gray, **kw)
    live = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in live.items()}
    with pytest.raises(ValueError):
        p.submit_video(rgb, flow=p.extract_flow(gray), **kw)   # a uint8 store: the means act on the float field
    _no_tvl1(monkeypatch)
    out = p.run_video(rgb, flow=fields, **kw)
    torch.cuda.synchronize()
    _assert_same_result(out, live)
    p.close()


def test_pipelined_pair_from_stored_flow_equals_two_live_calls(pipe, video37, monkeypatch):
    from video_analytics_amd import augment
    rgb, gray, fields = video37
    rgb2, gray2 = (t.cuda() for t in _synthetic_video(20, 240, 320, seed=43))
    views = augment.ten_crop_views(240, 320)
    kw = dict(n_snippets=4, views=(views[4:5], views[3:6]), consensus="logits")
    one = {k: v.clone() for k, v in pipe.run_video(rgb, gray, **kw).items() if isinstance(v, torch.Tensor)}
    two = {k: v.clone() for k, v in pipe.run_video(rgb2, gray2, **kw).items() if isinstance(v, torch.Tensor)}
    s1, s2 = pipe.extract_flow(gray), pipe.extract_flow(gray2, dtype=torch.float32)
    _no_tvl1(monkeypatch)
    a = pipe.submit_video(rgb, flow=s1, **kw)    # both submitted before either is waited for; a uint8 and a float32 store
    b = pipe.submit_video(rgb2, flow=s2, **kw)
    pipe.wait()
    torch.cuda.synchronize()
    for key in RESULT_TENSORS:
        assert torch.equal(a[key], one[key]), key
        assert torch.equal(b[key], two[key]), key


# ---- train_videos(flows=) and evaluateVideos(flows=) ----

@pytest.fixture
def training_workspaces_released():
    """The training workspaces this module's pipelines allocate leave the cache again: tests that run later find the training
    workspace of their own model as the only one (tests/test_train_gpu.py reads it back)."""
    yield
    from video_analytics_amd import vgg
    torch.cuda.synchronize()
    for key in [key for key in vgg._ws_cache if "train" in str(key)]:
        del vgg._ws_cache[key]


def test_train_videos_from_stored_flows(params, monkeypatch, training_workspaces_released):
    """Three steps on two pipelines built from the same seeds, which therefore stay in one state as long as the steps agree:
    float32 stores with drawn scale-jitter crops and uint8 stores with 224 x 224 crops against the live step; then uint8 stores
    with drawn crops against the temporal model's own step on a volume built from the restatement of S41."""
    from video_analytics_amd import augment, pipeline
    from video_analytics_amd import flow as vflow
    from video_analytics_amd.video import segmentPlan
    L, k, lr, mu = 10, 3, 1e-4, 0.9
    vids, starts = _videos()
    dev = [(r.cuda(), g.cuda()) for r, g in vids]
    labels = torch.tensor([5, 77])
    live, stored = pipeline.TwoStreamPipeline(device=0, tvl1_params=params), pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    f32 = [stored.extract_flow(g, dtype=torch.float32) for _, g in dev]
    u8 = [stored.extract_flow(g) for _, g in dev]
    plans = [segmentPlan(g.shape[0], st, L) for (_, g), st in zip(dev, starts)]
    rgbs = [r for r, _ in dev]

    def same(a, b, names=("stats_s", "stats_t", "desc_s", "desc_t")):
        torch.cuda.synchronize()
        for name in names:
            assert torch.isfinite(a[name]).all() and torch.equal(a[name], b[name]), name
        assert a["starts"] == b["starts"] and torch.equal(a["crops"], b["crops"])
        for m, o in ((live.spatial, stored.spatial), (live.temporal, stored.temporal)):
            assert all(torch.equal(x, y) for x, y in zip(_state(m), _state(o)))

    # float32 stores, drawn scale-jitter crops
    crops = augment.draw_scale_jitter_crops(6, 240, 320, random.Random(3))
    assert any(tuple(c[2:4]) != (224, 224) for c in crops.tolist())
    a = live.train_videos(dev, labels, k=k, starts=starts, crops=crops, lr=lr, momentum=mu, dropout_seed=5, invert_flow_x=True)
    with monkeypatch.context() as mp:
        _no_tvl1(mp)
        b = stored.train_videos(rgbs, labels, k=k, starts=starts, crops=crops, lr=lr, momentum=mu, dropout_seed=5,
                                invert_flow_x=True, flows=f32)
    same(a, b)
    assert b["flow"].dtype == torch.float32 and torch.equal(a["flow"], b["flow"])
    assert torch.equal(b["flow"], torch.cat([f[p.pairs] for f, p in zip(f32, plans)])) and "homography" not in b
    # uint8 stores, crops of the network's own size
    crops224 = crops.clone()
    crops224[:, 2:4] = 224
    crops224[:, 0].clamp_(max=240 - 224)
    crops224[:, 1].clamp_(max=320 - 224)
    a = live.train_videos(dev, labels, k=k, starts=starts, crops=crops224, lr=lr, momentum=mu, dropout_seed=6, invert_flow_x=True)
    with monkeypatch.context() as mp:
        _no_tvl1(mp)
        b = stored.train_videos([(r, None) for r in rgbs], labels, k=k, starts=starts, crops=crops224, lr=lr, momentum=mu,
                                dropout_seed=6, invert_flow_x=True, flows=u8)
    same(a, b)
    assert b["flow"].dtype == torch.uint8 and torch.equal(b["flow"], torch.cat([f[p.pairs] for f, p in zip(u8, plans)]))
    # uint8 stores, drawn crops: TSN's order, the restatement of S41 on the full stores with a table written out by hand
    first, base = [], 0
    for f, st in zip(u8, starts):
        first += [base + s for s in st]
        base += f.shape[0]
    xt = s41_resize(torch.cat(u8).cpu().numpy(), _full_table(crops, first, L), True).reshape(6, 2 * L, 224, 224)
    stats, desc = live.temporal.train_step_consensus(torch.from_numpy(xt).cuda(), labels, k, lr, mu, 7)
    with monkeypatch.context() as mp:
        _no_tvl1(mp)
        b = stored.train_videos(rgbs, labels, k=k, starts=starts, crops=crops, lr=lr, momentum=mu, dropout_seed=7,
                                invert_flow_x=True, flows=u8)
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and torch.equal(b["stats_t"], stats) and torch.equal(b["desc_t"], desc)
    assert all(torch.equal(x, y) for x, y in zip(_state(live.temporal), _state(stored.temporal)))
    # the argument rules, on the device: nothing is enqueued
    for bad in (dict(videos=dev, flows=u8), dict(videos=rgbs, flows=u8[:1]), dict(videos=rgbs, flows=[u8[0], f32[1]]),
                dict(videos=rgbs, flows=[u8[0].cpu(), u8[1]]), dict(videos=rgbs, flows=[u8[1], u8[0]])):
        with pytest.raises(ValueError):
            stored.train_videos(labels=labels, k=k, starts=starts, crops=crops, **bad)
    live.close()
    stored.close()


def test_train_videos_from_float_stores_follows_trajectories(params, monkeypatch, training_workspaces_released):
    """motion="trajectory" with mean_flow: float32 stores allow it, and the step keeps the live step's bits."""
    from video_analytics_amd import augment, pipeline
    vids, starts = _videos()
    dev = [(r.cuda(), g.cuda()) for r, g in vids]
    labels = torch.tensor([9, 3])
    kw = dict(device=0, tvl1_params=params, motion="trajectory", mean_flow=True)
    live, stored = pipeline.TwoStreamPipeline(**kw), pipeline.TwoStreamPipeline(**kw)
    f32 = [stored.extract_flow(g, dtype=torch.float32) for _, g in dev]
    u8 = [stored.extract_flow(g) for _, g in dev]
    crops = augment.draw_scale_jitter_crops(6, 240, 320, random.Random(4))
    step = dict(k=3, starts=starts, crops=crops, lr=1e-4, momentum=0.9, dropout_seed=8)
    a = live.train_videos(dev, labels, **step)
    _no_tvl1(monkeypatch)
    b = stored.train_videos([r for r, _ in dev], labels, flows=f32, **step)
    torch.cuda.synchronize()
    for name in ("stats_s", "stats_t", "desc_s", "desc_t"):
        assert torch.equal(a[name], b[name]), name
    assert all(torch.equal(x, y) for x, y in zip(_state(live.temporal), _state(stored.temporal)))
    with pytest.raises(ValueError):
        stored.train_videos([r for r, _ in dev], labels, flows=u8, **step)  # the chains follow the float field
    live.close()
    stored.close()


def test_evaluate_videos_from_stored_flows_equals_the_live_call(monkeypatch):
    from video_analytics_amd import _ffi, pipeline
    from video_analytics_amd.video import evaluateVideos
    p = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(epsilon=0.0, nscales=3, warps=1, iters=10))
    vids = [_synthetic_video(T, 224, 224, seed=50 + T) for T in (12, 15, 11)]
    dev = [(r.cuda(), g.cuda()) for r, g in vids]
    labels = [int(p.run_video(r, g, n_snippets=3)["pred"]) for r, g in dev]
    labels[1] = (labels[1] + 1) % 101
    live = evaluateVideos(p, dev, labels, n_snippets=3)
    assert live[2] == pytest.approx(2.0 / 3.0)
    stores = [[p.extract_flow(g, dtype=dt) for _, g in dev] for dt in (torch.uint8, torch.float32)]
    _no_tvl1(monkeypatch)
    for flows in stores:
        got = evaluateVideos(p, [r for r, _ in dev], labels, flows=iter(flows), n_snippets=3)
        assert got[:3] == live[:3] and np.array_equal(got[3], live[3])
    with pytest.raises(ValueError):
        evaluateVideos(p, [r for r, _ in dev], labels, flows=stores[0][:2], n_snippets=3)
    p.close()
