"""RGB difference on the device: va_rgbdiff_to_stack against the numpy restatement of
tests/test_rgbdiff_host.py and against differences of va_resize_images_u8 outputs, bit for bit; va_fuse_scores_n against the
S24 restatement; and the third stream of TwoStreamPipeline.run_video / train_videos / evaluateVideos against inputs built
independently, the torch-CPU VGG oracle and a plain two-stream pipeline."""
import numpy as np
import pytest
import torch

from test_rgbdiff_host import jitter_rows, moving_video, noise_video, s23_den, s23_stack, s24_fuse
from test_video_gpu import SCHEDULE, _item_mean, _synthetic_video
from test_video_host import s16_fuse

pytestmark = pytest.mark.gpu


# ---- S23: the gather ----

@pytest.mark.parametrize("D", [1, 5, 7])
@pytest.mark.parametrize("h,w", [(240, 320), (241, 321), (37, 29)])
def test_gather_equals_the_restatement_and_differences_of_resized_images(h, w, D):
    from video_analytics_amd import augment, rgbdiff
    T = 8
    table = jitter_rows(h, w, T - D)
    assert len(set(table[:, 0].tolist())) == T - D and len(table) > T - D  # every first frame, repeated: overlapping windows
    ttable = torch.from_numpy(table)
    n_out = len(table)
    den = torch.from_numpy(s23_den()).cuda().view(1, 1, 3, 1, 1)
    for kind, video in (("noise", noise_video(T, h, w, seed=h + D)), ("moving", moving_video(T, h, w, seed=w + D))):
        ref, ints = s23_stack(video, table, D, want_int=True)
        assert ints.min() < 0 < ints.max() and (kind == "noise" or (ints == 0).any())
        for layout in ("NCHW", "NHWC"):
            x = torch.from_numpy(video if layout == "NCHW" else np.ascontiguousarray(video.transpose(0, 2, 3, 1))).cuda()
            got = rgbdiff.rgb_diff_stack(x, ttable, D, layout=layout)
            assert tuple(got.shape) == (n_out, 3 * D, 224, 224) and got.dtype == torch.float32
            assert np.array_equal(got.cpu().numpy(), ref), (kind, layout)
            # a NaN-prefilled buffer: every element is written
            buf = torch.full((n_out, 3 * D, 224, 224), float("nan"), device="cuda")
            assert buf.data_ptr() % 16 == 0
            assert rgbdiff.rgb_diff_stack(x, ttable, D, layout=layout, out=buf).data_ptr() == buf.data_ptr()
            assert torch.equal(buf, got)
            # an unaligned volume (4 bytes past a 16-byte boundary): the scalar store path, and nothing outside it
            flat = torch.full((got.numel() + 2,), float("nan"), device="cuda")
            assert flat[1:-1].data_ptr() % 16 == 4
            un = rgbdiff.rgb_diff_stack(x, ttable, D, layout=layout, out=flat[1:-1])
            assert torch.equal(un, got) and bool(torch.isnan(flat[0])) and bool(torch.isnan(flat[-1]))
            # the second device path: va_resize_images_u8 of the D + 1 frames of every row, subtracted and divided by torch
            rows = ttable.repeat_interleave(D + 1, dim=0)
            rows[:, 0] += torch.arange(D + 1, dtype=torch.int32).repeat(n_out)
            r = augment.resize_images(x, rows, layout=layout).view(n_out, D + 1, 3, 224, 224).to(torch.int32)
            two = ((r[:, 1:] - r[:, :-1]).to(torch.float32) / den).view(n_out, 3 * D, 224, 224)
            assert torch.equal(two, got), (kind, layout)


def test_gather_refuses_bad_arguments():
    from video_analytics_amd import _ffi, rgbdiff
    import ctypes
    frames = torch.zeros(8, 3, 240, 320, dtype=torch.uint8, device="cuda")
    table = torch.tensor([[0, 0, 0, 224, 224, 0]], dtype=torch.int32)
    for kw in (dict(n_diff=8), dict(n_diff=0), dict(layout="NHWC"), dict(stds=(1.0, 0.0, 1.0)),
               dict(out=torch.zeros(15, 224, 224)), dict(table=torch.tensor([[3, 0, 0, 224, 224, 0]], dtype=torch.int32))):
        with pytest.raises(ValueError):
            rgbdiff.rgb_diff_stack(**dict(dict(frames_u8=frames, table=table), **kw))
    L, c = _ffi.lib(), _ffi.ctx(0)
    out = torch.zeros(1, 15, 224, 224, device="cuda")
    dt = table.cuda()
    good = (ctypes.c_float * 3)(58.0, 57.0, 57.5)

    def call(fr=frames, n=8, w=320, h=240, nhwc=0, D=5, den=good, tab=dt, n_out=1, dst=out):
        return L.va_rgbdiff_to_stack(c, _ffi.ptr(fr), n, w, h, nhwc, D, den, _ffi.ptr(tab), n_out, _ffi.ptr(dst),
                                     _ffi.stream_ptr(frames.device))
    assert call() == _ffi.VA_OK
    far = torch.tensor([[7, 0, 0, 224, 224, 0]], dtype=torch.int32).cuda()
    assert call(tab=far) == _ffi.VA_OK  # first frame 7 is clamped to 2 on the device: nothing is read out of bounds
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out))
    for kw in (dict(fr=None), dict(tab=None), dict(dst=None), dict(den=None), dict(n=5), dict(D=0), dict(D=22), dict(nhwc=2),
               dict(w=0), dict(n_out=0), dict(n_out=65536), dict(den=(ctypes.c_float * 3)(58.0, 0.0, 57.5)),
               dict(den=(ctypes.c_float * 3)(58.0, float("nan"), 57.5)), dict(den=(ctypes.c_float * 3)(58.0, float("inf"), 1.0))):
        assert call(**kw) == _ffi.VA_ERR_INVALID, kw
    torch.cuda.synchronize()


# ---- S24: fusion of m streams ----

@pytest.mark.parametrize("weights", [(1.0, 1.0), (1.0, 1.5), (0.0, 2.0), (0.25, 7.0)])
def test_fuse_scores_n_with_two_streams_is_fuse_scores(weights):
    from video_analytics_amd import fusion
    rs = np.random.RandomState(int(weights[1] * 8))
    a = torch.from_numpy(rs.dirichlet(np.ones(101), size=33).astype(np.float32)).cuda()
    b = torch.from_numpy(rs.dirichlet(np.ones(101), size=33).astype(np.float32)).cuda()
    f2, p2 = fusion.fuse_scores(a, b, weights)
    fn, pn = fusion.fuse_scores_n([a, b], weights)
    assert torch.equal(f2, fn) and torch.equal(p2, pn) and pn.dtype == torch.int32
    rf, rp = s16_fuse(a.cpu().numpy(), b.cpu().numpy(), *weights)
    assert np.array_equal(fn.cpu().numpy(), rf) and np.array_equal(pn.cpu().numpy(), rp)
    f1, p1 = fusion.fuse_scores_n([a, b])  # the default: all ones
    f0, p0 = fusion.fuse_scores(a, b)
    assert torch.equal(f1, f0) and torch.equal(p1, p0)


@pytest.mark.parametrize("m,weights", [(3, (1.0, 1.5, 0.5)), (3, (1.0, 1.0, 1.0)), (3, (0.3, 0.0, 0.7)),
                                       (5, (1.0, 1.5, 0.5, 2.0, 0.25)), (8, (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8))])
def test_fuse_scores_n_equals_the_restatement(m, weights):
    from video_analytics_amd import fusion
    rs = np.random.RandomState(m)
    scores = [rs.dirichlet(np.ones(300), size=5).astype(np.float32) for _ in range(m)]  # 300 classes: more than one pass of 256
    scores[1] = (scores[1] * np.float32(-3.0)).astype(np.float32)
    for s in scores:
        s[2, :] = 0.0
        s[2, [17, 260]] = 0.5                # an exact tie: the first maximum wins
    got, pred = fusion.fuse_scores_n([torch.from_numpy(s).cuda() for s in scores], weights)
    rf, rp = s24_fuse(scores, weights)
    assert np.array_equal(got.cpu().numpy(), rf) and np.array_equal(pred.cpu().numpy(), rp)
    f = got.cpu().numpy()
    assert f[2, 17] == f[2, 260] > 0 and int(pred[2]) == 17


def test_fuse_scores_n_ties_nan_and_bad_arguments():
    from video_analytics_amd import _ffi, fusion
    import ctypes
    a = np.zeros((2, 7), dtype=np.float32)
    a[0, [2, 5]] = 0.5
    b = a.copy()
    b[1, 3] = np.nan
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    f, pred = fusion.fuse_scores_n([da, da, da], (1.0, 1.5, 0.5))
    assert int(pred[0]) == 2 and float(f[0, 2]) == float(f[0, 5]) == 0.5
    f, _ = fusion.fuse_scores_n([da, db, da], (1.0, 0.0, 1.0))
    rf, _ = s24_fuse([a, b, a], (1.0, 0.0, 1.0))
    assert np.array_equal(f.cpu().numpy(), rf, equal_nan=True) and np.isnan(f.cpu().numpy()).sum() == 1
    for bad in ((-1.0, 2.0, 1.0), (0.0, 0.0, 0.0), (1.0, 1.0), (float("nan"), 1.0, 1.0)):
        with pytest.raises(ValueError):
            fusion.fuse_scores_n([da, da, da], bad)
    for bad in ([da], [da] * 9, [da, da.double()], [da, da[:1]], [da, da.cpu()]):
        with pytest.raises(ValueError):
            fusion.fuse_scores_n(bad)
    L, c = _ffi.lib(), _ffi.ctx(0)
    out, p = torch.zeros(2, 7, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")

    def call(m=3, ws=(1.0, 1.0, 1.0), ptrs=None, n=2, cc=7):
        ptrs = [da.data_ptr()] * len(ws) if ptrs is None else ptrs
        return L.va_fuse_scores_n(c, (ctypes.c_void_p * len(ptrs))(*ptrs), (ctypes.c_float * len(ws))(*ws), m, n, cc, _ffi.ptr(out),
                                  _ffi.ptr(p), None)
    assert call() == _ffi.VA_OK
    for kw in (dict(m=1, ws=(1.0,)), dict(m=9, ws=(1.0,) * 9), dict(ws=(1.0, -1.0, 1.0)), dict(ws=(0.0, 0.0, 0.0)),
               dict(ws=(1.0, float("nan"), 1.0)), dict(ws=(1.0, float("inf"), 1.0)), dict(ws=(3e38, 3e38, 1.0)),
               dict(ptrs=[da.data_ptr(), None, da.data_ptr()]), dict(n=0), dict(cc=0)):
        assert call(**kw) == _ffi.VA_ERR_INVALID, kw
    torch.cuda.synchronize()


# ---- S25: the third stream ----

def _diff_weights(c_in, seed=3):
    from oracle import vgg_oracle
    from video_analytics_amd import synth
    w = synth.synth_vgg16_weights(c_in=c_in, seed=seed)
    w["conv_w"][0] = vgg_oracle.copy_first_layer(w["conv_w"][0], c_in)
    return w


def test_run_video_with_the_difference_stream():
    from oracle import vgg_oracle
    from video_analytics_amd import _ffi, augment, pipeline, rgbdiff
    from video_analytics_amd.video import snippetStarts
    H, W, D = 240, 320, 5
    rgb, gray = _synthetic_video(20, H, W, seed=43)
    rgb2, gray2 = _synthetic_video(37, H, W, seed=45)
    params = _ffi.default_tvl1_params(**SCHEDULE)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params, rgb_diff=True)
    plain = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    assert pipe.diff.c_in == 3 * D and pipe.D == D and plain.diff is None
    views = augment.ten_crop_views(H, W)[[4, 6]]  # the centre, and the mirror's top left
    assert views[:, 2].tolist() == [0, 1]
    weights = (1.0, 1.5, 0.5)
    kw = dict(n_snippets=3, views=(views, views), invert_flow_x=True)
    for bad in ((1.0, 1.5), (1.0, 1.0, 0.0, 1.0), (0.0, 0.0, 0.0)):
        with pytest.raises(ValueError):
            pipe.submit_video(rgb.cuda(), gray.cuda(), fusion_weights=bad, **kw)
    with pytest.raises(ValueError):
        plain.submit_video(rgb.cuda(), gray.cuda(), fusion_weights=weights, **kw)
    assert pipe._n == 0 and plain._n == 0
    out = pipe.run_video(rgb.cuda(), gray.cuda(), fusion_weights=weights, **kw)
    starts = snippetStarts(20, 10, 3)
    assert out["starts"] == starts and len(set(starts)) == 3
    # the difference volumes from the restatement, through the stream itself
    xd = s23_stack(rgb.numpy(), rgbdiff.view_table(starts, views).numpy(), D).reshape(3, 2, 3 * D, 224, 224)
    _, _, dd, ld = pipe.diff.forward_views(torch.from_numpy(xd).cuda())
    torch.cuda.synchronize()
    assert tuple(out["logits_d_items"].shape) == (3, 2, 101) and torch.equal(out["logits_d_items"], ld)
    assert np.array_equal(out["desc_d"].cpu().numpy(), _item_mean(dd.cpu().numpy())) and tuple(out["desc_d"].shape) == (256,)
    # rows first, middle and last against the torch-CPU oracle
    wd = _diff_weights(3 * D)
    flat = xd.reshape(6, 3 * D, 224, 224)
    rows = [0, 3, 5]
    _, _, ref = vgg_oracle.forward(torch.from_numpy(flat[rows]), wd["conv_w"], wd["conv_b"], wd["fc_w"], wd["fc_b"])
    err = float((ld.view(6, 101)[rows].cpu() - ref).abs().max())
    print("difference stream: max |logit - oracle| = %.3g" % err)
    assert err < 1e-3
    # consensus of the third stream, fusion of the three
    from video_analytics_amd import fusion
    assert torch.equal(out["scores_d"], fusion.score_consensus(ld.unsqueeze(0), "softmax")[0])
    rf, rp = s24_fuse([out[key].cpu().numpy() for key in ("scores_s", "scores_t", "scores_d")], weights)
    assert np.array_equal(out["scores"].cpu().numpy(), rf) and int(out["pred"]) == int(rp) and out["pred"].dtype == torch.int32
    # the other two streams: a plain pipeline's bits
    two = plain.run_video(rgb.cuda(), gray.cuda(), fusion_weights=weights[:2], **kw)
    for key in ("scores_s", "scores_t", "desc_s", "desc_t", "logits_s_items", "logits_t_items"):
        assert torch.equal(out[key], two[key]), key
    assert "scores_d" not in two and plain._dstack == [None, None]
    dflt = plain.run_video(rgb.cuda(), gray.cuda(), **kw)          # fusion_weights=None: (1, 1), the two-way path
    rf, rp = s16_fuse(dflt["scores_s"].cpu().numpy(), dflt["scores_t"].cpu().numpy(), 1.0, 1.0)
    assert np.array_equal(dflt["scores"].cpu().numpy(), rf) and int(dflt["pred"]) == int(rp)
    # pipelined: both videos submitted before either is waited for (different lengths: the buffers are re-allocated)
    keys = ("scores_s", "scores_t", "scores_d", "scores", "pred", "desc_s", "desc_t", "desc_d", "logits_s_items", "logits_t_items",
            "logits_d_items")
    one = {key: out[key].clone() for key in keys}
    nxt = pipe.run_video(rgb2.cuda(), gray2.cuda(), **kw)          # None on a difference pipeline: (1, 1, 1)
    nxt = {key: nxt[key].clone() for key in keys}
    rf, _ = s24_fuse([nxt[key].cpu().numpy() for key in ("scores_s", "scores_t", "scores_d")], (1.0, 1.0, 1.0))
    assert np.array_equal(nxt["scores"].cpu().numpy(), rf)
    a = pipe.submit_video(rgb.cuda(), gray.cuda(), fusion_weights=weights, **kw)
    b = pipe.submit_video(rgb2.cuda(), gray2.cuda(), **kw)
    pipe.wait()
    torch.cuda.synchronize()
    for key in keys:
        assert torch.equal(a[key], one[key]), key
        assert torch.equal(b[key], nxt[key]), key
    # one RGB frame per clip: submit / run_batch ignore the third stream
    from video_analytics_amd import synth
    crgb, cgray, _ = synth.synth_clips(2, seed=7)
    x, y = pipe.run_batch(crgb.cuda(), cgray.cuda()), plain.run_batch(crgb.cuda(), cgray.cuda())
    assert sorted(x) == sorted(y) and all(torch.equal(x[key], y[key]) for key in ("logits_s", "logits_t", "desc_s", "desc_t"))
    pipe.close()
    plain.close()


def _weights(m):
    st = m.export_state()
    return [t.cpu() for k in ("conv_w", "conv_b", "fc_w", "fc_b") for t in st[k]]


def _state(m):
    """The 34 parameters, then the 34 momentum buffers."""
    mo = m.export_state(momentum=True)
    return _weights(m) + [t.cpu() for k in ("conv_w", "conv_b", "fc_w", "fc_b") for t in mo[k]]


@pytest.fixture
def training_workspaces_released():
    """The training workspaces this module's pipelines and the twin stream allocate leave the cache again: tests that run
    later find the training workspace of their own model as the only one (tests/test_train_gpu.py reads it back)."""
    yield
    from video_analytics_amd import vgg
    torch.cuda.synchronize()
    for key in [key for key in vgg._ws_cache if "train" in str(key)]:
        del vgg._ws_cache[key]


def test_train_videos_with_the_difference_stream(training_workspaces_released):
    import random
    from video_analytics_amd import _ffi, augment, pipeline, vgg
    from video_analytics_amd.parameters import NACTION_CLASSES, VIDEO_DESCRIPTOR_DIM
    D, k, lr, mu, seed = 5, 3, 1e-4, 0.9, 5
    vids = [_synthetic_video(25, 240, 320, seed=61), _synthetic_video(37, 240, 320, seed=63)]
    starts = [[0, 3, 14], [2, 13, 26]]  # overlapping windows, the last possible starts
    dev = [(r.cuda(), g.cuda()) for r, g in vids]
    crops = augment.draw_scale_jitter_crops(6, 240, 320, random.Random(3))
    crops[1] = torch.tensor([10, 50, 224, 224, 1], dtype=torch.int32)  # one snippet at the network's own size
    labels = torch.tensor([5, 77])
    params = _ffi.default_tvl1_params(**SCHEDULE)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params, rgb_diff=True)
    plain = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    wd = pipeline.build_stream_weights(3 * D, 3, pipe.device)
    twin = vgg.Vgg16Stream(wd["conv_w"], wd["conv_b"], wd["fc_w"], wd["fc_b"], NACTION_CLASSES, VIDEO_DESCRIPTOR_DIM, device=0,
                           ws_slot=7)
    before = _weights(pipe.diff)
    assert len(before) == 34 and all(torch.equal(a, b) for a, b in zip(before, _weights(twin)))
    kw = dict(k=k, starts=starts, crops=crops, lr=lr, momentum=mu, dropout_seed=seed)
    out = pipe.train_videos(dev, labels, **kw)
    two = plain.train_videos(dev, labels, **kw)
    torch.cuda.synchronize()
    # the third stream's input from the restatement: every snippet's window of the whole video, through the snippet's crop
    xd = np.concatenate([s23_stack(rgb.numpy(), np.array([[s] + cr for s, cr in zip(st, crops[3 * v:3 * v + 3].tolist())]), D)
                         for v, ((rgb, _), st) in enumerate(zip(vids, starts))])
    assert xd.shape == (6, 3 * D, 224, 224)
    stats, desc = twin.train_step_consensus(torch.from_numpy(xd).cuda(), labels, k, lr, mu, seed)
    torch.cuda.synchronize()
    assert torch.equal(out["stats_d"], stats) and torch.equal(out["desc_d"], desc) and tuple(desc.shape) == (6, 256)
    got, ref = _state(pipe.diff), _state(twin)
    assert len(got) == 68 and all(torch.equal(a, b) for a, b in zip(got, ref))
    assert any(not torch.equal(a, b) for a, b in zip(got[:34], before))  # the weights moved
    assert bool(torch.isfinite(stats).all())
    for key in ("stats_s", "stats_t", "desc_s", "desc_t", "flow"):
        assert torch.equal(out[key], two[key]), key
    assert "stats_d" not in two
    for a, b in ((pipe.spatial, plain.spatial), (pipe.temporal, plain.temporal)):
        assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(b)))
    half = pipeline.TwoStreamPipeline(device=0, cnn_dtype="bf16", rgb_diff=True, rgb_diff_count=2)
    with pytest.raises(ValueError, match="fp32"):
        half.train_videos(dev, labels, **kw)
    for p in (pipe, plain, half):
        p.close()
    twin.close()


def test_evaluate_videos_with_and_without_the_difference_stream():
    from video_analytics_amd import _ffi, pipeline
    from video_analytics_amd.video import evaluateVideos
    params = _ffi.default_tvl1_params(epsilon=0.0, nscales=3, warps=1, iters=10)
    vids = [_synthetic_video(T, 224, 224, seed=50 + T) for T in (12, 15)]
    dev = [(r.cuda(), g.cuda()) for r, g in vids]
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params, rgb_diff=True)
    outs = [pipe.run_video(r, g, n_snippets=3) for r, g in dev]
    torch.cuda.synchronize()
    labels = [int(outs[0]["pred"]), (int(outs[1]["pred"]) + 1) % 101]
    res = evaluateVideos(pipe, dev, labels, n_snippets=3)
    assert len(res) == 5
    acc_s, acc_t, acc_f, desc, acc_d = res
    assert acc_f == pytest.approx(0.5) and desc.dtype == np.float32 and desc.shape == (2, 768)
    assert acc_d == pytest.approx(np.mean([int(o["scores_d"].argmax()) == l for o, l in zip(outs, labels)]))
    assert acc_s == pytest.approx(np.mean([int(o["scores_s"].argmax()) == l for o, l in zip(outs, labels)]))
    for i, o in enumerate(outs):
        assert np.array_equal(desc[i], torch.cat([o["desc_s"], o["desc_t"], o["desc_d"]]).cpu().numpy())
    pipe.close()
    plain = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    res = evaluateVideos(plain, dev, labels, n_snippets=3)
    assert len(res) == 4 and res[3].shape == (2, 512)
    plain.close()
