"""Whole-video evaluation on the device: va_flow_to_stack_snippets against numpy gathers of the
oracle's S9 volume, va_score_consensus / va_fuse_scores against the float64 witness of tests/test_video_host.py, and
TwoStreamPipeline.run_video at 320x240 against independently built inputs, the TV-L1 oracle and the torch-CPU oracle."""
import numpy as np
import pytest
import torch

from test_motion_host import s11_means, s12_motion
from test_video_host import consensus_f64, consensus_tolerance, fuse_f64, s15_source_planes, s16_fuse
from video_analytics_amd.video import evaluateVideos, snippetPlan, snippetStarts

pytestmark = pytest.mark.gpu

MEAN, STD = np.float32(0.485), np.float32(0.229)
SCHEDULE = dict(epsilon=0.0, nscales=5, warps=3, iters=30)  # the golden fixtures' schedule


def _normalise(q_u8):
    return (q_u8.astype(np.float32) / np.float32(255.0) - MEAN) / STD


def _snippet_rows(fl, starts, views, L, invert, oracle):
    """numpy reference of S15: the oracle's S9 volume of flow [N,2,H,W] (or, for mirrored x-flow planes with ``invert``,
    255 - q of utils.flowToImages), output plane o = (s*V + v)*2L + c reading source plane 2*(starts[s] + c//2) + c%2
    through view v -> [n*V*2L, 224, 224]."""
    from video_analytics_amd import utils
    N, _, H, W = fl.shape
    full = oracle.flow_to_stack(fl)
    inv = _normalise(255 - utils.flowToImages(fl).reshape(2 * N, H, W)) if invert else None
    V = views.shape[0]
    src = s15_source_planes(starts, L, V)
    out = np.empty((len(src), 224, 224), dtype=np.float32)
    for o, p in enumerate(src.tolist()):
        top, left, flip = views[(o // (2 * L)) % V].tolist()
        plane = inv[p] if (invert and flip and p % 2 == 0) else full[p]
        win = plane[top:top + 224, left:left + 224]
        out[o] = win[:, ::-1] if flip else win
    return out


# ---- S15: the snippet gather ----

@pytest.mark.parametrize("h,w", [(240, 320), (241, 321)])
@pytest.mark.parametrize("invert", [False, True])
def test_snippet_gather_equals_s9_then_gather(oracle_tvl1, h, w, invert):
    from video_analytics_amd import augment
    from video_analytics_amd import flow as vflow
    L, N = 10, 36
    rs = np.random.RandomState(h + int(invert))
    fl = (rs.standard_normal((N, 2, h, w)) * 12.0).astype(np.float32)  # sigma 12 px: both clamps at +-20 are hit
    assert (fl > 20).any() and (fl < -20).any()
    views = augment.ten_crop_views(h, w)
    starts = [0, 1, 1, 7, 13, 26, 26]  # overlapping windows, duplicates, the last possible start
    d = torch.from_numpy(fl).cuda()
    got = vflow.crop_flow_to_stack_snippets(d, starts, views, L, invert_x_on_flip=invert)
    assert tuple(got.shape) == (len(starts), 10, 2 * L, 224, 224)
    ref = _snippet_rows(fl, starts, views, L, invert, oracle_tvl1)
    assert np.array_equal(got.cpu().numpy().reshape(-1, 224, 224), ref)
    # an unaligned volume (4 bytes past a 16-byte boundary): the scalar store path
    flat = torch.empty(got.numel() + 1, dtype=torch.float32, device="cuda")
    assert flat[1:].data_ptr() % 16 == 4
    un = vflow.crop_flow_to_stack_snippets(d, starts, views, L, invert_x_on_flip=invert, out=flat[1:])
    assert torch.equal(un, got)
    # the plan of a 37-frame video: 25 overlapping windows of its 36 fields, three views
    plan = snippetPlan(37, L, 25)
    got = vflow.crop_flow_to_stack_snippets(d, plan.index, views[3:6], L, invert_x_on_flip=invert)
    ref = _snippet_rows(fl, plan.index, views[3:6], L, invert, oracle_tvl1)
    assert np.array_equal(got.cpu().numpy().reshape(-1, 224, 224), ref)


@pytest.mark.parametrize("invert", [False, True])
def test_snippet_gather_with_disjoint_windows_is_the_views_gather(invert):
    from video_analytics_amd import augment
    from video_analytics_amd import flow as vflow
    B, L, h, w = 5, 10, 240, 320
    rs = np.random.RandomState(77)
    fl = torch.from_numpy((rs.standard_normal((B * L, 2, h, w)) * 12.0).astype(np.float32)).cuda()
    views = augment.ten_crop_views(h, w)
    a = vflow.crop_flow_to_stack_snippets(fl, [b * L for b in range(B)], views, L, invert_x_on_flip=invert)
    b = vflow.crop_flow_to_stack_views(fl, views, L, invert_x_on_flip=invert)
    assert torch.equal(a, b)


def test_snippet_gather_refuses_bad_arguments():
    from video_analytics_amd import _ffi, augment
    from video_analytics_amd import flow as vflow
    fl = torch.zeros(12, 2, 240, 320, device="cuda")
    views = augment.ten_crop_views(240, 320)
    for bad in ([3], [-1], []):
        with pytest.raises(ValueError):
            vflow.crop_flow_to_stack_snippets(fl, bad, views, 10)
    with pytest.raises(ValueError):
        vflow.crop_flow_to_stack_snippets(fl, [0], views, 13)
    L = _ffi.lib()
    c = _ffi.ctx(0)
    out = torch.zeros(1, 10, 20, 224, 224, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    cr = augment.crops_to_device(augment.expand_views(views, 1, 20), fl.device)

    def call(n_pairs=12, starts=st, n=1, flow_count=10, V=10, inv=0):
        return L.va_flow_to_stack_snippets(c, _ffi.ptr(fl), n_pairs, _ffi.ptr(starts), n, flow_count, V, 320, 240, 20.0, 0.485,
                                           0.229, _ffi.ptr(cr), inv, 224, 224, _ffi.ptr(out), _ffi.stream_ptr(fl.device))
    assert call() == _ffi.VA_OK
    for kw in (dict(n_pairs=9), dict(starts=None), dict(n=0), dict(flow_count=0), dict(V=0), dict(inv=2), dict(n=4000)):
        assert call(**kw) == _ffi.VA_ERR_INVALID, kw
    torch.cuda.synchronize()


# ---- S16: consensus and fusion ----

@pytest.mark.parametrize("mode", ["softmax", "logits"])
def test_consensus_agrees_with_the_float64_witness(mode):
    from video_analytics_amd import fusion
    rs = np.random.RandomState(160 + len(mode))
    worst = 0.0
    for (n, k, c) in [(6, 250, 101), (3, 25, 101), (2, 1, 7), (2, 10, 300), (1, 3, 2), (1, 250, 1)]:
        for scale in (0.5, 3.0, 10.0, 30.0):
            x = (rs.standard_normal((n, k, c)) * scale).astype(np.float32)
            d = torch.from_numpy(x).cuda()
            got = fusion.score_consensus(d, mode)
            again = fusion.score_consensus(d, mode)
            assert tuple(got.shape) == (n, c) and torch.equal(got, again)  # deterministic
            g = got.cpu().numpy()
            assert (g >= 0).all() and (g <= 1).all()
            for i in range(n):
                err = float(np.abs(g[i].astype(np.float64) - consensus_f64(x[i], mode)).max())
                worst = max(worst, err)
                print("consensus %s n=%d k=%d c=%d scale=%g video %d: max |device - witness| = %.3g (tolerance %.3g)"
                      % (mode, n, k, c, scale, i, err, consensus_tolerance(c, k)))
                assert err <= consensus_tolerance(c, k), (n, k, c, scale, i, err)
    print("consensus %s: worst |device - witness| = %.3g" % (mode, worst))
    # [N,n,V,C] is read snippet-major
    x = (rs.standard_normal((2, 5, 10, 101)) * 3).astype(np.float32)
    d = torch.from_numpy(x).cuda()
    assert torch.equal(fusion.score_consensus(d, mode), fusion.score_consensus(d.view(2, 50, 101), mode))


@pytest.mark.parametrize("mode", ["softmax", "logits"])
@pytest.mark.parametrize("weights", [(1.0, 1.0), (1.0, 1.5)])
def test_fused_prediction_equals_the_witness_on_every_video(mode, weights):
    from video_analytics_amd import fusion
    rs = np.random.RandomState(7)
    n, k, c = 12, 250, 101
    scale = np.repeat([0.5, 1.0, 3.0], 4).astype(np.float32)[:, None, None]  # three logit scales
    xs = (rs.standard_normal((n, k, c)).astype(np.float32) * scale).astype(np.float32)
    xt = (rs.standard_normal((n, k, c)).astype(np.float32) * scale).astype(np.float32)
    win = rs.randint(0, c, size=n)
    for i in range(n):  # the planted winner: +2 on one class in every item of both streams
        xs[i, :, win[i]] += np.float32(2.0)
        xt[i, :, win[i]] += np.float32(2.0)
    tol = consensus_tolerance(c, k)
    ref = np.stack([fuse_f64(consensus_f64(xs[i], mode), consensus_f64(xt[i], mode), *weights) for i in range(n)])
    top = np.sort(ref, axis=1)
    assert ((top[:, -1] - top[:, -2]) > 2 * tol).all(), (top[:, -1] - top[:, -2]).min()  # before the device is looked at
    ss = fusion.score_consensus(torch.from_numpy(xs).cuda(), mode)
    st = fusion.score_consensus(torch.from_numpy(xt).cuda(), mode)
    fused, pred = fusion.fuse_scores(ss, st, weights)
    fused2, pred2 = fusion.fuse_scores(ss, st, weights)
    assert torch.equal(fused, fused2) and torch.equal(pred, pred2) and pred.dtype == torch.int32
    assert np.array_equal(pred.cpu().numpy(), np.argmax(ref, axis=1)) and np.array_equal(np.argmax(ref, axis=1), win)
    err = float(np.abs(fused.cpu().numpy().astype(np.float64) - ref).max())
    print("fused %s %s: max |device - witness| = %.3g" % (mode, weights, err))
    assert err <= tol + 4 * 2.0 ** -24


@pytest.mark.parametrize("weights", [(1.0, 1.0), (1.0, 1.5), (0.0, 2.0), (3.0, 0.0), (0.25, 7.0)])
def test_fuse_scores_within_four_ulp_and_first_maximum_wins(weights):
    from video_analytics_amd import fusion
    rs = np.random.RandomState(int(weights[1] * 8))
    a = rs.dirichlet(np.ones(101), size=33).astype(np.float32)
    b = rs.dirichlet(np.ones(101), size=33).astype(np.float32)
    a[5, :] = 0.0
    b[5, :] = 0.0
    a[5, [17, 60]] = 0.5   # an exact tie: the first maximum wins
    b[5, [17, 60]] = 0.5
    fused, pred = fusion.fuse_scores(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), weights)
    f = fused.cpu().numpy()
    ref = fuse_f64(a, b, *weights)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    worst = float((np.abs(f.astype(np.float64) - ref) / ulp).max())
    print("fuse_scores %s: worst error %.3g ulp" % (weights, worst))
    assert worst <= 4.0
    rf, rp = s16_fuse(a, b, *weights)
    assert np.array_equal(f, rf) and np.array_equal(pred.cpu().numpy(), rp)  # the float32 restatement, bit for bit
    assert int(pred[5]) == 17 and f[5, 17] == f[5, 60]


def test_consensus_ties_nan_and_bad_arguments():
    from video_analytics_amd import _ffi, fusion
    rs = np.random.RandomState(3)
    x = rs.standard_normal((3, 40, 101)).astype(np.float32)
    x[:, :, 2] += 3.0
    x[:, :, 5] = x[:, :, 2]        # two identical columns: identical scores in either mode
    for mode in ("softmax", "logits"):
        s = fusion.score_consensus(torch.from_numpy(x).cuda(), mode)
        assert torch.equal(s[:, 2], s[:, 5])
        _, pred = fusion.fuse_scores(s, s, (1.0, 1.5))
        assert pred.tolist() == [2, 2, 2]
        y = x.copy()
        y[1, 7, 3] = np.nan
        s = fusion.score_consensus(torch.from_numpy(y).cuda(), mode).cpu().numpy()
        assert np.isnan(s[1]).all() and not np.isnan(s[[0, 2]]).any()
    a = torch.zeros(2, 101, device="cuda")
    for w in ((-1.0, 2.0), (0.0, 0.0), (1.0,), (float("nan"), 1.0)):
        with pytest.raises(ValueError):
            fusion.fuse_scores(a, a, w)
    with pytest.raises(ValueError):
        fusion.score_consensus(a.view(2, 1, 101), "max")
    with pytest.raises(ValueError):
        fusion.score_consensus(torch.zeros(1, 5000, 4, device="cuda"))
    L, c = _ffi.lib(), _ffi.ctx(0)
    p = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert L.va_fuse_scores(c, _ffi.ptr(a), _ffi.ptr(a), 2, 101, -1.0, 2.0, _ffi.ptr(a), _ffi.ptr(p), None) == _ffi.VA_ERR_INVALID
    assert L.va_fuse_scores(c, _ffi.ptr(a), _ffi.ptr(a), 2, 101, 0.0, 0.0, _ffi.ptr(a), _ffi.ptr(p), None) == _ffi.VA_ERR_INVALID
    assert L.va_score_consensus(c, _ffi.ptr(a), 2, 1, 101, 2, _ffi.ptr(a), None) == _ffi.VA_ERR_INVALID


# ---- the pipeline ----

def _synthetic_video(T, H, W, seed):
    """rgb u8 [T,3,H,W] (independent frames) and gray u8 [T,H,W] (one moving texture)."""
    from video_analytics_amd import synth
    rgb, _, _ = synth.synth_clips(T, seed=seed, H=H, W=W, n_gray=2)
    _, gray, _ = synth.synth_clips(1, seed=seed + 1, H=H, W=W, n_gray=T)
    return rgb, gray[0]


def _rgb_views(rgb, frames, views):
    xs = np.empty((len(frames), views.shape[0], 3, 224, 224), dtype=np.uint8)
    r = rgb.numpy()
    for i, f in enumerate(frames):
        for v, (top, left, flip) in enumerate(views.tolist()):
            win = r[f, :, top:top + 224, left:left + 224]
            xs[i, v] = win[:, :, ::-1] if flip else win
    return xs


def _item_mean(x):
    """[n,V,d] float32 -> [d]: added in item order, one division."""
    p = x.reshape(-1, x.shape[-1])
    acc = p[0].copy()
    for i in range(1, p.shape[0]):
        acc = acc + p[i]
    return acc / np.float32(p.shape[0])


def _check_video_output(out, pipe, rgb, gray, views_s, views_t, invert, mode, weights, oracle, field=None):
    """Everything run_video returns, against inputs built independently from the TV-L1 oracle's flow."""
    from oracle import vgg_oracle
    from video_analytics_amd import synth
    from video_analytics_amd.parameters import NORM_MEANS_TF, NORM_STDS_TF
    T, L = gray.shape[0], pipe.L
    n = len(out["starts"])
    plan = snippetPlan(T, L, n)
    assert out["starts"] == snippetStarts(T, L, n)
    # the planned flows are the oracle's TV-L1 of those frame pairs, each computed once
    fl_all = oracle.tvl1_flow(gray.numpy()[None], oracle.default_params(**SCHEDULE), nthreads=0)  # [T-1,2,H,W]
    fl = fl_all[plan.pairs]
    k = (pipe._n - 1) % pipe.depth
    assert tuple(pipe._flow[k].shape) == (len(plan.pairs), 2) + tuple(gray.shape[1:])
    assert np.array_equal(pipe._flow[k].cpu().numpy(), fl)
    if field is not None:
        fl = field(fl)
    xt = _snippet_rows(fl, plan.index, views_t, L, invert, oracle).reshape(n, views_t.shape[0], 2 * L, 224, 224)
    xs = _rgb_views(rgb, plan.starts, views_s)
    _, _, ds, ls = pipe.spatial.forward_views(torch.from_numpy(xs).cuda())
    _, _, dt, lt = pipe.temporal.forward_views(torch.from_numpy(xt).cuda())
    torch.cuda.synchronize()
    assert torch.equal(out["logits_s_items"], ls) and torch.equal(out["logits_t_items"], lt)
    assert tuple(ls.shape) == (n, views_s.shape[0], 101) and tuple(lt.shape) == (n, views_t.shape[0], 101)
    assert np.array_equal(out["desc_s"].cpu().numpy(), _item_mean(ds.cpu().numpy()))
    assert np.array_equal(out["desc_t"].cpu().numpy(), _item_mean(dt.cpu().numpy()))
    # consensus and fusion of those logits
    rs_ = consensus_f64(ls.cpu().numpy().reshape(-1, 101), mode)
    rt_ = consensus_f64(lt.cpu().numpy().reshape(-1, 101), mode)
    assert float(np.abs(out["scores_s"].cpu().numpy() - rs_).max()) <= consensus_tolerance(101, ls.shape[0] * ls.shape[1])
    assert float(np.abs(out["scores_t"].cpu().numpy() - rt_).max()) <= consensus_tolerance(101, lt.shape[0] * lt.shape[1])
    rf, rp = s16_fuse(out["scores_s"].cpu().numpy(), out["scores_t"].cpu().numpy(), *weights)
    assert np.array_equal(out["scores"].cpu().numpy(), rf) and int(out["pred"]) == int(rp)
    assert out["pred"].dtype == torch.int32 and tuple(out["scores"].shape) == (101,) and tuple(out["desc_s"].shape) == (256,)
    # rows 0, one in the middle and the last against the torch-CPU oracle
    ws = synth.synth_vgg16_weights(c_in=3, seed=1)
    wt = synth.synth_vgg16_weights(c_in=20, seed=2)
    wt["conv_w"][0] = vgg_oracle.copy_first_layer(wt["conv_w"][0], 20)
    for x, w, got, norm in ((xs, ws, ls, True), (xt, wt, lt, False)):
        flat = x.reshape((-1,) + x.shape[2:])
        rows = [0, flat.shape[0] // 2, flat.shape[0] - 1]
        xr = torch.from_numpy(flat[rows])
        if norm:
            xr = vgg_oracle.normalize_u8(xr, NORM_MEANS_TF, NORM_STDS_TF)
        _, _, ref = vgg_oracle.forward(xr, w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"])
        assert float((got.reshape(-1, 101)[rows].cpu() - ref).abs().max()) < 1e-3


def test_run_video_37_frames_ten_views(oracle_tvl1):
    from video_analytics_amd import _ffi, augment, pipeline
    T, H, W = 37, 240, 320
    rgb, gray = _synthetic_video(T, H, W, seed=41)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(**SCHEDULE))
    views = augment.ten_crop_views(H, W)
    for bad in (dict(views=None), dict(views=(views, views), crops=augment.draw_clip_crops(25, 10, (H, W), (H, W))),
                dict(views=(views, views), consensus="max"), dict(views=(views, views), fusion_weights=(0, 0))):
        with pytest.raises(ValueError):
            pipe.submit_video(rgb.cuda(), gray.cuda(), **bad)
    with pytest.raises(ValueError):
        pipe.submit_video(rgb[:10].cuda(), gray[:10].cuda(), views=(views, views))  # 9 pairs < L
    with pytest.raises(ValueError):
        pipe.submit_video(rgb, gray, views=(views, views))  # host tensors
    assert pipe._n == 0
    out = pipe.run_video(rgb.cuda(), gray.cuda(), views=(views, views), invert_flow_x=True, fusion_weights=(1.0, 1.5))
    assert out["plan"].pair_computations == 36 and len(set(out["starts"])) == 25
    _check_video_output(out, pipe, rgb, gray, views, views, True, "softmax", (1.0, 1.5), oracle_tvl1)
    pipe.close()


def test_run_video_20_frames_and_pipelined_pair(oracle_tvl1):
    from video_analytics_amd import _ffi, augment, pipeline
    H, W = 240, 320
    rgb, gray = _synthetic_video(20, H, W, seed=43)
    rgb2, gray2 = _synthetic_video(37, H, W, seed=45)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(**SCHEDULE))
    views = augment.ten_crop_views(H, W)
    vs, vt = views[4:5], views[3:6]  # a table of any length per stream
    kw = dict(views=(vs, vt), consensus="logits")
    out = pipe.run_video(rgb.cuda(), gray.cuda(), **kw)
    assert len(set(out["starts"])) == 10 and out["plan"].pair_computations == 19  # duplicates kept: 25 snippets
    assert tuple(out["logits_t_items"].shape) == (25, 3, 101) and tuple(out["logits_s_items"].shape) == (25, 1, 101)
    _check_video_output(out, pipe, rgb, gray, vs, vt, False, "logits", (1.0, 1.0), oracle_tvl1)
    keys = ("scores_s", "scores_t", "scores", "pred", "desc_s", "desc_t", "logits_s_items", "logits_t_items")
    one = {key: out[key].clone() for key in keys}
    two = pipe.run_video(rgb2.cuda(), gray2.cuda(), **kw)
    two = {key: two[key].clone() for key in keys}
    # pipelined: both videos submitted before either is waited for (different lengths: the buffers are re-allocated)
    a = pipe.submit_video(rgb.cuda(), gray.cuda(), **kw)
    b = pipe.submit_video(rgb2.cuda(), gray2.cuda(), **kw)
    pipe.wait()
    torch.cuda.synchronize()
    for key in keys:
        assert torch.equal(a[key], one[key]), key
        assert torch.equal(b[key], two[key]), key
    pipe.close()


def test_run_video_with_mean_flow(oracle_tvl1):
    from video_analytics_amd import _ffi, augment, pipeline
    H, W = 240, 320
    rgb, gray = _synthetic_video(20, H, W, seed=47)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(**SCHEDULE), mean_flow=True)
    views = augment.ten_crop_views(H, W)
    vs, vt = views[4:5], views[7:9]
    out = pipe.run_video(rgb.cuda(), gray.cuda(), n_snippets=5, views=(vs, vt), invert_flow_x=True)

    def field(fl):  # S11 then S12 per planned field
        return s12_motion(fl, 1, False, s11_means(fl))
    _check_video_output(out, pipe, rgb, gray, vs, vt, True, "softmax", (1.0, 1.0), oracle_tvl1, field=field)
    pipe.close()
    for motion in ("trajectory", "bidirectional"):
        bad = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(**SCHEDULE), motion=motion)
        with pytest.raises(ValueError):
            bad.submit_video(rgb.cuda(), gray.cuda(), views=(vs, vt))
        assert bad._n == 0
        bad.close()


def test_evaluate_videos_single_view():
    from video_analytics_amd import _ffi, pipeline
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(epsilon=0.0, nscales=3, warps=1, iters=10))
    vids = [_synthetic_video(T, 224, 224, seed=50 + T) for T in (12, 15, 11)]
    dev = [(r.cuda(), g.cuda()) for r, g in vids]
    outs = [pipe.run_video(r, g, n_snippets=3) for r, g in dev]
    torch.cuda.synchronize()
    ps = [int(o["scores_s"].argmax()) for o in outs]
    pt = [int(o["scores_t"].argmax()) for o in outs]
    pf = [int(o["pred"]) for o in outs]
    labels = [pf[0], (pf[1] + 1) % 101, pf[2]]
    acc_s, acc_t, acc_f, desc = evaluateVideos(pipe, dev, labels, n_snippets=3)
    assert acc_f == pytest.approx(2.0 / 3.0)
    assert acc_s == pytest.approx(np.mean([p == l for p, l in zip(ps, labels)]))
    assert acc_t == pytest.approx(np.mean([p == l for p, l in zip(pt, labels)]))
    assert desc.dtype == np.float32 and desc.shape == (3, 512)
    for i, o in enumerate(outs):
        assert np.array_equal(desc[i], torch.cat([o["desc_s"], o["desc_t"]]).cpu().numpy())
    with pytest.raises(ValueError):
        evaluateVideos(pipe, dev, labels[:2], n_snippets=3)
    pipe.close()
