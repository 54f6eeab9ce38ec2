"""TSN training on the device: the two crop-resize gathers against the float32 restatement of
tests/test_tsn_host.py bit for bit, the consensus step against the plain step (k = 1, bit for bit) and against torch-CPU
autograd + torch.optim.SGD (k = 3), and TwoStreamPipeline.train_videos against the same composition built independently
from the TV-L1 oracle's flow."""
import random

import numpy as np
import pytest
import torch

from test_train_gpu import TOL_UPDATE, _relerr, _rmserr
from test_tsn_host import s17_flow_stack, s17_images_u8
from test_video_gpu import SCHEDULE, _synthetic_video

pytestmark = pytest.mark.gpu


def _all_crops(h, w):
    """Every size pair x all 13 fixed offsets x both flip states -> rows {top, left, ch, cw, flip}."""
    from video_analytics_amd import augment
    rows = []
    for cw, ch in augment.scale_jitter_sizes(h, w)[1]:
        for left, top in augment.fixed_offsets(h, w, ch, cw, more=True):
            for flip in (0, 1):
                rows.append([top, left, ch, cw, flip])
    assert len(rows) == 260
    return rows


def _table(rows, n_src, seed):
    """Rows with a source each: planes repeat and overlap (n_src << len(rows)), neighbours share one now and then."""
    rs = np.random.RandomState(seed)
    src = rs.randint(0, n_src, size=len(rows))
    src[1::7] = src[0::7][:len(src[1::7])]
    return torch.tensor([[int(s)] + r for s, r in zip(src, rows)], dtype=torch.int32)


def _flows(h, w):
    """name -> float32 [3,2,h,w]: a smooth field that passes both clamps, sigma = 12 noise, and TV-L1 flow."""
    from video_analytics_amd import _ffi, synth
    from video_analytics_amd import flow as vflow
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    smooth = np.stack([np.stack([25.0 * np.sin(xx / (9.0 + i)) * np.cos(yy / 17.0), 25.0 * np.cos(xx / 23.0 + i) * np.sin(yy / 11.0)])
                       for i in range(3)]).astype(np.float32)
    noise = (np.random.RandomState(h).standard_normal((3, 2, h, w)) * 12.0).astype(np.float32)
    assert (noise > 20).any() and (noise < -20).any() and (smooth > 20).any() and (smooth < -20).any()
    _, gray, _ = synth.synth_clips(1, seed=h, H=h, W=w, n_gray=4)
    tv = vflow.tvl1_flow(gray.cuda(), _ffi.default_tvl1_params(**SCHEDULE)).cpu().numpy()
    assert tv.shape == (3, 2, h, w) and np.isfinite(tv).all() and np.abs(tv).max() > 0.1
    return dict(smooth=smooth, noise=noise, tvl1=tv)


# ---- S17: the gathers ----

@pytest.mark.parametrize("h,w", [(240, 320), (241, 321)])
def test_flow_resize_gather_equals_the_restatement_bit_for_bit(h, w):
    from video_analytics_amd import flow as vflow
    rows = _all_crops(h, w)
    for name, fl in _flows(h, w).items():
        d = torch.from_numpy(fl).cuda()
        for invert in (False, True):
            table = _table(rows, 6, seed=len(name) + int(invert))
            ref = s17_flow_stack(fl, table.numpy(), invert)
            out = torch.full((len(rows), 224, 224), float("nan"), device="cuda")
            got = vflow.resize_flow_to_stack(d, table, invert_x_on_flip=invert, out=out)
            g = got.cpu().numpy()
            assert not np.isnan(g).any()
            bad = int((g != ref).sum())
            print("%dx%d %s invert=%d: %d of %d values differ from the restatement" % (w, h, name, invert, bad, ref.size))
            assert np.array_equal(g, ref), (name, invert, bad)
            assert invert is False or name != "noise" or not np.array_equal(ref, s17_flow_stack(fl, table.numpy(), False))
    # an unaligned volume (4 bytes past a 16-byte boundary): the scalar store path
    flat = torch.full((len(rows) * 224 * 224 + 1,), float("nan"), device="cuda")
    assert flat[1:].data_ptr() % 16 == 4
    un = vflow.resize_flow_to_stack(d, table, invert_x_on_flip=True, out=flat[1:])
    assert torch.equal(un, got)


@pytest.mark.parametrize("h,w", [(240, 320), (241, 321)])
@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
def test_image_resize_gather_equals_the_restatement_bit_for_bit(h, w, layout):
    from video_analytics_amd import augment
    rows = _all_crops(h, w)
    rs = np.random.RandomState(h + len(layout))
    shape = (3, 3, h, w) if layout == "NCHW" else (3, h, w, 3)
    x = rs.randint(0, 256, size=shape).astype(np.uint8)
    table = _table(rows, 3, seed=w)
    ref = s17_images_u8(x, table.numpy(), layout)
    d = torch.from_numpy(x).cuda()
    got = augment.resize_images(d, table, layout=layout)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(rows), 3, 224, 224)
    g = got.cpu().numpy()
    print("%dx%d %s: %d of %d bytes differ from the restatement" % (w, h, layout, int((g != ref).sum()), ref.size))
    assert np.array_equal(g, ref)
    flat = torch.full((got.numel() + 1,), 77, dtype=torch.uint8, device="cuda")
    assert flat[1:].data_ptr() % 4 == 1
    un = augment.resize_images(d, table, layout=layout, out=flat[1:])
    assert torch.equal(un, got) and int(flat[0]) == 77


@pytest.mark.parametrize("h,w", [(240, 320), (241, 321), (224, 224)])
def test_224_tables_are_the_plain_crop_gathers(h, w):
    from video_analytics_amd import augment
    from video_analytics_amd import flow as vflow
    rng = random.Random(h)
    N = 5
    fl = torch.from_numpy((np.random.RandomState(w).standard_normal((N, 2, h, w)) * 12.0).astype(np.float32)).cuda()
    crops = augment.draw_flow_crops(1, N, h, w, rng=rng)                 # [2N,3] {top, left, flip}
    size = torch.full((2 * N, 2), 224, dtype=torch.int32)
    table = torch.cat([torch.arange(2 * N, dtype=torch.int32).view(-1, 1), crops[:, :2], size, crops[:, 2:]], dim=1)
    for invert in (False, True):
        a = vflow.resize_flow_to_stack(fl, table, invert_x_on_flip=invert)
        b = vflow.crop_flow_to_stack(fl, crops, invert_x_on_flip=invert)
        assert torch.equal(a, b), invert
    for layout in ("NCHW", "NHWC"):
        shape = (4, 3, h, w) if layout == "NCHW" else (4, h, w, 3)
        x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(h)).cuda()
        ic = augment.draw_image_crops(4, h, w, rng=rng)
        it = torch.cat([torch.arange(4, dtype=torch.int32).view(-1, 1), ic[:, :2], size[:4], ic[:, 2:]], dim=1)
        assert torch.equal(augment.resize_images(x, it, layout=layout), augment.crop_images(x, ic, layout=layout))


def test_resize_gathers_refuse_bad_arguments():
    from video_analytics_amd import _ffi, augment
    from video_analytics_amd import flow as vflow
    fl = torch.zeros(2, 2, 240, 320, device="cuda")
    x = torch.zeros(2, 3, 240, 320, dtype=torch.uint8, device="cuda")
    good = torch.tensor([[3, 0, 0, 240, 240, 1]], dtype=torch.int32)
    assert tuple(vflow.resize_flow_to_stack(fl, good).shape) == (1, 224, 224)
    for bad in ([[4, 0, 0, 240, 240, 0]], [[0, 1, 0, 240, 240, 0]], [[0, 0, 81, 240, 240, 0]], [[0, 0, 0, 0, 240, 0]],
                [[0, 0, 0, 240, 240, 3]]):
        with pytest.raises(ValueError):
            vflow.resize_flow_to_stack(fl, torch.tensor(bad, dtype=torch.int32))
    with pytest.raises(ValueError):
        vflow.resize_flow_to_stack(fl, good.cuda())
    with pytest.raises(ValueError):
        vflow.resize_flow_to_stack(fl, good, out=torch.zeros(2, 224, 224, device="cuda"))
    with pytest.raises(ValueError):
        augment.resize_images(x, torch.tensor([[2, 0, 0, 240, 240, 0]], dtype=torch.int32))
    with pytest.raises(ValueError):
        augment.resize_images(x.float(), good)
    with pytest.raises(ValueError):
        augment.resize_images(x, good, layout="CHWN")
    L, c = _ffi.lib(), _ffi.ctx(0)
    tab = good.cuda()
    out = torch.zeros(1, 224, 224, device="cuda")
    st = _ffi.stream_ptr(fl.device)

    def call(flow=fl, n_pairs=2, w=320, h=240, bound=20.0, std=0.229, table=tab, n_out=1, inv=0):
        return L.va_flow_to_stack_resize(c, _ffi.ptr(flow), n_pairs, w, h, bound, 0.485, std, _ffi.ptr(table), n_out, inv,
                                         _ffi.ptr(out), st)
    assert call() == _ffi.VA_OK
    for kw in (dict(flow=None), dict(table=None), dict(n_pairs=0), dict(w=0), dict(n_out=0), dict(n_out=70000), dict(inv=2),
               dict(bound=0.0), dict(std=0.0)):
        assert call(**kw) == _ffi.VA_ERR_INVALID, kw
    o8 = torch.zeros(1, 3, 224, 224, dtype=torch.uint8, device="cuda")

    def call8(src=x, n=2, ch=3, nhwc=0, table=tab, n_out=1):
        return L.va_resize_images_u8(c, _ffi.ptr(src), n, ch, 320, 240, nhwc, _ffi.ptr(table), n_out, _ffi.ptr(o8), st)
    assert call8() == _ffi.VA_OK  # src 3 is clamped to image 1 on the device: nothing is read out of bounds
    for kw in (dict(src=None), dict(table=None), dict(n=0), dict(ch=0), dict(nhwc=2), dict(n_out=0), dict(n_out=30000)):
        assert call8(**kw) == _ffi.VA_ERR_INVALID, kw
    torch.cuda.synchronize()


# ---- S20: the consensus step ----

def _state(m):
    st, mo = m.export_state(), m.export_state(momentum=True)
    return [t.cpu() for d in (st, mo) for k in ("conv_w", "conv_b", "fc_w", "fc_b") for t in d[k]]


@pytest.mark.parametrize("c_in,B,u8", [(3, 4, False), (3, 2, True), (20, 3, False)])
def test_consensus_step_with_one_snippet_is_the_plain_step(c_in, B, u8):
    from video_analytics_amd import synth, vgg
    from video_analytics_amd.parameters import NORM_MEANS_TF, NORM_STDS_TF
    w = synth.synth_vgg16_weights(c_in=3, seed=4)
    if c_in != 3:
        w["conv_w"][0] = vgg.copy_first_layer(w["conv_w"][0].cuda(), c_in).cpu()
    norm = (NORM_MEANS_TF, NORM_STDS_TF) if u8 else (None, None)
    u = synth.hash_uniform(71, c_in, B * c_in * 224 * 224).reshape(B, c_in, 224, 224)
    x = torch.from_numpy((u * 255.0).astype(np.uint8) if u8 else u * 4.0 - 2.0).cuda()
    labels = torch.tensor([(7 * i + 1) % 101 for i in range(B)], dtype=torch.int64)
    res = []
    for consensus in (False, True):
        m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, *norm)
        for step in range(2):  # the second step exercises the momentum buffers
            if consensus:
                stats, desc = m.train_step_consensus(x, labels.cuda(), 1, 1e-4, 0.9, 1000 + step)
            else:
                stats, desc = m.train_step(x, labels.cuda(), 1e-4, 0.9, 1000 + step)
        res.append((stats.cpu(), desc.cpu(), _state(m)))
        m.close()
    assert torch.isfinite(res[0][0]).all() and float(res[0][0][0]) > 0
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert len(res[0][2]) == 68 and all(torch.equal(a, b) for a, b in zip(res[0][2], res[1][2]))


def test_consensus_step_matches_autograd_on_the_mean_of_three_snippets():
    """n = 8 videos of k = 3 snippets against torch-CPU autograd of cross_entropy(logits.view(n, k, -1).mean(1), y) +
    torch.optim.SGD with the same dropout masks, at the tolerances of tests/test_train_gpu.py's plain step."""
    import torch.nn.functional as F
    from oracle import train_oracle, vgg_oracle
    from video_analytics_amd import synth, vgg
    torch.set_num_threads(8)
    n, k = 8, 3
    B = n * k
    w = synth.synth_vgg16_weights(c_in=3, seed=4)
    lr, mu, seed = 1e-4, 0.9, 1003
    x = torch.from_numpy(synth.hash_uniform(72, 3, B * 3 * 224 * 224).reshape(B, 3, 224, 224) * 4.0 - 2.0)
    labels = torch.tensor([(7 * i + 1) % 101 for i in range(n)], dtype=torch.int64)
    ora = train_oracle.TrainOracle(w, lr, mu)
    p = ora.params
    op = vgg_oracle.features(x, p["conv_w"], p["conv_b"]).reshape(B, -1)
    for l in range(3):
        op = F.relu(F.linear(op, p["fc_w"][l], p["fc_b"][l]))
        op = op * train_oracle.dropout_mask(seed, l, tuple(op.shape))
    desc_r = op.detach()
    cons = F.linear(op, p["fc_w"][3], p["fc_b"][3]).view(n, k, -1).mean(1)
    loss = F.cross_entropy(cons, labels)
    ora.opt.zero_grad()
    loss.backward()
    ora.opt.step()
    loss_r, corr_r = float(loss.detach()), int((cons.argmax(1) == labels).sum())

    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    stats, desc = m.train_step_consensus(x.cuda(), labels.cuda(), k, lr, mu, seed)
    stats = stats.cpu()
    print("consensus loss %.6f (autograd %.6f), hits %d (%d)" % (float(stats[0]), loss_r, int(stats[1]), corr_r))
    assert abs(float(stats[0]) - loss_r) < 2e-4 * max(1.0, abs(loss_r)), (float(stats[0]), loss_r)
    assert int(stats[1]) == corr_r
    assert tuple(desc.shape) == (B, 256) and _relerr(desc.cpu(), desc_r) < 1e-3
    got, ref = m.export_state(), ora.weights()
    gotm, refm = m.export_state(momentum=True), ora.momentum()
    worst, rms = [], []
    for key in ("conv_w", "conv_b", "fc_w", "fc_b"):
        for i, (g, r, o, gm, rm) in enumerate(zip(got[key], ref[key], w[key], gotm[key], refm[key])):
            e_upd, e_mom, e_rms = _relerr(g.cpu() - o, r - o), _relerr(gm.cpu(), rm), _rmserr(g.cpu() - o, r - o)
            worst.append((max(e_upd, e_mom), key, i))
            rms.append((e_rms, key, i))
            print("%-6s %2d: update err %.2e (rms %.2e)  momentum err %.2e" % (key, i, e_upd, e_rms, e_mom))
    assert max(worst)[0] < TOL_UPDATE, max(worst)
    assert max(rms)[0] < TOL_UPDATE, max(rms)
    tight = [e for e, key, i in worst if key.startswith("fc")]
    assert max(tight) < 5e-4, max(tight)
    # bad arguments; labels on the device outside [0, C) give a NaN loss as the plain step does
    xs = x[:6].cuda()
    with pytest.raises(ValueError, match="out of bounds"):
        m.train_step_consensus(xs, torch.tensor([1, 101]), 3, lr, mu, 0)
    for bad_k, bad_y in ((4, torch.tensor([1])), (0, torch.tensor([1])), (3, torch.tensor([1, 2, 3])), (3, [1, 2])):
        with pytest.raises(ValueError):
            m.train_step_consensus(xs, bad_y, bad_k, lr, mu, 0)
    st, _ = m.train_step_consensus(xs, torch.tensor([1, 101]).cuda(), 3, lr, mu, 0)
    assert torch.isnan(st.cpu()[0])
    m.close()


# ---- train_videos ----

def _videos():
    vids = [_synthetic_video(25, 240, 320, seed=61), _synthetic_video(37, 240, 320, seed=63)]
    starts = [[0, 3, 14], [2, 13, 26]]  # windows that overlap (0 and 3), the last possible starts (14 of 24, 26 of 36 pairs)
    return vids, starts


def _full_table(crops, first, L):
    """The flow table written out by hand: row i*2L + c = plane 2*first[i] + c through crop i."""
    rows = []
    for i, cr in enumerate(crops.tolist()):
        for c in range(2 * L):
            rows.append([2 * first[i] + c] + cr)
    return np.array(rows, dtype=np.int64)


def _assert_streams_equal(out, pipe, other, xs, xt, labels, k, lr, mu, seed):
    """out: pipe.train_videos' result; other: a pipeline in the initial state whose models take the same step on xs / xt."""
    for name, model, mine, x in (("s", other.spatial, pipe.spatial, xs), ("t", other.temporal, pipe.temporal, xt)):
        if x is None:
            continue
        stats, desc = model.train_step_consensus(torch.from_numpy(x).cuda(), labels, k, lr, mu, seed)
        torch.cuda.synchronize()
        assert torch.isfinite(stats).all()
        assert torch.equal(out["stats_" + name], stats), (name, out["stats_" + name], stats)
        assert torch.equal(out["desc_" + name], desc), name
        assert all(torch.equal(a, b) for a, b in zip(_state(mine), _state(model))), name


@pytest.mark.parametrize("invert", [False, True])
def test_train_videos_is_tvl1_then_the_gathers_then_the_consensus_step(oracle_tvl1, invert):
    from video_analytics_amd import _ffi, augment, pipeline
    from video_analytics_amd.video import segmentPlan
    L, k, lr, mu, seed = 10, 3, 1e-4, 0.9, 5
    vids, starts = _videos()
    dev = [(r.cuda(), g.cuda()) for r, g in vids]
    crops = augment.draw_scale_jitter_crops(6, 240, 320, random.Random(3))
    crops[1] = torch.tensor([10, 50, 224, 224, 1], dtype=torch.int32)  # one snippet at the network's own size
    labels = torch.tensor([5, 77])
    params = _ffi.default_tvl1_params(**SCHEDULE)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    other = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    before = [t.cpu() for t in pipe.temporal.export_state()["conv_w"]]
    out = pipe.train_videos(dev, labels, k=k, starts=starts, crops=crops, lr=lr, momentum=mu, dropout_seed=seed,
                            invert_flow_x=invert)
    torch.cuda.synchronize()
    assert out["starts"] == starts and torch.equal(out["crops"], crops)
    # the planned flow: the oracle's TV-L1 of exactly those pairs, each once
    full, planned, first, base = [], [], [], 0
    for (rgb, gray), st in zip(vids, starts):
        plan = segmentPlan(gray.shape[0], st, L)
        fl = oracle_tvl1.tvl1_flow(gray.numpy()[None], oracle_tvl1.default_params(**SCHEDULE), nthreads=0)  # [T-1,2,H,W]
        planned.append(fl[plan.pairs])
        first += [base + s for s in st]
        base += fl.shape[0]
        full.append(fl)
    planned = np.concatenate(planned)
    assert planned.shape[0] == 23 + 30  # video 0: pairs 0..12 and 14..23; video 1: three disjoint windows
    assert tuple(out["flow"].shape) == planned.shape and np.array_equal(out["flow"].cpu().numpy(), planned)
    # both inputs from the restatement, on the full flow of both videos and with a table written out by hand
    xt = s17_flow_stack(np.concatenate(full), _full_table(crops, first, L), invert).reshape(6, 2 * L, 224, 224)
    frames = np.stack([vids[v][0].numpy()[s] for v in range(2) for s in starts[v]])
    xs = s17_images_u8(frames, np.array([[i] + cr for i, cr in enumerate(crops.tolist())]))
    _assert_streams_equal(out, pipe, other, xs, xt, labels, k, lr, mu, seed)
    assert any(not torch.equal(a.cpu(), b) for a, b in zip(pipe.temporal.export_state()["conv_w"], before))  # the weights moved
    # drawn starts and crops: one seeded generator replays them; later forwards see the updated weights
    a = pipe.train_videos(dev, labels, k=k, lr=lr, rng=random.Random(9))
    rng = random.Random(9)
    from video_analytics_amd.video import segmentStarts
    assert a["starts"] == [segmentStarts(g.shape[0], k, L, rng) for _, g in vids]
    assert torch.equal(a["crops"], augment.draw_scale_jitter_crops(6, 240, 320, rng))
    assert torch.isfinite(a["stats_s"]).all() and torch.isfinite(a["stats_t"]).all()
    pipe.close()
    other.close()


@pytest.mark.parametrize("motion,mean_flow", [("stack", True), ("trajectory", True), ("bidirectional", False)])
def test_train_videos_applies_the_pipelines_motion(motion, mean_flow):
    """The temporal stream's step under the other motion inputs (S11-S13), against the same pieces called one by one: the
    motion field of every snippet window, then the restatement of the gather."""
    from video_analytics_amd import _ffi, augment, pipeline
    from video_analytics_amd import flow as vflow
    L, k, lr, mu, seed = 10, 3, 1e-4, 0.9, 6
    vids, starts = _videos()
    dev = [(r.cuda(), g.cuda()) for r, g in vids]
    crops = augment.draw_scale_jitter_crops(6, 240, 320, random.Random(4))
    labels = torch.tensor([9, 3])
    params = _ffi.default_tvl1_params(**SCHEDULE)
    kw = dict(device=0, tvl1_params=params, motion=motion, mean_flow=mean_flow)
    pipe, other = pipeline.TwoStreamPipeline(**kw), pipeline.TwoStreamPipeline(**kw)
    out = pipe.train_videos(dev, labels, k=k, starts=starts, crops=crops, lr=lr, momentum=mu, dropout_seed=seed)
    wins = torch.cat([g[s:s + L + 1][None] for (_, g), st in zip(dev, starts) for s in st])  # [6,L+1,H,W]
    tv = vflow.bidirectional_sequences(wins) if motion == "bidirectional" else wins
    fl = vflow.apply_motion(vflow.tvl1_flow(tv, params), L, motion, mean_flow)               # [6*L,2,H,W], per window
    xt = s17_flow_stack(fl.cpu().numpy(), _full_table(crops, [i * L for i in range(6)], L)).reshape(6, 2 * L, 224, 224)
    _assert_streams_equal(out, pipe, other, None, xt, labels, k, lr, mu, seed)
    pipe.close()
    other.close()


def test_train_videos_refuses_bad_arguments_before_anything_is_enqueued(monkeypatch):
    from video_analytics_amd import _ffi, augment, pipeline
    from video_analytics_amd import flow as vflow
    pipe = pipeline.TwoStreamPipeline(device=0)
    half = pipeline.TwoStreamPipeline(device=0, cnn_dtype="bf16")
    rgb = torch.zeros(25, 3, 240, 320, dtype=torch.uint8, device="cuda")
    gray = torch.zeros(25, 240, 320, dtype=torch.uint8, device="cuda")
    crops = augment.draw_scale_jitter_crops(6, 240, 320, random.Random(1))
    torch.cuda.synchronize()

    def boom(*a, **k):
        raise AssertionError("reached the GPU")
    for mod, name in ((_ffi, "ctx"), (_ffi, "lib"), (vflow, "tvl1_flow"), (vflow, "tvl1_flow_concurrent"),
                      (vflow, "resize_flow_to_stack"), (augment, "resize_images"), (augment, "crops_to_device")):
        monkeypatch.setattr(mod, name, boom)
    good = dict(videos=[(rgb, gray), (rgb, gray)], labels=[1, 2], k=3, starts=[[0, 3, 14], [0, 7, 14]], crops=crops)
    with pytest.raises(AssertionError, match="reached the GPU"):
        pipe.train_videos(**good)  # a good call passes every host check
    with pytest.raises(ValueError, match="fp32"):
        half.train_videos(**good)
    bad_crops = crops.clone()
    bad_crops[2, 1] = 320 - int(bad_crops[2, 3]) + 1  # the rectangle leaves the frame on the right
    cases = dict(
        too_many=dict(videos=[(rgb, gray)] * 22, labels=[0] * 22, starts=None, crops=None),
        short=dict(videos=[(rgb[:10], gray[:10])] * 2, starts=None),
        start_out=dict(starts=[[0, 3, 15], [0, 7, 14]]),
        start_count=dict(starts=[[0, 3], [0, 7, 14]]),
        starts_videos=dict(starts=[[0, 3, 14]]),
        crops_rect=dict(crops=bad_crops),
        crops_shape=dict(crops=crops[:5]),
        crops_dtype=dict(crops=crops.long()),
        crops_device=dict(crops=crops.cuda()),
        labels_count=dict(labels=[1]),
        label_range=dict(labels=[1, 101]),
        host=dict(videos=[(rgb.cpu(), gray.cpu())] * 2),
        sizes=dict(videos=[(rgb, gray), (rgb[:, :, :224], gray[:, :224])]),
        rgb_gray=dict(videos=[(rgb[:, :, :224], gray)] * 2),
        frames=dict(videos=[(rgb, gray[:-1])] * 2),
        rgb_dtype=dict(videos=[(rgb.float(), gray)] * 2),
        k_zero=dict(k=0, starts=None),
        no_videos=dict(videos=[], labels=[]),
    )
    for name, kw in cases.items():
        with pytest.raises(ValueError):
            pipe.train_videos(**dict(good, **kw))
            pytest.fail(name)
    monkeypatch.undo()
    pipe.close()
    half.close()
