"""The motion inputs on the device: va_flow_field_means and va_flow_motion against the numpy
restatements of tests/test_motion_host.py bit for bit, flowVolumesFromFrames(motion=, mean_flow=) composed with crops,
views and TSN flips against restated S12 -> the oracle's S9 -> numpy gathers, bi-directional flow against the oracle's
TV-L1 of explicitly built sequences, and TwoStreamPipeline(motion=, mean_flow=) against independently built volumes and
the torch-CPU oracle."""
import random

import numpy as np
import pytest
import torch

from test_motion_host import s11_means, s12_motion, smooth_flow

pytestmark = pytest.mark.gpu

KW = dict(epsilon=0.0, iters=28, warps=2)  # the short schedule of the 320x240 oracle comparisons
L = 10
MOTION_CASES = [("stack", True), ("trajectory", False), ("trajectory", True), ("bidirectional", False),
                ("bidirectional", True)]


def _normal12(N, h, w, seed):
    """sigma 12 px: trajectories leave the frame and clamp, the S9 clamps at +-20 are hit."""
    return (np.random.RandomState(seed).standard_normal((N, 2, h, w)) * 12.0).astype(np.float32)


def _unaligned(a):
    """A CUDA copy of a whose data starts 4 bytes past a 16-byte boundary (the kernels' scalar paths)."""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    return t


# ---- S11 ----

@pytest.mark.parametrize("h,w", [(224, 224), (240, 320), (300, 17)])
def test_field_means_equal_the_int64_restatement(h, w):
    from video_analytics_amd import flow as vflow
    fl = _normal12(8, h, w, h + w)
    rs = np.random.RandomState(w)
    for _ in range(40):  # planted values far outside the clamp
        fl[rs.randint(8), rs.randint(2), rs.randint(h), rs.randint(w)] = rs.choice([1e5, -1e5])
    fl[3, 0] = np.float32(-0.7)  # constant planes: the mean is exact
    fl[3, 1] = np.float32(2.0 ** -16 * 3)
    fl[5, 1] = np.float32(5.25)
    ref = s11_means(fl)
    assert ref[5, 1] == np.float32(5.25) and ref[3, 1] == np.float32(2.0 ** -16 * 3)
    got = vflow.flow_field_means(torch.from_numpy(fl).cuda())
    assert tuple(got.shape) == (8, 2) and np.array_equal(got.cpu().numpy(), ref)
    got = vflow.flow_field_means(_unaligned(fl))
    assert np.array_equal(got.cpu().numpy(), ref)


# ---- S12 ----

def _tvl1_synth(B, h, w):
    from video_analytics_amd import _ffi, synth
    from video_analytics_amd import flow as vflow
    _, gray, _ = synth.synth_clips(B, seed=7, H=h, W=w)
    return vflow.tvl1_flow(gray.cuda(), _ffi.default_tvl1_params(**KW)).cpu().numpy()


@pytest.mark.parametrize("source", ["normal12", "smooth", "tvl1"])
@pytest.mark.parametrize("chain_len", [1, 5, 10])
def test_motion_field_equals_the_float32_restatement(source, chain_len):
    from video_analytics_amd import flow as vflow
    h, w = 240, 320
    N = 20
    fl = {"normal12": lambda: _normal12(N, h, w, chain_len),
          "smooth": lambda: smooth_flow(N, h, w, phase=0.25),
          "tvl1": lambda: _tvl1_synth(2, h, w)}[source]()
    d = torch.from_numpy(fl).cuda()
    means = s11_means(fl)
    dm = vflow.flow_field_means(d)
    assert np.array_equal(dm.cpu().numpy(), means)
    for trajectory, with_means in ((True, False), (True, True), (False, True)):
        out = torch.full_like(d, float("nan"))  # every element must be written
        got = vflow.motion_field(d, chain_len, trajectory=trajectory, means=dm if with_means else None, out=out)
        assert got.data_ptr() == out.data_ptr()
        ref = s12_motion(fl, chain_len, trajectory, means if with_means else None)
        g = got.cpu().numpy()
        assert np.array_equal(g, ref), (trajectory, with_means, np.abs(g - ref).max())


@pytest.mark.parametrize("h,w", [(29, 37), (48, 64)])
def test_motion_field_scalar_paths(h, w):
    """Planes of a number of floats that is not a multiple of 4 (29 x 37), and unaligned buffers: the scalar paths."""
    from video_analytics_amd import flow as vflow
    fl = _normal12(15, h, w, h)
    fl[4, 0, 3, 5] = np.float32(1e5)
    means = s11_means(fl)
    d = _unaligned(fl)
    dm = vflow.flow_field_means(d)
    assert np.array_equal(dm.cpu().numpy(), means)
    for trajectory, m in ((True, None), (True, dm), (False, dm)):
        out = _unaligned(np.full(fl.shape, np.nan, dtype=np.float32))
        got = vflow.motion_field(d, 5, trajectory=trajectory, means=m, out=out).cpu().numpy()
        assert np.array_equal(got, s12_motion(fl, 5, trajectory, None if m is None else means)), (trajectory, m is None)


def test_motion_field_refuses_bad_arguments():
    from video_analytics_amd import _ffi
    from video_analytics_amd import flow as vflow
    d = torch.zeros(10, 2, 24, 32, device="cuda")
    m = vflow.flow_field_means(d)
    with pytest.raises(ValueError, match="nothing to do"):
        vflow.motion_field(d, 5)
    with pytest.raises(ValueError, match="overlap"):
        vflow.motion_field(d, 5, trajectory=True, out=d)
    buf = torch.zeros(2 * d.numel(), device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        vflow.motion_field(buf[: d.numel()].view(d.shape), 5, trajectory=True, out=buf[d.numel() // 2:][: d.numel()])
    with pytest.raises(ValueError):
        vflow.motion_field(d, 3, trajectory=True)  # 10 pairs are not clips of 3
    with pytest.raises(ValueError):
        vflow.motion_field(d, 5, means=m[:4])
    lib, c, s = _ffi.lib(), _ffi.ctx(0), _ffi.stream_ptr(0)
    out = torch.empty_like(d)
    p = _ffi.ptr
    assert lib.va_flow_motion(c, p(d), 2, 5, 0, 32, 24, None, p(out), s) == _ffi.VA_ERR_INVALID
    assert b"nothing to do" in lib.va_last_error()
    assert lib.va_flow_motion(c, p(d), 65536, 1, 1, 32, 24, None, p(out), s) == _ffi.VA_ERR_INVALID
    assert lib.va_flow_motion(c, p(d), 2, 5, 2, 32, 24, p(m), p(out), s) == _ffi.VA_ERR_INVALID
    assert lib.va_flow_motion(c, p(d), 2, 0, 1, 32, 24, None, p(out), s) == _ffi.VA_ERR_INVALID
    assert lib.va_flow_field_means(c, p(d), 0, 32, 24, p(m), s) == _ffi.VA_ERR_INVALID
    assert lib.va_flow_field_means(c, p(d), 10, 1 << 16, 1 << 15, p(m), s) == _ffi.VA_ERR_INVALID
    assert lib.va_flow_field_means(c, None, 10, 32, 24, p(m), s) == _ffi.VA_ERR_INVALID
    assert lib.va_version() & 0xffff == 6


# ---- composition with S9 / S10 at 320x240 ----

def _volume(fl, rows, invert, oracle, size=224):
    """numpy reference of S9 then S10: the oracle's S9 volume of the float array fl [N,2,H,W] (flow or motion field),
    plane (o // (V*2L)) * 2L + o % 2L read through row o; with invert, mirrored x planes are 255 - q."""
    from video_analytics_amd import utils
    N, _, H, W = fl.shape
    full = oracle.flow_to_stack(fl)
    inv = ((255 - utils.flowToImages(fl).reshape(2 * N, H, W)).astype(np.float32) / np.float32(255.0)
           - np.float32(0.485)) / np.float32(0.229)
    C = 2 * L
    V = rows.shape[0] // (2 * N)
    out = np.empty((rows.shape[0], size, size), dtype=np.float32)
    for o, (top, left, flip) in enumerate(rows.tolist()):
        b, c = o // (V * C), o % C
        plane = inv[b * C + c] if (invert and flip and c % 2 == 0) else full[b * C + c]
        win = plane[top:top + size, left:left + size]
        out[o] = win[:, ::-1] if flip else win
    return out


def _restated_field(fl, motion, mean_flow):
    if motion != "trajectory" and not mean_flow:
        return fl
    return s12_motion(fl, L, motion == "trajectory", s11_means(fl) if mean_flow else None)


@pytest.fixture(scope="module")
def clips(oracle_tvl1):
    """Three 320x240 clips and the oracle's TV-L1 of their plain and bi-directional sequences (checked against the device
    flow bit for bit)."""
    from video_analytics_amd import _ffi, synth
    from video_analytics_amd import flow as vflow
    B, H, W = 3, 240, 320
    rgb, gray, _ = synth.synth_clips(B, seed=29, H=H, W=W)
    g = gray.numpy()
    p = oracle_tvl1.default_params(**KW)
    plain = oracle_tvl1.tvl1_flow(g, p, nthreads=8)
    seqs = []
    for b in range(B):  # forward (tau ... tau + L/2), then backward (tau ... tau - L/2)
        seqs += [g[b, L // 2:], g[b, L // 2::-1]]
    bidir = oracle_tvl1.tvl1_flow(np.ascontiguousarray(np.stack(seqs)), p, nthreads=8)
    params = _ffi.default_tvl1_params(**KW)
    assert np.array_equal(vflow.tvl1_flow(gray.cuda(), params).cpu().numpy(), plain)
    dev_bidir = vflow.tvl1_flow(vflow.bidirectional_sequences(gray.cuda()), params).cpu().numpy()
    assert np.array_equal(dev_bidir, bidir), "bi-directional flow differs from the oracle's TV-L1 of the sequences"
    assert bidir.shape == plain.shape == (B * L, 2, H, W)
    return dict(rgb=rgb, gray=gray, flow={"stack": plain, "trajectory": plain, "bidirectional": bidir})


@pytest.mark.parametrize("motion,mean_flow", MOTION_CASES)
def test_flow_volumes_compose_with_crops_views_and_flips(clips, oracle_tvl1, motion, mean_flow):
    from video_analytics_amd import _ffi, augment
    from video_analytics_amd.temporalModel import flowVolumesFromFrames
    gray = clips["gray"].cuda()
    B, _, H, W = gray.shape
    field = _restated_field(clips["flow"][motion], motion, mean_flow)
    p = _ffi.default_tvl1_params(**KW)
    kw = dict(tvl1_params=p, motion=motion, mean_flow=mean_flow)
    random.seed(31)
    crops = augment.draw_flow_crops(B, L, H, W)
    for invert in (False, True):
        got = flowVolumesFromFrames(gray, crops=crops, invert_flow_x=invert, **kw)
        assert tuple(got.shape) == (B, 2 * L, 224, 224)
        assert np.array_equal(got.cpu().numpy().reshape(-1, 224, 224), _volume(field, crops, invert, oracle_tvl1)), invert
    views = augment.ten_crop_views(H, W)
    got = flowVolumesFromFrames(gray, views=views, invert_flow_x=True, **kw)
    assert tuple(got.shape) == (B, 10, 2 * L, 224, 224)
    ref = _volume(field, augment.expand_views(views, B, 2 * L), True, oracle_tvl1)
    assert np.array_equal(got.cpu().numpy().reshape(-1, 224, 224), ref)


def test_bidirectional_volume_starts_with_the_plain_stack_from_tau(clips):
    from video_analytics_amd import _ffi, augment
    from video_analytics_amd.temporalModel import flowVolumesFromFrames
    gray = clips["gray"].cuda()
    p = _ffi.default_tvl1_params(**KW)
    views = augment.ten_crop_views(240, 320)
    bi = flowVolumesFromFrames(gray, tvl1_params=p, views=views, motion="bidirectional")
    fwd = flowVolumesFromFrames(gray[:, L // 2:].contiguous(), flowSampleSize=L // 2, tvl1_params=p, views=views)
    assert torch.equal(bi[:, :, :L], fwd)
    assert not torch.equal(bi[:, :, L:], fwd)


# ---- the pipeline ----

@pytest.fixture(scope="module")
def default_pipe():
    from video_analytics_amd import _ffi, pipeline
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(**KW))
    yield pipe
    pipe.close()


@pytest.mark.parametrize("motion", ["stack", "trajectory", "bidirectional"])
def test_pipeline_motion_with_mean_flow(clips, oracle_tvl1, default_pipe, motion):
    from oracle import vgg_oracle
    from video_analytics_amd import _ffi, augment, pipeline, synth
    rgb, gray = clips["rgb"].cuda(), clips["gray"].cuda()
    B, _, H, W = gray.shape
    field = _restated_field(clips["flow"][motion], motion, True)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(**KW), motion=motion, mean_flow=True)
    with pytest.raises(ValueError):
        pipe.submit(rgb, None, flow_stack=torch.zeros(B, 2 * L, 224, 224, device="cuda"))
    assert pipe._n == 0

    # ten views
    views = augment.ten_crop_views(H, W)
    out = pipe.run_batch(rgb, gray, views=(views, views), invert_flow_x=True)
    xt = _volume(field, augment.expand_views(views, B, 2 * L), True, oracle_tvl1).reshape(B, 10, 2 * L, 224, 224)
    dt, lt, dtv, ltv = pipe.temporal.forward_views(torch.from_numpy(xt).cuda())
    base = default_pipe.run_batch(rgb, gray, views=(views, views), invert_flow_x=True)
    torch.cuda.synchronize()
    for key, ref in (("desc_t", dt), ("logits_t", lt), ("desc_t_views", dtv), ("logits_t_views", ltv)):
        assert torch.equal(out[key], ref), key
    for key in ("desc_s", "logits_s", "desc_s_views", "logits_s_views"):
        assert torch.equal(out[key], base[key]), key

    # random crops
    random.seed(37)
    crops = augment.draw_clip_crops(B, L, (H, W), (H, W))
    out_c = pipe.run_batch(rgb, gray, crops=crops)
    xc = _volume(field, crops[1], False, oracle_tvl1).reshape(B, 2 * L, 224, 224)
    _, dc, lc = pipe.temporal.forward(torch.from_numpy(xc).cuda())
    base_c = default_pipe.run_batch(rgb, gray, crops=crops)
    torch.cuda.synchronize()
    assert torch.equal(out_c["desc_t"], dc) and torch.equal(out_c["logits_t"], lc)
    for key in ("desc_s", "logits_s"):
        assert torch.equal(out_c[key], base_c[key]), key

    # the torch-CPU oracle on one view of one clip and one cropped clip
    wt = synth.synth_vgg16_weights(c_in=2 * L, seed=2)
    wt["conv_w"][0] = vgg_oracle.copy_first_layer(wt["conv_w"][0], 2 * L)
    x_ref = torch.from_numpy(np.stack([xt[1, 7], xc[2]]))
    _, _, l_ref = vgg_oracle.forward(x_ref, wt["conv_w"], wt["conv_b"], wt["fc_w"], wt["fc_b"])
    got = torch.stack([out["logits_t_views"][1, 7], out_c["logits_t"][2]]).cpu()
    assert float((got - l_ref).abs().max()) < 1e-3

    # two pipelined submits, the second ragged, equal the unpipelined runs
    random.seed(41)
    crops2 = augment.draw_clip_crops(2, L, (H, W), (H, W))
    single = pipe.run_batch(rgb[:2], gray[:2], crops=crops2)
    single_v = pipe.run_batch(rgb[:2], gray[:2], views=(views, views), invert_flow_x=True)
    a = pipe.submit(rgb, gray, crops=crops)
    b = pipe.submit(rgb[:2], gray[:2], crops=crops2)
    c = pipe.submit(rgb, gray, views=(views, views), invert_flow_x=True)
    d = pipe.submit(rgb[:2], gray[:2], views=(views, views), invert_flow_x=True)
    pipe.wait()
    for k in ("logits_s", "logits_t", "desc_s", "desc_t"):
        assert torch.equal(a[k], out_c[k]) and torch.equal(b[k], single[k]), k
        assert torch.equal(c[k], out[k]) and torch.equal(d[k], single_v[k]), k
    pipe.close()


def test_pipeline_flow_volume_and_option_checks():
    from video_analytics_amd import _ffi, pipeline, synth
    from video_analytics_amd import flow as vflow
    for bad in (dict(motion="optical"), dict(motion="trajectory+bidirectional"), dict(motion="bidirectional", flow_count=9),
                dict(mean_flow=1)):
        with pytest.raises(ValueError):
            pipeline.TwoStreamPipeline(device=0, **bad)
    _, gray, _ = synth.synth_clips(2, seed=3)
    p = _ffi.default_tvl1_params(**KW)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=p, motion="trajectory", mean_flow=True)
    got = pipe.flow_volume(gray.cuda())
    fl = vflow.tvl1_flow(gray.cuda(), p)
    ref = vflow.flow_to_stack(vflow.motion_field(fl, L, trajectory=True, means=vflow.flow_field_means(fl))).view(2, 2 * L, 224, 224)
    assert torch.equal(got, ref)
    pipe.close()
