"""Farneback optical flow on the GPU, bit for bit against the float32 oracle (tests/farneback_oracle.py):
the polynomial expansion alone (``va_farneback_polyexp``) and one pass alone (``va_farneback_pass``) under every tile shape,
``farneback_flow`` end to end and through every entry point that takes ``tvl1_params``.  No test depends on the default
parameters."""
import ctypes

import numpy as np
import pytest
import torch

import farneback_oracle as fo

pytestmark = pytest.mark.gpu

BASE = dict(pyr_scale=0.5, poly_sigma=1.2, levels=3, winsize=15, iterations=2, poly_n=5, gaussian=0)

# tile shapes the result must not depend on: the library's own, one narrower than 2 poly_n + 1 in both directions, one with
# neither side a divisor of anything, one wider than the small fields
POLY_TILES = [dict(), dict(poly_tile_w=8, poly_tile_h=4), dict(poly_tile_w=23, poly_tile_h=11), dict(poly_tile_w=96, poly_tile_h=8)]
PASS_TILES = [dict(), dict(pass_tile_w=8, pass_tile_h=4), dict(pass_tile_w=23, pass_tile_h=11), dict(pass_tile_w=64, pass_tile_h=16)]
TILE_IDS = ["default", "8x4", "23x11", "wide"]


def _texture(n, w, h, seed):
    """n smooth random fields in [0,255], float32, not whole numbers"""
    from video_analytics_amd import synth
    t = torch.from_numpy(np.random.RandomState(seed).rand(n, 1, h, w).astype(np.float32))
    t = synth._blur(t, 1.0)[:, 0]
    t = (t - t.amin()) / (t.amax() - t.amin()) * 255.0
    return t.numpy().astype(np.float32)


_poly_ref = {}


def _poly_reference(n, w, h, poly_n):
    """the oracle's expansion of the fields of (n, w, h): computed once, shared by the tile shapes, never changed"""
    key = (n, w, h, poly_n)
    if key not in _poly_ref:
        f = _texture(n, w, h, 100 * w + h)
        p = fo.params(**dict(BASE, poly_n=poly_n, poly_sigma=1.2 if poly_n == 5 else 1.5))
        _poly_ref[key] = (f, np.stack([fo.polyexp(f[i], p) for i in range(n)]))
    return _poly_ref[key]


@pytest.mark.parametrize("tiles", POLY_TILES, ids=TILE_IDS)
@pytest.mark.parametrize("poly_n", [5, 7])
@pytest.mark.parametrize("n,w,h", [(3, 83, 67), (1, 16, 16)])
def test_polyexp_is_the_oracle_under_every_tile_shape(n, w, h, poly_n, tiles):
    """83 x 67: ragged tiles and clamped borders on all four sides, three fields (a wrong field stride shows); 16 x 16: the
    smallest field, narrower than the default tile"""
    from video_analytics_amd import _ffi
    f, ref = _poly_reference(n, w, h, poly_n)
    p = _ffi.default_farneback_params(**dict(BASE, poly_n=poly_n, poly_sigma=1.2 if poly_n == 5 else 1.5, **tiles))
    d = torch.from_numpy(f).cuda()
    out = torch.full((n, 5, h, w), float("nan"), dtype=torch.float32, device="cuda")
    _ffi.check(_ffi.lib().va_farneback_polyexp(_ffi.ctx(0), _ffi.ptr(d), n, w, h, ctypes.byref(p), _ffi.ptr(out), _ffi.stream_ptr(d.device)))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(ref))
    assert torch.equal(d.cpu(), torch.from_numpy(f))  # input untouched


def _incoming(kind, n, w, h):
    rs = np.random.RandomState(7 * w + h)
    if kind == "zero":
        return np.zeros((n, 2, h, w), dtype=np.float32)
    if kind == "inside":  # every vector lands at least one pixel inside the frame
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
        tx = (rs.rand(n, h, w) * (w - 3) + 1).astype(np.float32)
        ty = (rs.rand(n, h, w) * (h - 3) + 1).astype(np.float32)
        return np.stack([tx - xs, ty - ys], axis=1).astype(np.float32)
    return ((rs.rand(n, 2, h, w) * 2 - 1) * 40).astype(np.float32)  # +-40 px: leaves the frame on each side


_pass_ref = {}


def _pass_reference(w, h, winsize, gaussian, kind):
    """planes the oracle produced, an incoming flow, and the oracle's pass on them: computed once per case"""
    key = (w, h, winsize, gaussian, kind)
    if key not in _pass_ref:
        n = 2
        p = fo.params(**dict(BASE, winsize=winsize, gaussian=gaussian))
        f = _texture(2 * n, w, h, 3 * w + h)
        r = np.stack([fo.polyexp(f[i], p) for i in range(2 * n)])
        r0, r1 = np.ascontiguousarray(r[:n]), np.ascontiguousarray(r[n:])
        fl = _incoming(kind, n, w, h)
        ref = np.stack([np.stack(fo.one_pass(r0[i], r1[i], fl[i, 0], fl[i, 1], p)) for i in range(n)]).astype(np.float32)
        _pass_ref[key] = (r0, r1, fl, ref)
    return _pass_ref[key]


@pytest.mark.parametrize("tiles", PASS_TILES, ids=TILE_IDS)
@pytest.mark.parametrize("kind", ["zero", "inside", "leaving"])
@pytest.mark.parametrize("gaussian", [0, 1])
@pytest.mark.parametrize("w,h,winsize", [(83, 67, 15), (20, 16, 31)])
def test_one_pass_is_the_oracle_under_every_tile_shape(w, h, winsize, gaussian, kind, tiles):
    """83 x 67 with winsize 15: several ragged tiles; 20 x 16 with winsize 31: a window wider than the field, every tap
    clamps.  Incoming flow of zero, with every vector inside the frame, and of +-40 px (the rule of S65 for positions that
    leave the frame, on each side)."""
    from video_analytics_amd import _ffi
    r0, r1, fl, ref = _pass_reference(w, h, winsize, gaussian, kind)
    if kind == "leaving":
        assert (fl[:, 0] + np.arange(w) < 0).any() and (fl[:, 0] + np.arange(w) > w).any()
        assert (fl[:, 1] + np.arange(h)[:, None] < 0).any() and (fl[:, 1] + np.arange(h)[:, None] > h).any()
    p = _ffi.default_farneback_params(**dict(BASE, winsize=winsize, gaussian=gaussian, **tiles))
    d0, d1, din = (torch.from_numpy(a).cuda() for a in (r0, r1, fl))
    out = torch.full(tuple(fl.shape), float("nan"), dtype=torch.float32, device="cuda")
    _ffi.check(_ffi.lib().va_farneback_pass(_ffi.ctx(0), _ffi.ptr(d0), _ffi.ptr(d1), _ffi.ptr(din), _ffi.ptr(out), fl.shape[0], w, h,
                                            ctypes.byref(p), _ffi.stream_ptr(out.device)))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(ref))
    assert torch.equal(din.cpu(), torch.from_numpy(fl)) and torch.equal(d1.cpu(), torch.from_numpy(r1))  # inputs untouched


def _frames(kind):
    from video_analytics_amd import synth
    if kind == "80x64":  # [2,3,64,80] uint8: three levels
        _, gray, _ = synth.synth_clips(2, seed=3, H=64, W=80, n_gray=3)
        return gray
    _, gray, _ = synth.synth_clips(2, seed=4, H=67, W=83, n_gray=3)  # [2,3,67,83]: rows of 83 in a pitch of 84
    if kind == "83x67u8":
        return gray
    return gray.float() * 0.97 + 1.25  # float32, not whole numbers


_flow_ref = {}


def _flow_reference(kind):
    if kind not in _flow_ref:
        fr = _frames(kind)
        _flow_ref[kind] = (fr, torch.from_numpy(fo.farneback_flow(fr.numpy(), fo.params(**BASE))))
    return _flow_ref[kind]


@pytest.mark.parametrize("kind", ["80x64", "83x67", "83x67u8"])
def test_farneback_flow_is_the_oracle_through_every_entry(kind):
    """2 sequences of 3 frames, iterations 2: ``farneback_flow``, its keyword form, ``tvl1_flow`` and ``tvl1_flow_concurrent``
    handed the FarnebackParams, ``out=``, a workspace slot that a TV-L1 call and a Brox call left dirty, and a second tile
    shape"""
    from video_analytics_amd import _ffi, flow as vflow
    fr, ref = _flow_reference(kind)
    d = fr.cuda()
    p = _ffi.default_farneback_params(**BASE)
    assert len(vflow.pyramid_sizes(fr.shape[3], fr.shape[2], p)) == 3
    got = vflow.farneback_flow(d, p)
    assert got.shape == ref.shape and torch.equal(got.cpu(), ref)
    assert torch.equal(vflow.farneback_flow(d, **BASE).cpu(), ref)  # keyword form
    vflow.tvl1_flow(d, epsilon=0.0, iters=5, warps=1)  # TV-L1 and Brox through the same workspace slot
    vflow.brox_flow(d, warps=1, inner_iters=1, solver_iters=2, nscales=3)
    vflow._ws_cache[(0, "tvl1", 0)].fill_(255)  # NaN bit patterns everywhere
    assert torch.equal(vflow.tvl1_flow(d, p).cpu(), ref)
    out = torch.full(tuple(ref.shape), float("nan"), dtype=torch.float32, device="cuda")
    assert vflow.farneback_flow(d, p, out=out) is out and torch.equal(out.cpu(), ref)
    assert torch.equal(vflow.tvl1_flow_concurrent(d, p, n_streams=2).cpu(), ref)
    tiled = _ffi.default_farneback_params(**dict(BASE, poly_tile_w=23, poly_tile_h=11, pass_tile_w=24, pass_tile_h=40))
    assert torch.equal(vflow.farneback_flow(d, tiled).cpu(), ref)


def test_farneback_params_reach_the_consumers():
    from video_analytics_amd import _ffi, flow as vflow, pipeline, synth, temporalModel
    _, gray, _ = synth.synth_clips(2, seed=0)
    gray = gray.cuda()
    p = _ffi.default_farneback_params(**dict(BASE, levels=2, iterations=1))
    want_flow = vflow.farneback_flow(gray, p)
    want = vflow.flow_to_stack(want_flow).view(2, 20, 224, 224)
    vol = temporalModel.flowVolumesFromFrames(gray, tvl1_params=p)
    assert vol.shape == want.shape and torch.equal(vol, want)
    assert not torch.equal(vol, temporalModel.flowVolumesFromFrames(gray, tvl1_params=_ffi.default_tvl1_params(epsilon=0.0, iters=5, warps=1)))
    # rerun_camera's second pass
    field, H, _ = vflow.rerun_camera(gray, want_flow, p)
    assert torch.equal(field, vflow.farneback_flow(vflow.warp_pairs(gray, H), p))
    _, video, _ = synth.synth_clips(1, seed=7, H=48, W=64, n_gray=5)
    video = video[0].cuda()
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=p)
    try:
        store = pipe.extract_flow(video, dtype=torch.float32)
        pairs = torch.stack([video[:-1], video[1:]], dim=1)  # [4,2,48,64]: every consecutive pair on its own
        assert torch.equal(store, vflow.farneback_flow(pairs, p))
    finally:
        pipe.close()


def test_farneback_params_reach_run_batch():
    """2 clips of 224 x 224 with levels 2, iterations 1: the temporal network's input is ``flow_to_stack`` of
    ``farneback_flow``"""
    from video_analytics_amd import _ffi, flow as vflow, pipeline, synth
    rgb, gray, _ = synth.synth_clips(2, seed=1)
    p = _ffi.default_farneback_params(**dict(BASE, levels=2, iterations=1))
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=p)
    try:
        seen = {}
        model = pipe.temporal
        forward = model.forward

        def spy(x, *a, **k):
            seen["x"] = x.detach().clone()
            return forward(x, *a, **k)

        model.forward = spy
        pipe.run_batch(rgb.cuda(), gray.cuda())
        torch.cuda.synchronize()
        model.forward = forward
        want = vflow.flow_to_stack(vflow.farneback_flow(gray.cuda(), p)).view(2, 20, 224, 224)
        assert torch.equal(seen["x"].view(2, 20, 224, 224), want)
    finally:
        pipe.close()


def test_what_farneback_flow_does_not_have_is_refused_by_name():
    from video_analytics_amd import _ffi, flow as vflow
    p = _ffi.default_farneback_params(**BASE)
    d = torch.zeros((1, 2, 32, 32), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="tile_plan"):
        vflow.tile_plan(224, 224, p)
    with pytest.raises(ValueError, match="median"):
        vflow.tvl1_flow(d, p, median=5)
    with pytest.raises(ValueError, match="median"):
        vflow.farneback_flow(d, p, median_every=3)
    p.median = 3
    with pytest.raises(ValueError, match="median"):
        vflow.tvl1_flow(d, p)
    q = _ffi.default_farneback_params(**BASE)
    with pytest.raises(ValueError, match="profile_enable"):
        vflow.profile_enable(q)
    with pytest.raises(ValueError, match="profile_levels"):
        vflow.profile_levels(q)
    with pytest.raises(ValueError, match="profile_read"):
        vflow.profile_read(q)
    with pytest.raises(ValueError, match="poly_n"):
        vflow.farneback_flow(d, poly_n=9)
    with pytest.raises(ValueError, match="winsize"):
        vflow.farneback_flow(d, winsize=14)
