"""Brox optical flow on the GPU, bit for bit against the float32 oracle (tests/brox_oracle.py): the inner
step alone (``va_brox_inner_step``) under every kernel shape, ``brox_flow`` end to end and through every entry point that
takes ``tvl1_params``.  No test depends on the default parameters."""
import ctypes

import numpy as np
import pytest
import torch

import brox_oracle as bo

pytestmark = pytest.mark.gpu

BASE = dict(alpha=0.197, gamma=50.0, scale_step=0.8, omega=1.9, epsilon=1e-3, nscales=16)
E2E = dict(BASE, warps=2, inner_iters=2, solver_iters=3)

# kernel shapes the result must not depend on: the library's choice (whole field where it fits), whole field off with the
# default tile, the smallest legal tile with K = 1, K = solver_iters on a tile with neither side a divisor of anything, and
# a K between the two (two launches of 2 + 1 sweeps)
TUNINGS = [dict(), dict(whole_field=0), dict(whole_field=0, tile_w=2, tile_h=2, sweeps_per_launch=1),
           dict(whole_field=0, tile_w=23, tile_h=11, sweeps_per_launch=3), dict(whole_field=0, tile_w=40, tile_h=64, sweeps_per_launch=2)]


def _fields(n, w, h):
    """n sets of the fields an inner step reads, with the magnitudes a [0,1] image pair gives them"""
    rs = np.random.RandomState(100 * w + h)
    g = lambda s: (rs.standard_normal((n, h, w)) * s).astype(np.float32)
    f = dict(Ix=g(0.05), Iy=g(0.05), Ixx=g(0.02), Ixy=g(0.02), Iyy=g(0.02), Iz=g(0.05), Ixz=g(0.02), Iyz=g(0.02))
    return f, g(1.5), g(1.5), g(0.2), g(0.2)


_step_ref = {}


def _inner_reference(w, h):
    """the oracle's inner step on the fields of (w, h): computed once, shared by the tunings, never changed"""
    if (w, h) not in _step_ref:
        f, u, v, du, dv = _fields(3, w, h)
        p = bo.params(**dict(BASE, warps=1, inner_iters=1, solver_iters=3))
        ref = [bo.inner_step({k: a[i] for k, a in f.items()}, u[i], v[i], du[i], dv[i], p) for i in range(3)]
        _step_ref[(w, h)] = (f, u, v, du, dv, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]))
    return _step_ref[(w, h)]


@pytest.mark.parametrize("tuning", TUNINGS, ids=["default", "tiled", "tile2x2_K1", "tile23x11_K3", "tile40x64_K2"])
@pytest.mark.parametrize("w,h", [(17, 16), (67, 45), (150, 131)])
def test_inner_step_is_the_oracle_under_every_kernel_shape(w, h, tuning):
    """17 x 16: the smallest S1 level, odd width; 67 x 45: whole field, neither side a multiple of anything; 150 x 131: above
    the whole-field limit, several tiles and partial last tiles.  Three fields per call: a wrong field stride shows."""
    from video_analytics_amd import _ffi
    f, u, v, du, dv, rdu, rdv = _inner_reference(w, h)
    p = _ffi.default_brox_params(**dict(BASE, warps=1, inner_iters=1, solver_iters=3, **tuning))
    dev = {k: torch.from_numpy(a).cuda() for k, a in f.items()}
    du_d, dv_d = torch.from_numpy(du).cuda(), torch.from_numpy(dv).cuda()
    u_d, v_d = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
    scratch = torch.full((4 * 3 * w * h,), float("nan"), dtype=torch.float32, device="cuda")
    unused = torch.zeros((3, h, w), dtype=torch.float32, device="cuda")
    ptr = _ffi.ptr
    _ffi.check(_ffi.lib().va_brox_inner_step(
        _ffi.ctx(0), ptr(unused), ptr(unused), ptr(unused), ptr(dev["Ix"]), ptr(dev["Iy"]), ptr(dev["Ixx"]), ptr(dev["Ixy"]),
        ptr(dev["Iyy"]), ptr(dev["Iz"]), ptr(dev["Ixz"]), ptr(dev["Iyz"]), ptr(u_d), ptr(v_d), ptr(du_d), ptr(dv_d), 3, w, h,
        ctypes.byref(p), ptr(scratch), scratch.numel() * 4, _ffi.stream_ptr(du_d.device)))
    torch.cuda.synchronize()
    assert torch.equal(du_d.cpu(), torch.from_numpy(rdu)) and torch.equal(dv_d.cpu(), torch.from_numpy(rdv))
    assert torch.equal(u_d.cpu(), torch.from_numpy(u)) and torch.equal(dev["Iz"].cpu(), torch.from_numpy(f["Iz"]))  # inputs untouched


@pytest.mark.parametrize("w,h,tuning", [(73, 73, dict()), (160, 190, dict(whole_field=0, tile_w=62, tile_h=62, sweeps_per_launch=3))],
                         ids=["whole73x73", "region78x78"])
def test_inner_step_with_the_largest_regions(w, h, tuning):
    """The three-pairs-per-lane instantiation and more than 64 KB of LDS, which no shape above reaches: the largest level
    of the 224 x 224 pyramid that runs whole (37 x 73 = 2701 pixel pairs), and tiles whose regions are the largest legal
    ones (62 + 2 * 8 = 78 a side, 3042 pairs)."""
    test_inner_step_is_the_oracle_under_every_kernel_shape(w, h, tuning)


def _frames(kind):
    from video_analytics_amd import synth
    if kind == "u8":  # [2,3,45,67] uint8
        _, gray, _ = synth.synth_clips(2, seed=3, H=45, W=67, n_gray=3)
        return gray
    _, gray, _ = synth.synth_clips(1, seed=4, H=131, W=150, n_gray=2)  # [1,2,131,150] float32, not whole numbers
    return gray.float() * 0.97 + 1.25


_flow_ref = {}


def _flow_reference(kind):
    if kind not in _flow_ref:
        fr = _frames(kind)
        _flow_ref[kind] = (fr, torch.from_numpy(bo.brox_flow(fr.numpy(), bo.params(**E2E))))
    return _flow_ref[kind]


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_brox_flow_is_the_oracle_through_every_entry(kind):
    """all the levels S1 gives (5 and 10), two warps: ``brox_flow``, ``tvl1_flow`` and ``tvl1_flow_concurrent`` handed the
    BroxParams, ``out=``, a workspace that TV-L1 and an earlier call left dirty, and a tiled kernel shape"""
    from video_analytics_amd import _ffi, flow as vflow
    fr, ref = _flow_reference(kind)
    d = fr.cuda()
    p = _ffi.default_brox_params(**E2E)
    assert len(vflow.pyramid_sizes(fr.shape[3], fr.shape[2], p)) == (5 if kind == "u8" else 10)
    got = vflow.brox_flow(d, p)
    assert got.shape == ref.shape and torch.equal(got.cpu(), ref)
    assert torch.equal(vflow.brox_flow(d, **E2E).cpu(), ref)  # keyword form
    vflow.tvl1_flow(d, epsilon=0.0, iters=5, warps=1)  # TV-L1 through the same workspace slot
    vflow._ws_cache[(0, "tvl1", 0)].fill_(255)  # NaN bit patterns everywhere
    assert torch.equal(vflow.tvl1_flow(d, p).cpu(), ref)
    out = torch.full(tuple(ref.shape), float("nan"), dtype=torch.float32, device="cuda")
    assert vflow.brox_flow(d, p, out=out) is out and torch.equal(out.cpu(), ref)
    assert torch.equal(vflow.tvl1_flow_concurrent(d, p, n_streams=2).cpu(), ref)
    tiled = _ffi.default_brox_params(**dict(E2E, whole_field=0, tile_w=32, tile_h=24, sweeps_per_launch=2))
    assert torch.equal(vflow.brox_flow(d, tiled).cpu(), ref)


def test_brox_params_reach_the_flow_volumes_and_the_stored_flow():
    from video_analytics_amd import _ffi, flow as vflow, pipeline, synth, temporalModel
    _, gray, _ = synth.synth_clips(2, seed=0)
    gray = gray.cuda()
    p = _ffi.default_brox_params(**dict(BASE, warps=1, inner_iters=1, solver_iters=2, nscales=3))
    vol = temporalModel.flowVolumesFromFrames(gray, tvl1_params=p)
    want = vflow.flow_to_stack(vflow.brox_flow(gray, p)).view(2, 20, 224, 224)
    assert vol.shape == want.shape and torch.equal(vol, want)
    assert not torch.equal(vol, temporalModel.flowVolumesFromFrames(gray, tvl1_params=_ffi.default_tvl1_params(epsilon=0.0, iters=5, warps=1)))
    _, video, _ = synth.synth_clips(1, seed=7, H=48, W=64, n_gray=5)
    video = video[0].cuda()
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=p)
    try:
        store = pipe.extract_flow(video, dtype=torch.float32)
        pairs = torch.stack([video[:-1], video[1:]], dim=1)  # [4,2,48,64]: every consecutive pair on its own
        assert torch.equal(store, vflow.brox_flow(pairs, p))
    finally:
        pipe.close()


def test_what_brox_flow_does_not_have_is_refused_by_name():
    from video_analytics_amd import _ffi, flow as vflow
    p = _ffi.default_brox_params(**E2E)
    d = torch.zeros((1, 2, 32, 32), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="tile_plan"):
        vflow.tile_plan(224, 224, p)
    with pytest.raises(ValueError, match="median"):
        vflow.tvl1_flow(d, p, median=5)
    with pytest.raises(ValueError, match="median"):
        vflow.brox_flow(d, p, median_every=3)
    p.median = 3
    with pytest.raises(ValueError, match="median"):
        vflow.tvl1_flow(d, p)
    with pytest.raises(ValueError, match="omega"):
        vflow.brox_flow(d, omega=2.0)
    with pytest.raises(ValueError, match="profile_levels"):
        vflow.profile_levels(_ffi.default_brox_params(**E2E))
