"""Brox optical flow on the GPU AWAY from the one parameter set of tests/test_brox_gpu.py and AT every number the host code
compares a size with: both sides of the four limits between the kernel instantiations, the last whole field and the first
tiled one, every sweep split, kMaxK, the three-buffer rotation, alpha / gamma / omega / epsilon one at a time, scale steps
whose inverse is not 1.25, and frame content the synthetic clips never produce.

Same bar as tests/test_brox_gpu.py: BIT-EXACT against the float32 oracle (tests/brox_oracle.py) under every kernel shape.
The oracle is pinned to its float64 witness at these parameters in tests/test_brox_host.py.  Every test first asserts that
the oracle's result is finite, so that no NaN can sit on both sides of a comparison, and asserts through
tests/flow_shapes.py that the case reaches the kernel form it is named for.
"""
import ctypes

import numpy as np
import pytest
import torch

import brox_oracle as bo
import flow_shapes as fs
from test_brox_gpu import BASE, E2E, _fields

pytestmark = pytest.mark.gpu

_step_ref = {}


def _inner_reference(w, h, solver_iters, phys):
    """the oracle's inner step on the three fields of (w, h): computed once per parameter set, shared by the tunings"""
    key = (w, h, solver_iters, tuple(sorted(phys.items())))
    if key not in _step_ref:
        f, u, v, du, dv = _fields(3, w, h)
        p = bo.params(**dict(BASE, warps=1, inner_iters=1, solver_iters=solver_iters, **phys))
        ref = [bo.inner_step({k: a[i] for k, a in f.items()}, u[i], v[i], du[i], dv[i], p) for i in range(3)]
        rdu, rdv = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
        assert np.isfinite(rdu).all() and np.isfinite(rdv).all(), "the oracle's step is not finite: %r" % (phys,)
        _step_ref[key] = (f, u, v, du, dv, rdu, rdv)
    return _step_ref[key]


def _check_inner(w, h, solver_iters, tuning, phys=None):
    """``va_brox_inner_step`` on three fields equals the oracle bit for bit; the scratch starts as NaN; inputs stay as they were"""
    from video_analytics_amd import _ffi
    phys = phys or {}
    f, u, v, du, dv, rdu, rdv = _inner_reference(w, h, solver_iters, phys)
    p = _ffi.default_brox_params(**dict(BASE, warps=1, inner_iters=1, nscales=1, solver_iters=solver_iters, **phys, **tuning))
    assert _ffi.lib().va_brox_workspace_bytes(w, h, 1, 2, ctypes.byref(p)) > 0, _ffi.lib().va_last_error()
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
    gdu, gdv = du_d.cpu().numpy(), dv_d.cpu().numpy()
    bad = int((gdu != rdu).sum() + (gdv != rdv).sum())
    assert bad == 0, "%d values differ, max abs diff %g" % (bad, max(np.nanmax(np.abs(gdu - rdu)), np.nanmax(np.abs(gdv - rdv))))
    assert torch.equal(u_d.cpu(), torch.from_numpy(u)) and torch.equal(v_d.cpu(), torch.from_numpy(v))
    for k, a in f.items():
        assert torch.equal(dev[k].cpu(), torch.from_numpy(a)), k  # inputs untouched


# ------------------------------------------------------------------------------------------------ a. instantiation limits

@pytest.mark.parametrize("w,h,solver_iters,pairs,form", fs.BROX_WHOLE_CASES, ids=["%dx%d" % c[:2] for c in fs.BROX_WHOLE_CASES])
def test_inner_step_at_both_sides_of_every_instantiation_limit(w, h, solver_iters, pairs, form):
    """Whole fields of 256 / 272, 1024 / 1025, 2048 / 2079 and 3072 pixel pairs: the last field <256,1>, <256,4> and
    <1024,2> run and the first one their successors run, and the last whole field in three aspect ratios."""
    s = fs.brox_shape(w, h, solver_iters)
    assert s["whole"] and s["pairs"] == pairs and s["form"] == form
    _check_inner(w, h, solver_iters, dict())


@pytest.mark.parametrize("c", fs.BROX_TILED_CASES, ids=["%dx%d" % (c["w"], c["h"]) for c in fs.BROX_TILED_CASES])
def test_inner_step_with_tiles_sized_for_more_than_2048_pairs(c):
    """97 x 64 = 3136 pairs under the default tuning, the first field the library tiles on its own: four tiles of 49 x 32
    with K 5, the launch sized for regions of 73 x 56 = 2072 pairs (three pairs per lane), every region cut by the border.
    150 x 63 in three tiles as high as the field: the middle region is 66 x 63 = 2079 pairs, all of them run, and its last
    row, which holds the pairs past 2048, is a row of the result."""
    assert fs.brox_shape(96, 64, c["solver_iters"])["whole"]
    s = fs.brox_shape(c["w"], c["h"], c["solver_iters"], **c["tuning"])
    assert not s["whole"] and all(s[k] == c[k] for k in ("K", "H", "TW", "TH", "rw", "rh", "pairs", "form")), s
    assert 2048 < s["pairs"] <= 2080 and max(fs._pairs(*r) for r in fs.brox_regions(s, c["w"], c["h"])) == c["runs"]
    _check_inner(c["w"], c["h"], c["solver_iters"], c["tuning"])


# ------------------------------------------------------------------------------------------------ b. sweep split

@pytest.mark.parametrize("w,h", fs.BROX_SPLIT_FIELDS)
@pytest.mark.parametrize("solver_iters,spl,K,launches", fs.BROX_SPLIT_CASES, ids=["%d_by_%d" % c[:2] for c in fs.BROX_SPLIT_CASES])
def test_inner_step_under_every_sweep_split(solver_iters, spl, K, launches, w, h):
    """base + (i < extra) with extra 1 of 3 and 2 of 3, an odd number of launches, K clamped by solver_iters, kMaxK (halo
    36: tiles of 6 x 6, regions of 78 x 78 on 150 x 131) and 40 sweeps as 14 + 13 + 13"""
    s = fs.brox_shape(w, h, solver_iters, whole_field=0, sweeps_per_launch=spl)
    assert not s["whole"] and s["K"] == K and s["launches"] == launches and s["H"] == 2 * K + 2
    if K == fs.BROX_MAX_K:
        assert (s["TW"], s["TH"]) == (6, 6) and s["rw"] == 78 and s["rh"] == min(78, h) and s["form"] == (1024, 3)
    _check_inner(w, h, solver_iters, dict(whole_field=0, sweeps_per_launch=spl))


# ------------------------------------------------------------------------------------------------ c. alpha, gamma, omega, epsilon

# one parameter away from BASE at a time: gradient constancy off and dominant; smoothness weak and dominant; under-relaxation
# (om1 = 1 - omega > 0), Gauss-Seidel (om1 = 0) and the upper end; epsilon^2 at 1e-12 and at 1
PHYS = [dict(gamma=0.0), dict(gamma=200.0), dict(alpha=0.01), dict(alpha=30.0), dict(omega=0.5), dict(omega=1.0), dict(omega=1.99),
        dict(epsilon=1e-6), dict(epsilon=1.0)]


@pytest.mark.parametrize("tuning", [dict(), dict(whole_field=0)], ids=["default", "tiled"])
@pytest.mark.parametrize("w,h", [(67, 45), (150, 131)])
@pytest.mark.parametrize("phys", PHYS, ids=lambda o: ",".join("%s=%g" % kv for kv in o.items()))
def test_inner_step_one_parameter_at_a_time(phys, w, h, tuning):
    assert fs.brox_shape(67, 45, 3)["whole"] and not fs.brox_shape(150, 131, 3)["whole"]
    _check_inner(w, h, 3, tuning, phys)


# ------------------------------------------------------------------------------------------------ d. end to end

TILED = dict(whole_field=0, tile_w=32, tile_h=24, sweeps_per_launch=2)
FLOW_CASES = [dict(scale_step=0.5), dict(scale_step=0.65), dict(scale_step=0.95, nscales=6), dict(nscales=1), dict(nscales=2), dict(warps=3),
              dict(gamma=0.0), dict(omega=1.0)]
# (scale_step, nscales) -> levels of the 67 x 45 pyramid
FLOW_LEVELS = {(0.5, 16): 2, (0.65, 16): 3, (0.95, 6): 6, (0.8, 1): 1, (0.8, 2): 2, (0.8, 16): 5}

_flow_ref = {}


def _frames():
    from video_analytics_amd import synth
    _, gray, _ = synth.synth_clips(2, seed=3, H=45, W=67, n_gray=3)  # [2,3,45,67] uint8
    return gray


def _flow_reference(key, frames, kw):
    """the oracle's flow: computed once per case, shared by the tunings, asserted finite"""
    if key not in _flow_ref:
        ref = bo.brox_flow(frames.numpy(), bo.params(**kw))
        assert np.isfinite(ref).all(), "the oracle's flow is not finite: %r" % (kw,)
        _flow_ref[key] = ref
    return _flow_ref[key]


def _check_flow(frames, ref, kw, tuning):
    from video_analytics_amd import flow as vflow
    d = frames.cuda()
    keep = d.clone()
    out = torch.full(tuple(ref.shape), float("nan"), dtype=torch.float32, device="cuda")
    assert vflow.brox_flow(d, out=out, **kw, **tuning) is out
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, ref), "%r %r: %d values differ, max abs diff %g" % (kw, tuning, int((got != ref).sum()), np.nanmax(np.abs(got - ref)))
    assert torch.equal(d, keep)  # input untouched


@pytest.mark.parametrize("tuning", [dict(), TILED], ids=["default", "tiled"])
@pytest.mark.parametrize("over", FLOW_CASES, ids=lambda o: ",".join("%s=%g" % kv for kv in o.items()))
def test_brox_flow_one_parameter_at_a_time(over, tuning):
    """[2,3,45,67] uint8, four pairs: 1 / scale_step of 2, 1.538... and 1.052..., one and two levels, a third warp, gradient
    constancy off, Gauss-Seidel"""
    from video_analytics_amd import _ffi, flow as vflow
    kw = dict(E2E, **over)
    sizes = vflow.pyramid_sizes(67, 45, _ffi.default_brox_params(**kw))
    assert len(sizes) == FLOW_LEVELS[(kw["scale_step"], kw["nscales"])]
    frames = _frames()
    _check_flow(frames, _flow_reference(tuple(sorted(over.items())), frames, kw), kw, tuning)


@pytest.mark.parametrize("spl,ends", [(1, [1, 2, 0, 1]), (2, [2, 1, 0, 2])], ids=["three_launches", "two_launches"])
def test_brox_flow_follows_the_buffer_rotation(spl, ends):
    """inner_iters 4, solver_iters 3, tiled: three launches per step (sweeps_per_launch 1) and two (2), so that the step's
    result ends in each of the three (du, dv) buffers in turn, and the update reads it from there"""
    kw = dict(E2E, inner_iters=4)
    tuning = dict(TILED, sweeps_per_launch=spl)
    s = fs.brox_shape(67, 45, 3, **tuning)
    assert len(s["launches"]) == 4 - spl and fs.brox_rotation(s, 4) == ends and set(ends) == {0, 1, 2}
    frames = _frames()
    _check_flow(frames, _flow_reference("inner_iters=4", frames, kw), kw, tuning)


@pytest.mark.parametrize("tuning", [dict(), TILED], ids=["default", "tiled"])
@pytest.mark.parametrize("name", fs.CONTENTS)
def test_brox_flow_on_content_the_clips_do_not_produce(name, tuning):
    """three pairs of 67 x 45 each: identical constant frames (the oracle's flow is exactly 0), saturated checkerboards
    moved by one pixel, and magnified textures whose flow leaves the frame on all four sides"""
    frames = torch.from_numpy(fs.content_pairs(name, 45, 67))
    ref = _flow_reference(name, frames, E2E)
    if name == "constant":
        assert np.all(ref == 0.0)
    if name == "leaving":
        assert fs.leaves_on_all_sides(ref)
    _check_flow(frames, ref, E2E, tuning)
