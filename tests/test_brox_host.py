"""Brox optical flow without a GPU: the float32 oracle (tests/brox_oracle.py, the executable form of the
specification) against an independent float64 witness (tests/brox_witness_f64.py) and against known answers, and the host
side of the C ABI (parameter validation, the Python parameter object).  No test depends on the default parameters: every one
names the values it runs with."""
import ctypes

import numpy as np
import pytest
import torch

import brox_oracle as bo
import brox_witness_f64 as bw

# the parameter set of the known-answer tests, spelled out
PAPER = dict(alpha=0.197, gamma=50.0, scale_step=0.8, omega=1.9, epsilon=1e-3, nscales=16, warps=1, inner_iters=3, solver_iters=5)
DISPLACEMENT = (1.5, -0.75)


@pytest.fixture(scope="module")
def synth_pair():
    from video_analytics_amd import synth
    _, gray, _ = synth.synth_clips(1, seed=0, H=40, W=48, n_gray=2)
    return gray[0].numpy()


@pytest.fixture(scope="module")
def planted():
    """A blurred texture of 64 x 48 and the same texture translated by DISPLACEMENT (sampled from a larger one): float32"""
    from video_analytics_amd import synth
    H, W, M = 48, 64, 8
    t = torch.from_numpy(np.random.RandomState(5).rand(1, 1, H + 2 * M, W + 2 * M).astype(np.float32))
    t = synth._blur(t, 2.0)[0, 0].numpy().astype(np.float64)
    t = (t - t.min()) / (t.max() - t.min()) * 255.0
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    f0 = bw.sample(t, xx + M, yy + M)
    f1 = bw.sample(t, xx + M - DISPLACEMENT[0], yy + M - DISPLACEMENT[1])
    return f0.astype(np.float32), f1.astype(np.float32)


def epe(f):
    """mean end-point error against DISPLACEMENT over the interior, 8 px from the border"""
    e = np.sqrt((f[0].astype(np.float64) - DISPLACEMENT[0]) ** 2 + (f[1].astype(np.float64) - DISPLACEMENT[1]) ** 2)
    return float(e[8:-8, 8:-8].mean())


@pytest.fixture(scope="module")
def planted_flows(planted):
    p = bo.params(**PAPER)
    return bo.flow_pair(planted[0], planted[1], p), bw.flow_pair(planted[0], planted[1], p)


def test_identical_frames_give_exactly_zero_flow(synth_pair):
    """b = 0: every sweep leaves du = dv = 0, on every level"""
    f = bo.flow_pair(synth_pair[0], synth_pair[0], bo.params(**dict(PAPER, warps=2)))
    assert f.shape == (2, 40, 48) and f.dtype == np.float32
    assert np.all(f == 0.0)


def test_the_oracle_agrees_with_the_float64_witness(synth_pair):
    """48 x 40 pair of synth.synth_clips, two levels, inner_iters = 2, solver_iters = 5.  The bound is not derivable (the
    drift of float32 through two levels of nonlinear iterations depends on the data).  Measured when the test was written:
    maximum difference 4.15e-5 px, median 6.97e-7 px (the flow reaches 4.0 px); asserted: four times that."""
    p = bo.params(**dict(PAPER, nscales=2, inner_iters=2, solver_iters=5))
    fo, fw = bo.flow_pair(synth_pair[0], synth_pair[1], p), bw.flow_pair(synth_pair[0], synth_pair[1], p)
    d = np.abs(fo.astype(np.float64) - fw)
    print("max %.3e median %.3e" % (d.max(), np.median(d)))
    assert np.abs(fw).max() > 1.0  # the pair moves
    assert d.max() <= 4 * 4.15e-5 and np.median(d) <= 4 * 6.97e-7


# The oracle against the witness away from PAPER, one parameter at a time, on the 48 x 40 pair with two levels: (overrides,
# largest difference in px, median difference in px), measured when the tests were written and printed by the test below.
# None is derivable (see test_the_oracle_agrees_with_the_float64_witness).  gamma 0 and alpha 5 move the flow slowly: with
# inner_iters 2, solver_iters 5 it stays below 0.05 px, so these two run four warps of 4 x 25 sweeps (flow of 2.1 and 2.6 px).
AWAY = [
    (dict(gamma=0.0, warps=4, inner_iters=4, solver_iters=25), 2.315e-6, 4.924e-7),
    (dict(alpha=5.0, warps=4, inner_iters=4, solver_iters=25), 2.747e-6, 3.732e-7),
    (dict(omega=0.5, inner_iters=2, solver_iters=5), 1.823e-6, 3.816e-8),
    (dict(scale_step=0.5, inner_iters=2, solver_iters=5), 3.604e-5, 8.218e-7),
]


@pytest.mark.parametrize("over,dmax,dmed", AWAY, ids=[",".join("%s=%g" % kv for kv in o.items()) for o, _, _ in AWAY])
def test_the_oracle_agrees_with_the_float64_witness_away_from_the_defaults(synth_pair, over, dmax, dmed):
    """Gradient constancy off, under-relaxation (1 - omega > 0), a smoothness weight 25 times the paper's and a scale step
    whose inverse is 2: the settings tests/test_brox_params_gpu.py holds the kernels to the oracle at.  Measured when the
    test was written (maximum / median difference, the witness's largest flow):
        gamma 0          2.315e-6 / 4.924e-7 px, flow up to 2.13 px
        alpha 5          2.747e-6 / 3.732e-7 px, flow up to 2.56 px
        omega 0.5        1.823e-6 / 3.816e-8 px, flow up to 1.36 px
        scale_step 0.5   3.604e-5 / 8.218e-7 px, flow up to 4.76 px
    asserted: four times the measured figures, a finite oracle flow, and a flow above 1 px."""
    p = bo.params(**dict(dict(PAPER, nscales=2), **over))
    assert len(bo.pyramid(synth_pair[0], p)) == 2
    fo, fw = bo.flow_pair(synth_pair[0], synth_pair[1], p), bw.flow_pair(synth_pair[0], synth_pair[1], p)
    d = np.abs(fo.astype(np.float64) - fw)
    print("max %.3e median %.3e (flow up to %.2f px)" % (d.max(), np.median(d), np.abs(fw).max()))
    assert np.isfinite(fo).all() and np.abs(fw).max() > 1.0  # the pair moves
    assert d.max() <= 4 * dmax and np.median(d) <= 4 * dmed


def test_sor_never_raises_the_quadratic_energy(synth_pair):
    """A frozen inner step's system is symmetric positive definite and 0 < omega < 2: every SOR sweep lowers (or keeps)
    1/2 x'Ax - b'x.  A theorem, asserted strictly, sweep by sweep, in the witness."""
    p = bo.params(**PAPER)
    d0, d1 = (bw.derivatives(np.asarray(g, dtype=np.float64) / 255.0) for g in synth_pair)
    h, w = synth_pair[0].shape
    u, v = np.zeros((h, w)), np.zeros((h, w))
    A, b = bw.system(bw.warp(d0, d1, u, v), u, v, u, v, p)
    assert abs(A - A.T).max() == 0.0 and A.diagonal().min() > 0.0
    order = bw.redblack_order(h, w)
    x = np.zeros(2 * h * w)
    energies = [bw.energy(A, b, x)]
    for _ in range(12):
        x = bw.sor_sweep(A, b, x, p["omega"], order)
        energies.append(bw.energy(A, b, x))
    assert all(e1 <= e0 for e0, e1 in zip(energies, energies[1:])), energies
    assert energies[-1] < energies[0]


def test_a_planted_translation_is_found(planted_flows):
    """64 x 48 texture translated by (1.5, -0.75) px, parameters PAPER.  The bound is not derivable.  Measured when the test
    was written: the float64 witness's mean end-point error over the interior is 0.15266 px (the oracle's 0.15266 px);
    asserted for the oracle: twice the witness's, and below half the displacement's length (0.8385 px)."""
    fo, fw = planted_flows
    print("epe oracle %.5f witness %.5f" % (epe(fo), epe(fw)))
    assert epe(fo) <= 2 * 0.15266
    assert epe(fo) < 0.5 * float(np.hypot(*DISPLACEMENT))


def test_gradient_constancy_survives_a_brightness_offset(planted):
    """10 gray levels added to the second frame: with gamma = 50 the error stays below the error with gamma = 0 (measured
    0.160 px against 1.54 px)."""
    f0, f1 = planted[0], planted[1] + np.float32(10.0)
    with_g = epe(bo.flow_pair(f0, f1, bo.params(**PAPER)))
    without = epe(bo.flow_pair(f0, f1, bo.params(**dict(PAPER, gamma=0.0))))
    print("gamma 50: %.4f  gamma 0: %.4f" % (with_g, without))
    assert with_g < without


BAD = [(dict(alpha=0.0), "alpha"), (dict(alpha=-1.0), "alpha"), (dict(gamma=-0.5), "gamma"), (dict(omega=0.0), "omega"),
       (dict(omega=2.0), "omega"), (dict(scale_step=0.0), "scale_step"), (dict(scale_step=1.0), "scale_step"),
       (dict(epsilon=0.0), "epsilon"), (dict(epsilon=-1e-3), "epsilon"), (dict(nscales=0), "nscales"), (dict(warps=0), "warps"),
       (dict(inner_iters=0), "inner_iters"), (dict(solver_iters=0), "solver_iters")]


@pytest.mark.parametrize("over,field", BAD, ids=[",".join("%s=%s" % kv for kv in o.items()) for o, _ in BAD])
def test_workspace_bytes_rejects_bad_brox_parameters(over, field):
    """va_brox_workspace_bytes needs no GPU: 0 and a message that names the field; the legal neighbours are accepted."""
    from video_analytics_amd import _ffi
    L = _ffi.lib()
    assert L.va_brox_workspace_bytes(64, 48, 1, 2, ctypes.byref(_ffi.default_brox_params(**dict(PAPER, **over)))) == 0, over
    assert field in L.va_last_error().decode(), (over, L.va_last_error())
    for ok in (dict(gamma=0.0), dict(omega=0.01), dict(omega=1.99), dict(scale_step=0.05), dict(scale_step=0.95), dict(nscales=40),
               dict(epsilon=1e-6)):
        assert L.va_brox_workspace_bytes(64, 48, 1, 2, ctypes.byref(_ffi.default_brox_params(**dict(PAPER, **ok)))) > 0, ok


def test_brox_parameter_object():
    from video_analytics_amd import _ffi, flow
    with pytest.raises(ValueError, match="foo"):
        _ffi.default_brox_params(foo=1)
    p = _ffi.default_brox_params(**PAPER)
    assert p.struct_bytes == ctypes.sizeof(_ffi.BroxParams) == 72
    assert _ffi.lib().va_brox_workspace_bytes(8, 8, 1, 2, ctypes.byref(p)) == 0 and b"out of range" in _ffi.lib().va_last_error()
    # a tile the sweep depth leaves no room for is refused by name, before anything runs
    q = _ffi.default_brox_params(**dict(PAPER, solver_iters=12, whole_field=0, tile_w=64, tile_h=64, sweeps_per_launch=12))
    assert _ffi.lib().va_brox_workspace_bytes(224, 224, 1, 2, ctypes.byref(q)) == 0 and b"tuning" in _ffi.lib().va_last_error()
    # the pyramid is S1's, for either parameter object; TV-L1's tile plan is not this method's
    from oracle import tvl1_oracle
    for (w, h) in ((224, 224), (67, 45), (150, 131)):
        assert flow.pyramid_sizes(w, h, p) == tvl1_oracle.pyramid_sizes(w, h, 16, 0.8)
        assert flow.pyramid_sizes(w, h, _ffi.default_brox_params(**dict(PAPER, nscales=3))) == tvl1_oracle.pyramid_sizes(w, h, 3, 0.8)
    with pytest.raises(ValueError, match="tile_plan"):
        flow.tile_plan(224, 224, p)


def _accepts(w, h, **kw):
    from video_analytics_amd import _ffi
    return _ffi.lib().va_brox_workspace_bytes(w, h, 1, 2, ctypes.byref(_ffi.default_brox_params(**dict(PAPER, nscales=1, **kw)))) > 0


@pytest.mark.parametrize("K,th,last", [(1, 70, 70), (3, 62, 62), (5, 54, 54), (17, 6, 6)])
def test_the_shape_helper_refuses_the_tiles_the_library_refuses(K, th, last):
    """tests/flow_shapes.py against ``pick_shape`` where its decision shows on the host: on 224 x 224, every tile width
    from 2 to 120 beside a height that makes the region 78 rows.  The two agree on every width; the largest accepted tile
    has a region of 78 x 78 (3042 pixel pairs of the 3072) and the next width is refused (79 x 78: 3120).

    This is also the one place where the halo H = 2K + 2 itself shows.  The coefficients are wrong up to one pixel from an
    inner region edge and K red-black sweeps carry that to 2K pixels at the most, so a halo of 2K + 1 would give the same
    flow bit for bit: no comparison of results can tell the two apart, the accepted tile widths do."""
    import flow_shapes as fs
    got = [tw for tw in range(2, 121) if _accepts(224, 224, solver_iters=K, whole_field=0, tile_w=tw, tile_h=th, sweeps_per_launch=K)]
    want = [tw for tw in range(2, 121) if fs.brox_shape(224, 224, K, whole_field=0, tile_w=tw, tile_h=th, sweeps_per_launch=K)]
    assert got == want == list(range(2, last + 1))
    s = fs.brox_shape(224, 224, K, whole_field=0, tile_w=last, tile_h=th, sweeps_per_launch=K)
    assert (s["rw"], s["rh"], s["pairs"], s["form"]) == (78, 78, 3042, (1024, 3)) and s["lds"] == 80 * 80 * 12
    # a region of exactly 3072 pairs (96 x 64, as wide as the frame) is the last one accepted
    assert _accepts(96, 224, solver_iters=3, whole_field=0, tile_w=96, tile_h=48, sweeps_per_launch=3)
    assert fs.brox_shape(96, 224, 3, whole_field=0, tile_w=96, tile_h=48, sweeps_per_launch=3)["pairs"] == 3072
    assert not _accepts(97, 224, solver_iters=3, whole_field=0, tile_w=97, tile_h=48, sweeps_per_launch=3)
    assert fs.brox_shape(97, 224, 3, whole_field=0, tile_w=97, tile_h=48, sweeps_per_launch=3) is None


def test_every_brox_limit_case_is_legal_and_reaches_the_form_it_is_named_for():
    """the cases of tests/test_brox_params_gpu.py, before a GPU sees them: the library accepts each, and the helper gives the
    pixel pairs, the instantiation, the sweep split and an LDS size below the limit"""
    import flow_shapes as fs
    for w, h, it, pairs, form in fs.BROX_WHOLE_CASES:
        s = fs.brox_shape(w, h, it)
        assert _accepts(w, h, solver_iters=it) and s["whole"] and (s["pairs"], s["form"]) == (pairs, form) and s["lds"] <= fs.MAX_LDS
    # both sides of each number launch_inner compares with, and of the whole-field limit
    assert [fs.brox_form(n) for n in (256, 257, 1024, 1025, 2048, 2049, 3072)] == [(256, 1), (256, 4), (256, 4), (1024, 2), (1024, 2),
                                                                                   (1024, 3), (1024, 3)]
    for c in fs.BROX_TILED_CASES:
        s = fs.brox_shape(c["w"], c["h"], c["solver_iters"], **c["tuning"])
        assert _accepts(c["w"], c["h"], solver_iters=c["solver_iters"], **c["tuning"]) and not s["whole"]
        assert all(s[k] == c[k] for k in ("K", "H", "TW", "TH", "rw", "rh", "pairs", "form")), s
        assert max(fs._pairs(*r) for r in fs.brox_regions(s, c["w"], c["h"])) == c["runs"]
    for w, h in fs.BROX_SPLIT_FIELDS:
        for it, spl, K, launches in fs.BROX_SPLIT_CASES:
            s = fs.brox_shape(w, h, it, whole_field=0, sweeps_per_launch=spl)
            assert _accepts(w, h, solver_iters=it, whole_field=0, sweeps_per_launch=spl), (w, h, it, spl)
            assert (s["K"], s["launches"]) == (K, launches) and s["pairs"] <= fs.BROX_MAX_PAIRS and s["lds"] <= fs.MAX_LDS
    s = fs.brox_shape(150, 131, 17, whole_field=0, sweeps_per_launch=17)
    assert (s["TW"], s["TH"], s["H"], s["rw"], s["rh"], s["pairs"]) == (6, 6, 36, 78, 78, 3042)
    # the rotation of the three (du, dv) buffers: three launches and two launches per step end in each buffer in turn
    for spl, ends in ((1, [1, 2, 0, 1]), (2, [2, 1, 0, 2]), (3, [1, 2, 0, 1])):
        assert fs.brox_rotation(fs.brox_shape(67, 45, 3, whole_field=0, tile_w=32, tile_h=24, sweeps_per_launch=spl), 4) == ends
    assert fs.brox_rotation(fs.brox_shape(67, 45, 3), 4) == [0, 0, 0, 0]
    assert not _accepts(64, 48, solver_iters=20, whole_field=0, sweeps_per_launch=18)  # kMaxK is the last K
    assert _accepts(64, 48, solver_iters=20, whole_field=0, sweeps_per_launch=fs.BROX_MAX_K)
