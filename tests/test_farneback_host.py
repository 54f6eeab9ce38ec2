"""Farneback optical flow without a GPU: the float32 oracle (tests/farneback_oracle.py, the executable
form of the specification) against an independent float64 witness (tests/farneback_witness_f64.py) and against known answers,
and the host side of the C ABI (parameter validation, the Python parameter object).  No test depends on the default
parameters: every one names the values it runs with."""
import ctypes

import numpy as np
import pytest
import torch

import brox_witness_f64 as bw
import farneback_oracle as fo
import farneback_witness_f64 as fw

SHEET = dict(pyr_scale=0.5, poly_sigma=1.2, levels=3, winsize=15, iterations=3, poly_n=5, gaussian=0)  # the modelled project's call
DISPLACEMENT = (1.5, -0.75)

# The oracle against the witness, measured when the tests were written (the figures are printed by the tests below):
#   polynomial expansion of the textured 40 x 32 frame: largest difference POLY_DIFF over the five planes (coefficients up to 48)
#   flow of the 3-level run on the 80 x 64 pair: largest difference FLOW_DIFF px (the flow reaches 1.6 px)
# Neither is derivable (float32 rounding through eleven-tap sums of values near 255, then nine passes of a 2x2 solve); each
# is asserted at four times the measured figure, which covers how float32 rounding varies between inputs of the same size.
POLY_DIFF = 1.979e-5
FLOW_DIFF = 1.523e-6


def _texture(H, W, seed, sigma, M):
    """a blurred random texture of (H + 2M) x (W + 2M) in [0,255], float64"""
    from video_analytics_amd import synth
    t = torch.from_numpy(np.random.RandomState(seed).rand(1, 1, H + 2 * M, W + 2 * M).astype(np.float32))
    t = synth._blur(t, sigma)[0, 0].numpy().astype(np.float64)
    return (t - t.min()) / (t.max() - t.min()) * 255.0


@pytest.fixture(scope="module")
def planted():
    """A smooth random texture of 80 x 64 and the same texture translated by DISPLACEMENT (sampled from a larger one)"""
    H, W, M = 64, 80, 8
    t = _texture(H, W, 5, 2.0, M)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    f0 = bw.sample(t, xx + M, yy + M)
    f1 = bw.sample(t, xx + M - DISPLACEMENT[0], yy + M - DISPLACEMENT[1])
    return f0.astype(np.float32), f1.astype(np.float32)


@pytest.fixture(scope="module")
def planted_flows(planted):
    p = fo.params(**SHEET)
    return fo.flow_pair(planted[0], planted[1], p), fw.flow_pair(planted[0], planted[1], p)


def epe(f):
    """mean end-point error against DISPLACEMENT over the interior, 8 px from the border"""
    e = np.sqrt((f[0].astype(np.float64) - DISPLACEMENT[0]) ** 2 + (f[1].astype(np.float64) - DISPLACEMENT[1]) ** 2)
    return float(e[8:-8, 8:-8].mean())


@pytest.mark.parametrize("poly_n,poly_sigma", [(5, 1.2), (7, 1.5)])
def test_the_witness_recovers_an_exact_quadratic(poly_n, poly_sigma):
    """The fit is exact for a quadratic image wherever the window stays inside the frame: f(d) = c + b.d + d'Ad around every
    pixel has the image's own second derivatives and the gradient at that pixel.  Derivable: float64 rounding, a relative 1e-9."""
    yy, xx = np.mgrid[0:32, 0:40].astype(np.float64)
    x, y = xx - 20.0, yy - 15.0
    img = 3.0 + 0.7 * x - 0.4 * y + 0.05 * x * x - 0.03 * y * y + 0.02 * x * y
    r = fw.polyexp(img, fo.params(**dict(SHEET, poly_n=poly_n, poly_sigma=poly_sigma)))
    want = (0.7 + 0.1 * x + 0.02 * y, -0.4 - 0.06 * y + 0.02 * x, 0.05 + 0 * x, -0.03 + 0 * x, 0.02 + 0 * x)
    inner = (slice(poly_n, -poly_n), slice(poly_n, -poly_n))
    for got, w in zip(r, want):
        rel = np.abs(got[inner] - w[inner]).max() / np.abs(w[inner]).max()
        print("relative error %.3e" % rel)
        assert rel <= 1e-9


def test_the_oracle_expansion_agrees_with_the_float64_witness():
    """polynomial expansion of a textured 40 x 32 frame: the separable float32 closed form against the per-pixel least-squares
    fit, borders included"""
    img = _texture(32, 40, 11, 1.0, 0).astype(np.float32)
    p = fo.params(**SHEET)
    a, b = fo.polyexp(img, p), fw.polyexp(img, p)
    assert a.dtype == np.float32 and a.shape == (5, 32, 40)
    d = np.abs(a.astype(np.float64) - b).max()
    print("max difference %.3e (coefficients up to %.1f)" % (d, np.abs(b).max()))
    assert np.abs(b).max() > 10.0  # the frame is textured
    assert d <= 4 * POLY_DIFF


def test_the_oracle_flow_agrees_with_the_float64_witness(planted_flows):
    """the flow of the 3-level run on the 80 x 64 pair"""
    a, b = planted_flows
    assert a.dtype == np.float32 and a.shape == (2, 64, 80)
    d = np.abs(a.astype(np.float64) - b)
    print("max difference %.3e median %.3e (flow up to %.2f px)" % (d.max(), np.median(d), np.abs(b).max()))
    assert np.abs(b).max() > 1.0  # the pair moves
    assert d.max() <= 4 * FLOW_DIFF


def test_a_planted_translation_is_found(planted_flows):
    """80 x 64 texture translated by (1.5, -0.75) px, the modelled project's parameters.  Measured when the test was written:
    the float64 witness's mean end-point error over the interior is 0.01604 px (the method's accuracy on this
    scene; not asserted against an outside number).  Asserted for the oracle: at most the witness's plus the
    oracle-against-witness bound above."""
    a, b = planted_flows
    print("epe oracle %.5f witness %.5f" % (epe(a), epe(b)))
    assert epe(a) <= epe(b) + 4 * FLOW_DIFF


def test_identical_frames_give_exactly_zero_flow(planted):
    """db = 0 on every level: h = 0 and the solve returns 0 whatever G is"""
    f = fo.flow_pair(planted[0], planted[0], fo.params(**SHEET))
    assert f.shape == (2, 64, 80) and np.all(f == 0.0)


BAD = [(dict(pyr_scale=0.0), "pyr_scale"), (dict(pyr_scale=1.0), "pyr_scale"), (dict(winsize=14), "winsize"), (dict(winsize=1), "winsize"),
       (dict(winsize=65), "winsize"), (dict(poly_n=9), "poly_n"), (dict(poly_n=6), "poly_n"), (dict(poly_sigma=0.0), "poly_sigma"),
       (dict(poly_sigma=-1.2), "poly_sigma"), (dict(levels=0), "levels"), (dict(iterations=0), "iterations"), (dict(gaussian=2), "gaussian"),
       (dict(pass_tile_w=256, pass_tile_h=256), "tuning"), (dict(poly_tile_w=-1), "tuning"), (dict(pass_tile_h=257), "tuning")]


def _raw(**over):
    """a FarnebackParams with the values written into it unchecked, as a C caller would"""
    from video_analytics_amd import _ffi
    p = _ffi.default_farneback_params()
    for k, v in dict(SHEET, **over).items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("over,field", BAD, ids=[",".join("%s=%s" % kv for kv in o.items()) for o, _ in BAD])
def test_bad_farneback_parameters_are_refused_by_name(over, field):
    """va_farneback_workspace_bytes needs no GPU: 0 and a message that names the field; default_farneback_params raises
    ValueError with the same text"""
    from video_analytics_amd import _ffi
    L = _ffi.lib()
    assert L.va_farneback_workspace_bytes(64, 48, 1, 2, ctypes.byref(_raw(**over))) == 0, over
    assert field in L.va_last_error().decode(), (over, L.va_last_error())
    with pytest.raises(ValueError, match=field):
        _ffi.default_farneback_params(**dict(SHEET, **over))


def test_farneback_parameter_object():
    from video_analytics_amd import _ffi, flow
    L = _ffi.lib()
    with pytest.raises(ValueError, match="foo"):
        _ffi.default_farneback_params(foo=1)
    p = _ffi.default_farneback_params()
    assert p.struct_bytes == ctypes.sizeof(_ffi.FarnebackParams) == 64
    got = {k: getattr(p, k) for k in SHEET}
    assert got == dict(SHEET, pyr_scale=0.5, poly_sigma=float(np.float32(1.2))) and list(p.tuning) == [0] * 8
    for ok in (dict(pyr_scale=0.05), dict(pyr_scale=0.95), dict(winsize=3), dict(winsize=63), dict(poly_n=7), dict(levels=40),
               dict(gaussian=1), dict(pass_tile_w=1, pass_tile_h=1), dict(poly_tile_w=256, poly_tile_h=8)):
        assert L.va_farneback_workspace_bytes(64, 48, 1, 2, ctypes.byref(_ffi.default_farneback_params(**dict(SHEET, **ok)))) > 0, ok
    for (w, h) in ((8, 64), (64, 15), (16385, 64)):
        assert L.va_farneback_workspace_bytes(w, h, 1, 2, ctypes.byref(p)) == 0 and b"out of range" in L.va_last_error()
    # the pyramid is S1's: levels is its nscales, pyr_scale its scale_step, and a deep request is read as the deepest S1 allows
    from oracle import tvl1_oracle
    for (w, h) in ((224, 224), (83, 67), (80, 64)):
        assert flow.pyramid_sizes(w, h, p) == tvl1_oracle.pyramid_sizes(w, h, 3, 0.5)
        deep = _ffi.default_farneback_params(**dict(SHEET, levels=40))
        assert flow.pyramid_sizes(w, h, deep) == tvl1_oracle.pyramid_sizes(w, h, 16, 0.5)
    # what describes TV-L1's kernels refuses the object by name
    for who, call in (("tile_plan", lambda: flow.tile_plan(224, 224, p)), ("profile_enable", lambda: flow.profile_enable(p)),
                      ("profile_levels", lambda: flow.profile_levels(p)), ("profile_read", lambda: flow.profile_read(p))):
        with pytest.raises(ValueError, match=who):
            call()


# The oracle against the witness away from SHEET, one setting at a time, on the 80 x 64 pair with three levels and three
# iterations (the odd count: SHEET's own, repeated here beside the others): (overrides, largest difference in px), measured
# when the tests were written and printed by the test below.  None is derivable (see FLOW_DIFF).
AWAY = [
    (dict(winsize=3), 4.382e-5),      # an ill-conditioned 3 x 3 window: the flow reaches 15 px
    (dict(winsize=63), 3.462e-6),
    (dict(winsize=63, gaussian=1), 1.425e-6),
    (dict(gaussian=1), 3.362e-6),
    (dict(pyr_scale=0.8), 1.694e-6),
    (dict(iterations=3), 1.523e-6),
    (dict(poly_n=7, poly_sigma=1.5), 1.780e-6),
]


@pytest.mark.parametrize("over,dmax", AWAY, ids=[",".join("%s=%g" % kv for kv in o.items()) for o, _ in AWAY])
def test_the_oracle_flow_agrees_with_the_float64_witness_away_from_the_defaults(planted, over, dmax):
    """The settings tests/test_farneback_params_gpu.py holds the kernels to the oracle at.  Measured when the test was
    written (maximum difference, the witness's largest flow):
        winsize 3               4.382e-5 px, flow up to 15.47 px
        winsize 63              3.462e-6 px, flow up to 1.51 px
        winsize 63, gaussian 1  1.425e-6 px, flow up to 1.53 px
        gaussian 1              3.362e-6 px, flow up to 3.48 px
        pyr_scale 0.8           1.694e-6 px, flow up to 1.65 px
        iterations 3            1.523e-6 px, flow up to 1.65 px
        poly_n 7, sigma 1.5     1.780e-6 px, flow up to 1.70 px
    asserted: four times the measured figure, a finite oracle flow, and a flow above 1 px."""
    p = fo.params(**dict(SHEET, **over))
    a, b = fo.flow_pair(planted[0], planted[1], p), fw.flow_pair(planted[0], planted[1], p)
    d = np.abs(a.astype(np.float64) - b)
    print("max difference %.3e median %.3e (flow up to %.2f px)" % (d.max(), np.median(d), np.abs(b).max()))
    assert np.isfinite(a).all() and np.abs(b).max() > 1.0  # the pair moves
    assert d.max() <= 4 * dmax


def _accepts(**over):
    return _ffi_lib().va_farneback_workspace_bytes(64, 48, 1, 2, ctypes.byref(_raw(**over))) > 0


def _ffi_lib():
    from video_analytics_amd import _ffi
    return _ffi.lib()


@pytest.mark.parametrize("winsize,th,last", [(63, 16, 25), (59, 16, 33), (31, 16, 102), (63, 1, 66), (15, 0, 164)])
def test_the_shape_helper_refuses_the_pass_tiles_the_library_refuses(winsize, th, last):
    """tests/flow_shapes.py against ``pass_tile`` where its decision shows on the host: every caller's tile width from 1 to
    256 beside one height (0: the library's 16).  The two agree on every width, and the last accepted one is named."""
    import flow_shapes as fs
    got = [tw for tw in range(1, 257) if _accepts(winsize=winsize, pass_tile_w=tw, pass_tile_h=th)]
    want = [tw for tw in range(1, 257) if fs.pass_tile(winsize, tw, th)]
    assert got == want == list(range(1, last + 1))
    assert fs.pass_lds(winsize, last, th or 16) <= fs.MAX_LDS and (last == 256 or fs.pass_lds(winsize, last + 1, th or 16) > fs.MAX_LDS)


@pytest.mark.parametrize("poly_n,th,last", [(5, 64, 143), (7, 64, 137), (5, 256, 29), (7, 8, 256)])
def test_the_shape_helper_refuses_the_polyexp_tiles_the_library_refuses(poly_n, th, last):
    """the same for ``poly_tile``"""
    import flow_shapes as fs
    got = [tw for tw in range(1, 257) if _accepts(poly_n=poly_n, poly_tile_w=tw, poly_tile_h=th)]
    want = [tw for tw in range(1, 257) if fs.poly_tile(poly_n, tw, th)]
    assert got == want == list(range(1, last + 1))
    assert fs.poly_lds(poly_n, last, th) <= fs.MAX_LDS and (last == 256 or fs.poly_lds(poly_n, last + 1, th) > fs.MAX_LDS)


def test_every_farneback_limit_case_is_legal_and_runs_the_tile_it_is_named_for():
    """the cases of tests/test_farneback_params_gpu.py, before a GPU sees them, and the figures the tiles are known by"""
    import flow_shapes as fs
    # the window of 63: a caller's 16 x 16 is accepted with 146,640 B, 32 x 16 refused with 176,720 B of the 163,840
    assert _accepts(winsize=63, pass_tile_w=16, pass_tile_h=16) and fs.pass_tile(63, 16, 16) == (16, 16, 146640)
    assert not _accepts(winsize=63, pass_tile_w=32, pass_tile_h=16) and fs.pass_tile(63, 32, 16) is None and fs.pass_lds(63, 32, 16) == 176720
    assert b"tuning" in _ffi_lib().va_last_error()
    # the library's own tile: 32 x 16 up to a window of 59 (162,000 B), halved once for 61 and 63
    assert [fs.pass_tile(ws)[:2] for ws in (3, 5, 15, 31, 57, 59, 61, 63)] == [(32, 16)] * 6 + [(16, 16)] * 2
    assert fs.pass_tile(59)[2] == 162000 and fs.pass_lds(61, 32, 16) > fs.MAX_LDS == 163840
    # poly_n 7: 128 x 64 is accepted with 153,360 B, 256 x 64 refused
    assert _accepts(poly_n=7, poly_tile_w=128, poly_tile_h=64) and fs.poly_tile(7, 128, 64) == (128, 64, 153360)
    assert not _accepts(poly_n=7, poly_tile_w=256, poly_tile_h=64) and fs.poly_tile(7, 256, 64) is None
    for winsize, tile, run, lds, fields in fs.FB_PASS_CASES:
        assert fs.pass_tile(winsize, *tile) == run + (lds,) and lds <= fs.MAX_LDS
        for w, h in fields:
            p = _raw(winsize=winsize, levels=1, pass_tile_w=tile[0], pass_tile_h=tile[1])
            assert _ffi_lib().va_farneback_workspace_bytes(w, h, 1, 2, ctypes.byref(p)) > 0, (winsize, tile, w, h)
    for poly_n, sigma, tile, lds, (w, h) in fs.FB_POLY_CASES:
        assert fs.poly_tile(poly_n, *tile)[2] == lds <= fs.MAX_LDS
        p = _raw(poly_n=poly_n, poly_sigma=sigma, levels=1, poly_tile_w=tile[0], poly_tile_h=tile[1])
        assert _ffi_lib().va_farneback_workspace_bytes(w, h, 1, 2, ctypes.byref(p)) > 0, (poly_n, tile, w, h)
    assert sorted(lds > 64 * 1024 for _, _, _, lds, _ in fs.FB_POLY_CASES) == [False] * 7 + [True] * 2
