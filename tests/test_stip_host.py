"""Space-time interest points on the CPU: the float32 / integer oracle (tests/stip_oracle.py) held to an
independent float64 witness (tests/stip_witness_f64.py), the index fold, the cell edges and the 2^32 bound.  No GPU.

Tolerances are 16 times the deviation recorded on these scenes (relative to max |.| of each array), the project's practice
since the Fisher-vector tests.  Recorded (two scenes, all scale pairs):
    L          4.7e-07   (float32 rounding of three passes of up to 45 tap pairs)
    products   3.1e-06
    H          3.5e-06
    descriptor 1.7e-05 absolute on unit-norm rows: the arctangent polynomial of S70 (2e-6 of a bin) and the fixed point of
               S88 (2^-8 gray levels per vote, 2^-12 pixels of flow) bound it from below
"""
import math

import numpy as np
import pytest

import stip_oracle as so
import stip_scenes as scenes
import stip_witness_f64 as sw

DEV_L, DEV_S, DEV_H, DEV_DESC = 4.7e-7, 3.1e-6, 3.5e-6, 1.7e-5
SINGLE = dict(sigmas=(2.0,), taus=(2.0 ** 0.5,))
# the planted reversal: distance in voxels from the event to the strongest point of the scale pair with the strongest point
EVENT_DISTANCE = 4.13  # recorded: event (24, 25, 6), strongest point (20, 24, 6) at the finest pair; the blob's track lies to its left

_cache = {}


def case(name):
    """(gray, flow, event, params, oracle {pair: (L, S, H)}, oracle points / response / desc, witness {pair: (L, S, H)}):
    computed once per scene, never changed"""
    if name not in _cache:
        if name == "defaults":
            gray, flow, ev = scenes.events(T=12, w=48, h=40, seed=6)
            p = so.params()
        else:
            gray, flow, ev = scenes.events(T=16, w=96, h=80, seed=4, grid=(8, 6))
            p = so.params(**SINGLE)
        keep = {}
        pts, resp, desc = so.extract(gray, flow, p, keep)
        wit = {(si, ti): sw.harris(gray, s, t, p) for si, s in enumerate(p["sigmas"]) for ti, t in enumerate(p["taus"])}
        _cache[name] = (gray, flow, ev, p, keep, pts, resp, desc, wit)
    return _cache[name]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", ["defaults", "single"])
def test_oracle_fields_are_the_witness(name):
    _, _, _, p, keep, _, _, _, wit = case(name)
    worst = [0.0, 0.0, 0.0]
    for pair, (L, S, H) in keep.items():
        Lw, Sw, Hw = wit[pair]
        worst[0] = max(worst[0], _rel(L, Lw))
        worst[1] = max(worst[1], max(_rel(S[c], Sw[c]) for c in range(6)))
        worst[2] = max(worst[2], _rel(H, Hw))
    print("deviation L %.3g products %.3g H %.3g" % tuple(worst))
    assert worst[0] <= 16 * DEV_L and worst[1] <= 16 * DEV_S and worst[2] <= 16 * DEV_H


@pytest.mark.parametrize("neighbours", [6, 26])
@pytest.mark.parametrize("name", ["defaults", "single"])
def test_oracle_points_are_the_witness_maxima(name, neighbours):
    """every witness maximum that clears its neighbours by more than m is an oracle point; every oracle point is a witness
    maximum or within m of being one; at least 20 witness points have such a margin (6 neighbours)"""
    _, _, _, p, keep, _, _, _, wit = case(name)
    strong = 0
    for pair, (_, _, Ho) in keep.items():
        Hw = wit[pair][2]
        m = 16 * DEV_H * float(np.abs(Hw).max())
        margin = sw.neighbour_margin(Hw, neighbours)
        opts = set(map(tuple, so.maxima(Ho, p["min_response"], neighbours).tolist()))
        wpts = set(map(tuple, np.asarray(sw.maxima(Hw, p["min_response"], neighbours)).tolist()))
        for x, y, t in wpts:
            if margin[t, y, x] > m and Hw[t, y, x] > p["min_response"] + m:
                strong += 1
                assert (x, y, t) in opts, "witness maximum %r of pair %r is not an oracle point" % ((x, y, t), pair)
        for x, y, t in opts:
            assert (x, y, t) in wpts or (margin[t, y, x] > -m and Hw[t, y, x] > p["min_response"] - m), \
                "oracle point %r of pair %r is no witness maximum" % ((x, y, t), pair)
    print("witness points with the margin: %d" % strong)
    assert strong >= 20


def test_planted_reversal_is_the_strongest_point():
    _, _, ev, p, _, pts, resp, _, _ = case("defaults")
    best = pts[int(np.argmax(resp))]
    same = (pts[:, 3] == best[3]) & (pts[:, 4] == best[4])
    assert float(resp[same].max()) == float(resp.max())
    d = math.sqrt(sum((int(best[i]) - ev[i]) ** 2 for i in range(3)))
    print("event %r strongest %r distance %.3f" % (ev, best.tolist(), d))
    assert d <= EVENT_DISTANCE + 1.0


@pytest.mark.parametrize("name", ["defaults", "single"])
def test_oracle_descriptors_are_the_witness(name):
    _, flow, _, p, _, pts, _, desc, wit = case(name)
    assert len(pts) >= 20
    dw = sw.describe(pts, {k: v[0] for k, v in wit.items()}, flow, p, so.HOG_VMAX, so.FLOW_VMAX)
    dev = float(np.abs(dw - desc).max())
    print("descriptor deviation %.3g" % dev)
    assert desc.shape == (len(pts), so.descriptor_length(p)) and desc.dtype == np.float32
    assert np.allclose(np.sqrt((desc.astype(np.float64) ** 2).sum(axis=1)), 1.0, atol=1e-6)
    assert dev <= 16 * DEV_DESC


def test_taps_are_scipys_kernel():
    from scipy.ndimage import _filters
    for s in list(so.DEFAULTS["sigmas"]) + [2 * v for v in so.DEFAULTS["sigmas"]] + list(so.DEFAULTS["taus"]) + [0.3, 128.0]:
        r, g = so.taps(s)
        ref = _filters._gaussian_kernel1d(s, 0, r)[r:]
        assert r == int(4.0 * s + 0.5) and g.dtype == np.float32 and len(g) == r + 1
        assert np.abs(g.astype(np.float64) - ref).max() <= 2.0 ** -24 * ref.max()
    assert so.taps(so.DEFAULTS["sigmas"][-1] * 2)[0] == 91 and so.taps(128.0)[0] == so.MAX_RADIUS


@pytest.mark.parametrize("n,r", [(7, 3), (5, 5), (5, 8), (3, 7), (1, 4), (2, 9)])
def test_index_fold_is_numpy_symmetric_padding(n, r):
    """r < n, r = n, n < r < 2n, r > 2n, and the axes of length 1 and 2"""
    a = np.arange(n)
    ref = np.pad(a, r, mode="symmetric")
    assert np.array_equal(so.fold(np.arange(-r, n + r), n), ref)


def test_smoothing_is_scipy_reflect_on_a_short_axis():
    """radii larger than every axis (the 37 x 29 x 7 volume of the GPU test at sigma 22.63, tau 4)"""
    f = np.random.RandomState(0).rand(7, 29, 37) * 255
    from scipy import ndimage
    ref = ndimage.gaussian_filter(f, (4.0, 22.63, 22.63), mode="reflect", truncate=4.0)
    assert _rel(so.smooth(f, 22.63, 4.0), ref) <= 16 * DEV_L


def test_cell_edges_are_their_literal_restatement():
    rs = np.random.RandomState(1)
    for _ in range(200):
        c, n, size = int(rs.randint(-5, 70)), int(rs.randint(1, 9)), int(rs.randint(1, 64))
        delta = float(rs.uniform(0.5, 420.0))
        got = so.cell_edges(c, delta, n, size)
        ref = [int(np.clip(np.rint(c - delta / 2 + j * delta / n), 0, size)) for j in range(n + 1)]
        assert got == ref and got == sw.edges(c, delta, n, size)
        assert all(b >= a for a, b in zip(got, got[1:])) and all(b - a <= math.ceil(delta / n) + 1 for a, b in zip(got, got[1:]))
    assert so.cell_edges(3, 36.0, 3, 48) == [0, 0, 9, 21]  # a cuboid that leaves the frame: an empty first cell


def test_largest_admitted_cell_stays_below_2_32():
    """S88's proof, evaluated: the largest slice the defaults admit, and the largest any accepted parameters admit"""
    p = so.params()
    assert so.max_slice(p) == 69 * 69 <= so.MAX_SLICE
    for vmax, shift in ((so.HOG_VMAX, so.HOG_SHIFT), (so.FLOW_VMAX, so.FLOW_SHIFT)):
        top = int(vmax * 2 ** shift)
        assert top == 2 ** 17
        assert so.MAX_SLICE * top < 2 ** 32 <= (so.MAX_SLICE + 1) * top
    # the clamp is reached and not passed: one vote, along a bin centre and between two
    v = so.group_votes(np.float32([1e6, 3e4]), np.float32([0.0, 3e4]), so.FLOW_VMAX, so.FLOW_SHIFT, 4)
    assert int(v.max()) == 2 ** 17 and v[:, 0].tolist() == [2 ** 17, 0, 0, 0]


def test_maxima_rules_on_a_hand_made_volume():
    H = np.zeros((5, 5, 6), dtype=np.float32)
    H[2, 2, 2] = 1.0            # a point
    H[2, 2, 4] = np.nan         # never a point, and (2,2,3) beside it neither
    H[0, 2, 2] = 5.0            # on a face
    assert so.maxima(H, 0.0, 6).tolist() == [[2, 2, 2]] and so.maxima(H, 0.0, 26).tolist() == [[2, 2, 2]]
    assert sw.maxima(H.astype(np.float64), 0.0, 6).tolist() == [[2, 2, 2]]
    H[2, 2, 3] = 1.0            # an exact tie along x disqualifies both
    assert len(so.maxima(H, 0.0, 6)) == 0
    H[2, 2, 3] = 0.0
    H[3, 3, 3] = 1.0            # a diagonal tie: both stay with 6 neighbours, neither with 26
    assert so.maxima(H, 0.0, 6).tolist() == [[2, 2, 2], [3, 3, 3]] and len(so.maxima(H, 0.0, 26)) == 0
    assert len(so.maxima(H, 1.0, 6)) == 0  # min_response is strict


def test_library_taps_and_defaults_are_the_oracle():
    """needs the built library, not a GPU"""
    from video_analytics_amd import _ffi, stip
    p = _ffi.default_stip_params()
    d = so.params()
    assert p.sigma_list == list(d["sigmas"]) and p.tau_list == list(d["taus"])
    for name in ("integration", "k", "min_response", "cuboid", "neighbours", "nx", "ny", "nt", "bins"):
        assert getattr(p, name) == d[name], name
    assert stip.descriptor_length(p) == so.descriptor_length(d) == 144
    for s in list(d["sigmas"]) + [2.0 * v for v in d["sigmas"]] + list(d["taus"]) + [2.0 * v for v in d["taus"]] + [0.2, 128.0]:
        assert np.array_equal(_ffi.stip_taps(s).view(np.uint32), so.taps(s)[1].view(np.uint32))
    with pytest.raises(ValueError, match="sigmas\\[0\\]"):
        _ffi.default_stip_params(sigmas=[100.0])
    with pytest.raises(ValueError, match="cell slice"):
        _ffi.default_stip_params(cuboid=30.0)
    with pytest.raises(ValueError, match="bins"):
        _ffi.default_stip_params(bins=1)
    with pytest.raises(ValueError, match="neighbours"):
        _ffi.default_stip_params(neighbours=18)
    with pytest.raises(ValueError, match="unknown"):
        _ffi.default_stip_params(sigma=2.0)
    assert stip.point_bound(48, 40, 12, p) == 23 * 38 * 10 * 12
