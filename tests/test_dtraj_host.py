"""Dense trajectories without a GPU: the polynomial of S70 against ``np.arctan2``, the float32 / integer
oracle (tests/dtraj_oracle.py) against the independent float64 witness (tests/dtraj_witness_f64.py), a planted scene whose
trajectories are known, and the parameter validation of the library's host side."""
import ctypes
import math

import numpy as np
import pytest

import dtraj_oracle as do
import dtraj_scenes as scenes
import dtraj_witness_f64 as wit

# S70, measured with this test's grid (bins of 45 degrees): the largest |a - arctan2| over 4 x 2,000,001 directions.  The
# assertion is twice that; DESIGN.md S70 records both numbers.
POLY_MEASURED = 7.75e-7
POLY_BOUND = 2 * POLY_MEASURED


def test_polynomial_against_arctan2():
    th = np.linspace(0.0, 2.0 * math.pi, 2000001)
    worst = 0.0
    for r in (1.0, 0.37, 123.4, 1e-3):
        x, y = (r * np.cos(th)).astype(np.float32), (r * np.sin(th)).astype(np.float32)
        m, a = do.orient(x, y)
        assert a.dtype == np.float32 and float(a.min()) >= 0.0 and float(a.max()) <= 8.0
        ref = np.mod(np.arctan2(y.astype(np.float64), x.astype(np.float64)), 2.0 * math.pi) / (math.pi / 4.0)
        d = np.abs(a.astype(np.float64) - ref)
        worst = max(worst, float(np.minimum(d, 8.0 - d).max()))
    print("S70 polynomial: max |a - arctan2| = %.3e bins (bound %.3e)" % (worst, POLY_BOUND))
    assert worst <= POLY_BOUND
    # the seams: exact on the axes, the zero vector has no angle and no length
    m, a = do.orient(np.float32([1, 0, -1, 0, 0]), np.float32([0, 1, 0, -1, 0]))
    assert a.tolist() == [0.0, 2.0, 4.0, 6.0, 0.0] and m.tolist() == [1.0, 1.0, 1.0, 1.0, 0.0]


def _smooth_scene(w, h, seed):
    """gray in [0,255] and a smooth flow of about a pixel whose length stays clear of min_flow's threshold"""
    g, a, b = scenes.texture(3, w, h, seed)
    u, v = (a - 128.0) / 96.0, (b - 128.0) / 96.0
    return g, u.astype(np.float32), v.astype(np.float32)


def test_votes_and_cell_sums_agree_with_the_float64_witness():
    """Per vote the oracle differs from the witness by the rounding to the fixed-point quantum (half a quantum) and by what the
    polynomial and float32 do to the angle and the length: a is within POLY_BOUND of the angle (the measurement includes a's
    own rounding), f = a - floor(a) is exact, 1 - f and the product round once each (2^-24), and m carries at most 2^-22 of
    itself (two products, a sum, a root).  That is m (POLY_BOUND + 2^-22 + 2^-23), which for this scene's magnitudes stays
    below another half quantum in every group (asserted).  So a vote agrees within one quantum and a cell's sum within one
    quantum times its pixels."""
    w, h = 48, 40
    g, u, v = _smooth_scene(w, h, 3)
    p = do.params(patch=16)
    q = do.votes(g, u, v, p)
    ref = wit.votes(g, u, v, p["min_flow"])
    assert np.abs(wit.flow_magnitude(u, v) - p["min_flow"]).min() > 1e-4  # no pixel sits on the threshold of the ninth bin
    assert q[16].sum() > 0 and (q[16] == 0).sum() > 0                      # and both sides of it occur
    float_err = POLY_BOUND + 2.0 ** -22 + 2.0 ** -23
    for name, p0, nb in do.GROUPS:
        shift = do.HOG_SHIFT if name == "hog" else do.FLOW_SHIFT
        quantum = 2.0 ** -shift
        mmax = ref[p0:p0 + 8].sum(axis=0).max()  # the two bins of a pixel share m
        assert mmax * float_err < quantum / 2, (name, mmax)
        err = np.abs(q[p0:p0 + nb].astype(np.float64) * quantum - ref[p0:p0 + nb]).max()
        print("%s: max |vote - witness| = %.3e (quantum %.3e)" % (name, err, quantum))
        assert err <= quantum, name
    I = do.integral(q)
    for (x, y) in [(0, 0), (w - 1, h - 1), (20, 17), (3, 30), (w - 1, 2)]:
        got = []
        cs = p["patch"] // p["nxy"]
        for cy in range(p["nxy"]):
            for cx in range(p["nxy"]):
                xa, ya = x - p["patch"] // 2 + cx * cs, y - p["patch"] // 2 + cy * cs
                box = (min(max(xa, 0), w), min(max(xa + cs, 0), w), min(max(ya, 0), h), min(max(ya + cs, 0), h))
                got.append(do.cell_sum(I, *box))
                assert got[-1].tolist() == do.direct_cell_sum(q, *box)
        got = np.array(got, dtype=np.float64)
        want = wit.tube_slice(ref, x, y, p["patch"], p["nxy"])
        for name, p0, nb in do.GROUPS:
            quantum = 2.0 ** -(do.HOG_SHIFT if name == "hog" else do.FLOW_SHIFT)
            assert np.abs(got[:, p0:p0 + nb] * quantum - want[:, p0:p0 + nb]).max() <= quantum * cs * cs, (name, x, y)


def test_integral_cell_sums_are_exact_where_the_planes_wrap():
    """300 x 300 of the largest HOG vote: the running sum passes 2^32 ten times over, a 64 x 64 cell's sum is exactly 2^31"""
    top = int(do.HOG_VMAX * 2 ** do.HOG_SHIFT)
    q = np.full((2, 300, 300), top, dtype=np.uint32)
    q[1] = np.random.RandomState(0).randint(0, top + 1, size=(300, 300)).astype(np.uint32)
    I = do.integral(q)
    assert int(q[0].astype(np.uint64).sum()) > 10 * 2 ** 32 and int(I[0, 300, 300]) == (300 * 300 * top) % 2 ** 32
    assert 64 * 64 * top == 2 ** 31 < 2 ** 32 and 64 * 64 * int(do.FLOW_VMAX * 2 ** do.FLOW_SHIFT) == 2 ** 31  # S71's inequality
    for box in [(0, 64, 0, 64), (236, 300, 236, 300), (100, 164, 7, 71), (299, 300, 0, 64), (5, 5, 0, 64), (17, 70, 250, 300)]:
        assert do.cell_sum(I, *box).tolist() == do.direct_cell_sum(q, *box), box
    assert do.cell_sum(I, 236, 300, 236, 300)[0] == 2 ** 31


PLANTED = dict(length=6, nt=3, patch=16)


@pytest.fixture(scope="module")
def planted():
    gray, flow, rects = scenes.planted()
    p = do.params(**PLANTED)
    dropped = []
    out = do.extract(gray, flow, do.median3(flow), p, dropped)
    return gray, flow, rects, p, out, dropped


def _inside(pt, rect, margin=0):
    return rect[0] + margin <= pt[0] <= rect[2] - 1 - margin and rect[1] + margin <= pt[1] <= rect[3] - 1 - margin


def test_planted_scene_trajectories(planted):
    gray, flow, rects, p, out, dropped = planted
    L = p["length"]
    assert out["count"] >= 50 and len(out["started_frames"]) >= 3
    unit = np.array([2.0, 1.0]) / (L * math.hypot(2.0, 1.0))
    a = math.atan2(1.0, 2.0) / (math.pi / 4.0)
    assert 0 < a < 1
    on_box = 0
    for desc, pts, start in zip(out["desc"], out["points"], out["start"]):
        if not all(_inside(pts[k], rects[start + k]) for k in range(L + 1)):
            continue
        on_box += 1
        assert np.array_equal(pts[1:] - pts[:-1], np.tile(np.float32([2, 1]), (L, 1)))
        assert np.abs(desc[:2 * L].reshape(L, 2) - unit).max() < 1e-7
        hof = desc[2 * L + 96:2 * L + 204].reshape(-1, 9)
        assert np.all(hof[:, 2:8] == 0) and hof[:, 0].sum() > 0 and hof[:, 1].sum() > 0  # only the bins around atan2(1, 2), and bin 8
        for name, lo, hi in (("hog", 0, 96), ("hof", 96, 204), ("mbhx", 204, 300), ("mbhy", 300, 396)):
            n = float(np.linalg.norm(desc[2 * L + lo:2 * L + hi].astype(np.float64)))
            assert n == 0.0 or abs(n - 1.0) < 1e-6, (name, n)
    assert on_box >= 40
    # the background: a track the box never reaches stands still, is rejected as static, and its flow histogram is all bin 8
    assert out["rejected"]["erratic"] == 0 and out["rejected"]["jump"] == 0 and out["rejected"]["unfinished"] == 0
    still = 0
    for t, code in dropped:
        far = all(not _inside(t["pts"][0], rects[t["start"] + k], -(p["patch"] // 2 + 1)) for k in range(L + 1))
        if far:
            still += 1
            assert code == 1 and len(set(t["pts"])) == 1
            hof = t["acc"].reshape(-1, 33)[:, 8:17]
            assert np.all(hof[:, :8] == 0) and np.all(hof[:, 8] > 0)
    assert still >= 20


def test_planted_scene_agrees_with_the_witness(planted):
    """the scene's flow is whole pixels, so both follow the same points; the descriptors agree as far as the quantum allows"""
    gray, flow, rects, p, out, dropped = planted
    found, rej = wit.extract(gray.astype(np.float64), flow.astype(np.float64), do.median3(flow).astype(np.float64), p)
    assert len(found) == out["count"] and rej == [out["rejected"][k] for k in do.REJECTED]
    for (d, pts, start), od, opts, ostart in zip(found, out["desc"], out["points"], out["start"]):
        assert start == ostart and np.array_equal(np.array(pts), opts.astype(np.float64))
        assert np.abs(d - od.astype(np.float64)).max() < 1e-4


def test_default_parameters_and_exports():
    from video_analytics_amd import _ffi, trajectories
    p = _ffi.default_dense_traj_params()
    got = {k: getattr(p, k) for k in do.DEFAULTS}
    assert got == {k: (v if isinstance(v, int) else float(np.float32(v))) for k, v in do.DEFAULTS.items()}
    assert p.struct_bytes == ctypes.sizeof(_ffi.DenseTrajParams) and list(p.tuning) == [0] * 8
    assert trajectories.descriptor_length(p) == do.descriptor_length(do.params()) == 426
    for name in ("va_dtraj_default_params", "va_dtraj_workspace_bytes", "va_dtraj_extract", "va_dtraj_votes", "va_dtraj_integral",
                 "va_dtraj_corner", "va_dtraj_sample", "va_dtraj_step", "va_dtraj_finish"):
        assert name in _ffi.EXPORTS
    L = _ffi.lib()
    small = L.va_dtraj_workspace_bytes(320, 240, 150, 1000, ctypes.byref(_ffi.default_dense_traj_params(chunk_frames=1)))
    large = L.va_dtraj_workspace_bytes(320, 240, 150, 1000, ctypes.byref(_ffi.default_dense_traj_params(chunk_frames=8)))
    per_frame = 33 * 4 * (320 * 240 + 321 * 241)  # votes and integral planes of one frame: the chunk is accounted for
    assert small > 0 and large - small >= 7 * per_frame
    assert trajectories.trajectory_bound(320, 240, 150, p) == 64 * 48 * 135
    nbytes, off = _ffi.dtraj_state_layout(40, 30, p)
    assert list(off) == list(_ffi.DTRAJ_STATE_REGIONS) and sorted(off.values()) == list(off.values()) and nbytes > off["pending"]


BAD = [
    (dict(length=16), "length"), (dict(nt=0), "nt"), (dict(patch=33), "patch"), (dict(patch=132, nxy=2), "patch / nxy"),
    (dict(nxy=0), "nxy"), (dict(step=1), "step"), (dict(quality=0.0), "quality"), (dict(quality=1.0), "quality"),
    (dict(quality=float("nan")), "quality"), (dict(min_flow=0.0), "min_flow"), (dict(min_std=-1.0), "min_std"),
    (dict(max_std=0.0), "max_std"), (dict(max_dis=float("nan")), "max_dis"), (dict(max_dis_share=0.0), "max_dis_share"),
    (dict(chunk_frames=-1), "tuning[0]"), (dict(votes_tile_w=257), "tuning[1]"), (dict(votes_tile_h=65), "tuning[2]"),
    (dict(votes_tile_w=256, votes_tile_h=64), "LDS"),
]


@pytest.mark.parametrize("over,msg", BAD, ids=[",".join("%s=%s" % kv for kv in o.items()) for o, _ in BAD])
def test_refused_parameters_are_named(over, msg):
    from video_analytics_amd import _ffi
    with pytest.raises(ValueError, match="va_dtraj") as e:
        _ffi.default_dense_traj_params(**over)
    assert msg in str(e.value), str(e.value)


def test_refused_sizes_and_unknown_names():
    from video_analytics_amd import _ffi
    L, p = _ffi.lib(), _ffi.default_dense_traj_params()
    for args, msg in (((15, 64, 10, 5), "out of range"), ((64, 16385, 10, 5), "out of range"), ((64, 64, 1, 5), "n_frames"),
                      ((64, 64, 10, 0), "capacity")):
        assert L.va_dtraj_workspace_bytes(*args, ctypes.byref(p)) == 0 and msg in L.va_last_error().decode(), args
    assert L.va_dtraj_workspace_bytes(64, 64, 2, 1, ctypes.byref(p)) > 0
    p.tuning[5] = 1
    assert L.va_dtraj_workspace_bytes(64, 64, 10, 5, ctypes.byref(p)) == 0 and "reserved" in L.va_last_error().decode()
    with pytest.raises(ValueError, match="unknown dense-trajectory parameter"):
        _ffi.default_dense_traj_params(lenght=15)
    tiny = _ffi.DenseTrajParams()
    assert L.va_dtraj_workspace_bytes(64, 64, 10, 5, ctypes.byref(tiny)) == 0 and "struct_bytes" in L.va_last_error().decode()
