"""Space-time interest points on the GPU, bit for bit against the float32 / integer oracle
(tests/stip_oracle.py): every stage alone through its test entry (``va_stip_smooth`` ... ``va_stip_describe``), then
``space_time_interest_points`` end to end on the scenes of tests/test_stip_host.py.  Every comparison is on the raw bits."""
import ctypes

import numpy as np
import pytest
import torch

import stip_oracle as so
import test_stip_host as host

pytestmark = pytest.mark.gpu

# the shapes the dispatcher picks on its own, and shapes forced on it: strips and tiles that divide nothing
TILES = [dict(), dict(row_tile_w=23, col_tile_w=7, col_tile_n=5), dict(row_tile_w=64, col_tile_w=64, col_tile_n=3)]
TILE_IDS = ["default", "23-7x5", "64-64x3"]


def _params(p=None, **tuning):
    from video_analytics_amd import _ffi
    return _ffi.default_stip_params(**dict(p or {}, **tuning))


def _call(name, *args):
    from video_analytics_amd import _ffi
    _ffi.check(getattr(_ffi.lib(), name)(_ffi.ctx(0), *args, _ffi.stream_ptr(torch.device("cuda", 0))))
    torch.cuda.synchronize()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, ref):
    return np.array_equal(_bits(got), _bits(ref))


def _volume(T, h, w, seed, u8=False):
    a = np.random.RandomState(seed).rand(T, h, w) * 255
    return np.rint(a).astype(np.uint8) if u8 else a.astype(np.float32)


def _smooth(f, sigma, tau, **tuning):
    from video_analytics_amd import _ffi
    T, h, w = f.shape
    src = _dev(f)
    n = 2 * T * h * w + 2048
    tmp = torch.empty(n, dtype=torch.float32, device="cuda")
    out = torch.full((T, h, w), float("nan"), dtype=torch.float32, device="cuda")
    p = _params(**tuning)
    _call("va_stip_smooth", _ffi.ptr(src), int(f.dtype == np.uint8), T, w, h, float(sigma), float(tau), ctypes.byref(p), _ffi.ptr(out),
          _ffi.ptr(tmp), n)
    assert np.array_equal(src.cpu().numpy().view(np.uint8), f.view(np.uint8))  # (bytes: the input may hold a NaN)
    return out


# ---------------------------------------------------------------- smoothing (S83-S84)

@pytest.mark.parametrize("tiles", TILES, ids=TILE_IDS)
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("w", [1, 5, 63, 64, 65, 257])
def test_smoothing_is_the_oracle_across_widths(w, u8, tiles):
    """sigma 2 has r = 8: larger than the width 5 and than the 3 frames and 6 rows; widths on either side of a wave"""
    f = _volume(3, 6, w, w, u8)
    assert _same(_smooth(f, 2.0, 2.0, **tiles), so.smooth(f, 2.0, 2.0))


@pytest.mark.parametrize("tiles", TILES, ids=TILE_IDS)
def test_smoothing_with_radii_larger_than_every_axis(tiles):
    """the integration scale of the largest default sigma: r = 91 and 16 on 37 x 29 x 7"""
    f = _volume(7, 29, 37, 1)
    assert so.taps(22.63)[0] == 91 and so.taps(4.0)[0] == 16
    assert _same(_smooth(f, 22.63, 4.0, **tiles), so.smooth(f, 22.63, 4.0))


@pytest.mark.parametrize("shape", [(1, 9, 11), (5, 1, 11), (1, 1, 70), (4, 3, 1)], ids=str)
def test_smoothing_of_flat_volumes(shape):
    f = _volume(*shape, seed=2)
    assert _same(_smooth(f, 1.5, 1.0), so.smooth(f, 1.5, 1.0))


@pytest.mark.parametrize("shape,sigma,tau", [((2, 400, 9), 40.0, 1.0), ((1, 20, 9), 64.0, 1.0), ((300, 2, 5), 1.0, 32.0)], ids=str)
def test_smoothing_in_every_tile_length_the_dispatcher_picks(shape, sigma, tau):
    """the column pass cuts its axis where a 64 KB tile ends (400 rows at r = 160: tiles of 192), falls back to tiles of 8
    beyond r = 252 (r = 256 here, which is also the first tile above 64 KB of LDS), and takes the whole axis otherwise (the
    other tests); the same along t"""
    f = _volume(*shape, seed=3)
    assert _same(_smooth(f, sigma, tau), so.smooth(f, sigma, tau))


def test_smoothing_refuses_by_name():
    from video_analytics_amd import _ffi
    f = _volume(2, 4, 4, 0)
    with pytest.raises(ValueError, match="sigma must be > 0"):
        _smooth(f, 0.0, 1.0)
    with pytest.raises(ValueError, match="tau must be > 0 with a radius"):
        _smooth(f, 1.0, 200.0)
    with pytest.raises(ValueError, match="needs .* bytes of LDS"):
        _smooth(f, 128.0, 1.0, col_tile_w=64)
    with pytest.raises(ValueError, match="tuning\\[1\\]"):
        _params(col_tile_w=65)
    src = _dev(f)
    tmp = torch.empty(16, dtype=torch.float32, device="cuda")
    p = _params()
    with pytest.raises(ValueError, match="tmp of 16 floats"):
        _call("va_stip_smooth", _ffi.ptr(src), 0, 2, 4, 4, 1.0, 1.0, ctypes.byref(p), _ffi.ptr(src), _ffi.ptr(tmp), 16)


# ---------------------------------------------------------------- derivatives, products, response (S85-S86)

def _products(L):
    from video_analytics_amd import _ffi
    T, h, w = L.shape
    d = _dev(L)
    out = torch.full((6, T, h, w), float("nan"), dtype=torch.float32, device="cuda")
    _call("va_stip_gradient_products", _ffi.ptr(d), T, w, h, _ffi.ptr(out))
    return out


def _response(S, k):
    from video_analytics_amd import _ffi
    _, T, h, w = S.shape
    d = S if isinstance(S, torch.Tensor) else _dev(S)
    out = torch.full((T, h, w), float("nan"), dtype=torch.float32, device="cuda")
    _call("va_stip_response", _ffi.ptr(d), T, w, h, float(k), _ffi.ptr(out))
    return out


@pytest.mark.parametrize("shape", [(1, 2, 3), (3, 1, 2), (2, 3, 1), (1, 1, 1), (3, 3, 3), (4, 5, 67)], ids=str)
def test_gradient_products_are_the_oracle(shape):
    L = _volume(*shape, seed=5)
    assert _same(_products(L), so.gradient_products(L))


def test_response_is_the_oracle():
    S = np.random.RandomState(6).randn(6, 3, 5, 67).astype(np.float32) * 50
    S[:3] = np.abs(S[:3])
    assert _same(_response(S, 0.005), so.response(S, np.float32(0.005)))


def _chain(f, sigma, tau, p):
    """S84-S86 through the test entries -> H on the device"""
    from video_analytics_amd import _ffi
    L = _smooth(f, sigma, tau)
    P = _products(L.cpu().numpy())
    s = p["integration"]
    S = torch.stack([_smooth(P[c].cpu().numpy(), s * sigma, s * tau) for c in range(6)])
    return L, S, _response(S.contiguous(), p["k"])


def test_a_nan_voxel_stays_inside_the_filter_radii():
    """sigma 1 (r = 4), the derivative (1) and the integration scale (r = 8): the NaN reaches 13 voxels and no farther"""
    p = so.params(sigmas=(1.0,), taus=(1.0,))
    f = _volume(12, 12, 40, 7)
    g = f.copy()
    g[5, 6, 3] = np.nan
    _, _, Hc = _chain(f, 1.0, 1.0, p)
    _, _, Hn = _chain(g, 1.0, 1.0, p)
    Lo, So, Ho = so.harris(g, 1.0, 1.0, p)
    Hn_, Hc_ = Hn.cpu().numpy(), Hc.cpu().numpy()
    assert np.array_equal(np.isnan(Hn_), np.isnan(Ho)) and np.array_equal(_bits(np.nan_to_num(Hn_)), _bits(np.nan_to_num(Ho)))
    assert _same(Hc, so.harris(f, 1.0, 1.0, p)[2])
    assert np.isnan(Hn_[:, :, :17]).all() and np.array_equal(_bits(Hn_[:, :, 17:]), _bits(Hc_[:, :, 17:]))
    # the NaN and its neighbours are never points
    H = Hc_.copy()
    H[5, 6, 20] = np.nan
    H[5, 6, 21] = H[5, 5, 20] = H[4, 6, 20] = np.float32(3e38)
    for nb in (6, 26):
        pts, _, n = _maxima(H, 0.0, nb)
        assert n == len(so.maxima(H, 0.0, nb)) and np.array_equal(pts[:, :3], so.maxima(H, 0.0, nb))
        assert not any(abs(x - 20) + abs(y - 6) + abs(t - 5) <= 1 for x, y, t in pts[:, :3].tolist())


# ---------------------------------------------------------------- maxima (S87)

def _maxima(H, min_response, neighbours, capacity=4096, before=0, si=1, ti=2):
    """-> (points [min(n, capacity)][5], response, n found by this call); the rows behind the capacity must stay untouched"""
    from video_analytics_amd import _ffi
    T, h, w = H.shape
    d = _dev(H)
    pts = torch.full((capacity + 8, 5), -7, dtype=torch.int32, device="cuda")
    resp = torch.full((capacity + 8,), -7.0, dtype=torch.float32, device="cuda")
    counts = torch.zeros(16, dtype=torch.int32, device="cuda")
    counts[0] = before
    scratch = torch.empty(2 * T * h + 256, dtype=torch.int32, device="cuda")
    _call("va_stip_maxima", _ffi.ptr(d), T, w, h, float(min_response), neighbours, si, ti, _ffi.ptr(pts), _ffi.ptr(resp), capacity,
          _ffi.ptr(counts), _ffi.ptr(scratch))
    c = counts.cpu().numpy()
    assert c[1] == before
    n = int(c[0]) - before
    top = min(before + n, capacity)
    assert (pts[top:] == -7).all() and (resp[top:] == -7.0).all() and (pts[:before] == -7).all()
    return pts[before:top].cpu().numpy(), resp[before:top].cpu().numpy(), n


@pytest.mark.parametrize("neighbours", [6, 26])
def test_maxima_with_ties_plateaus_and_faces(neighbours):
    """a volume of five levels: plateaus and exact ties everywhere, maxima on every face, rows of 70 (two wave chunks)"""
    H = np.random.RandomState(8).randint(0, 5, size=(5, 7, 70)).astype(np.float32)
    H[0, 3, 3] = H[2, 0, 9] = H[2, 3, 0] = H[4, 6, 69] = 9.0
    H[1, 2, 30] = H[3, 4, 63] = H[3, 5, 64] = H[2, 1, 1] = 7.0  # peaks over all 26 neighbours, two of them on a diagonal
    ref = so.maxima(H, 0.0, neighbours)
    assert len(ref) >= (3 if neighbours == 26 else 10) and len(so.maxima(H, 0.0, 6)) > len(so.maxima(H, 0.0, 26))
    pts, resp, n = _maxima(H, 0.0, neighbours, before=3)
    assert n == len(ref) and np.array_equal(pts[:, :3], ref) and (pts[:, 3] == 1).all() and (pts[:, 4] == 2).all()
    assert _same(resp, H[ref[:, 2], ref[:, 1], ref[:, 0]])
    order = [(t, y, x) for x, y, t in pts[:, :3].tolist()]
    assert order == sorted(order)


def test_maxima_count_zero_and_count_above_the_capacity():
    flat = np.ones((4, 5, 6), dtype=np.float32)
    assert _maxima(flat, 0.0, 6)[2] == 0
    assert _maxima(np.ones((2, 5, 6), dtype=np.float32), 0.0, 6)[2] == 0  # no inner voxel at all
    H = np.zeros((5, 9, 70), dtype=np.float32)
    H[1:4:2, 1:8:2, 1:69:2] = 1.0
    ref = so.maxima(H, 0.0, 6)
    assert len(ref) == 2 * 4 * 34
    pts, _, n = _maxima(H, 0.0, 6, capacity=100)
    assert n == len(ref) and len(pts) == 100 and np.array_equal(pts[:, :3], ref[:100])
    assert _maxima(H, 1.0, 6)[2] == 0  # min_response is strict


@pytest.mark.parametrize("shape", [(5, 204, 9), (4, 256, 9), (5, 205, 9), (8, 205, 9)], ids=str)
def test_maxima_across_the_rounds_of_the_row_scan(shape):
    """k_stip_scan scans the T h row counts 1024 at a time: 1020 rows (short of one round), 1024 (one full round), 1025 (one
    row into a second round, a face row) and 1640, where points lie in rows of the second round and their offsets carry the
    first round's total"""
    T, h, w = shape
    H = _volume(T, h, w, seed=11)
    ref = so.maxima(H, 0.0, 6)
    assert 100 < len(ref) < 4096
    assert ((ref[:, 2] * h + ref[:, 1] >= 1024).sum() > 100) == (T * h > 1025)
    pts, resp, n = _maxima(H, 0.0, 6, before=5)
    assert n == len(ref) and np.array_equal(pts[:, :3], ref)
    assert _same(resp, H[ref[:, 2], ref[:, 1], ref[:, 0]])


# ---------------------------------------------------------------- votes and cuboids (S88-S89)

def _votes(L, flow, p):
    from video_analytics_amd import _ffi
    T, h, w = L.shape
    dl, df = _dev(L), _dev(flow)
    hog = torch.full((T, p.bins, h, w), -1, dtype=torch.int32, device="cuda")
    hof = torch.full((T, p.bins, h, w), -1, dtype=torch.int32, device="cuda")
    _call("va_stip_votes", _ffi.ptr(dl), _ffi.ptr(df), T, w, h, ctypes.byref(p), _ffi.ptr(hog), _ffi.ptr(hof))
    return hog, hof


@pytest.mark.parametrize("bins", [4, 8, 6, 2])
def test_votes_are_the_oracle(bins):
    """ramps along the axes and the diagonals (the seams of the bins), a flat patch, flow with zeros, a NaN, an infinity and
    vectors beyond VMAX"""
    T, h, w = 3, 9, 37
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    L = _volume(T, h, w, 9)
    L[0] = 3 * xs
    L[1, :, :12] = 50.0
    L[1, :, 12:24] = (2 * (xs + ys))[:, 12:24]
    L[1, :, 24:] = (5 * ys)[:, 24:]
    L[2, 4, 4] = 4000.0  # a gradient beyond VMAX
    flow = np.random.RandomState(10).randn(T - 1, 2, h, w).astype(np.float32) * 3
    flow[0, :, 0, :4] = 0.0
    flow[0, :, 1, :4] = np.float32([[3, -3, 3, -3], [3, 3, -3, -3]])
    flow[0, :, 2, :4] = np.float32([[2, -2, 0, 0], [0, 0, 2, -2]])
    flow[1, 0, 3, 3] = np.nan
    flow[1, 1, 3, 5] = np.inf
    flow[1, :, 5, :3] = np.float32([[100, -250, 1e30], [30, 10, 1e30]])
    p = _params(bins=bins, nt=1)
    hog, hof = _votes(L, flow, p)
    rh, rf = so.votes_hog(L, bins), so.votes_hof(flow, bins)
    assert int(rh.max()) == 2 ** 17 == int(rf.max())
    assert _same(hog, rh) and _same(hof, rf)
    assert np.array_equal(_bits(hof[2]), _bits(hof[1]))  # the last pair's field stands in for the last frame


def _describe(points, hogI, hofI, p):
    from video_analytics_amd import _ffi
    T, bins, h1, w1 = hogI.shape
    d = _dev(np.asarray(points, dtype=np.int32))
    a, b = _dev(hogI.view(np.int32)), _dev(hofI.view(np.int32))
    dim = 2 * p.nx * p.ny * p.nt * p.bins
    out = torch.full((len(points), dim), float("nan"), dtype=torch.float32, device="cuda")
    _call("va_stip_describe", _ffi.ptr(d), len(points), _ffi.ptr(a), _ffi.ptr(b), T, w1 - 1, h1 - 1, ctypes.byref(p), _ffi.ptr(out))
    return out


@pytest.mark.parametrize("over", [dict(), dict(nx=2, ny=4, nt=3, bins=8), dict(nx=8, ny=8, nt=1, bins=4)], ids=["3x3x2x4", "2x4x3x8", "8x8x1x4"])
def test_cuboids_are_the_oracle(over):
    """votes over their whole range, and four words far beyond it that make the integral planes wrap mod 2^32; cuboids that leave
    the volume on every side, cuboids with empty cells, and points whose whole cuboid holds nothing"""
    T, h, w = 9, 40, 48
    op = so.params(**over)
    bins = op["bins"]
    rs = np.random.RandomState(11)
    hog = rs.randint(0, 2 ** 17 + 1, size=(T, bins, h, w)).astype(np.uint32)
    hof = rs.randint(0, 2 ** 17 + 1, size=(T, bins, h, w)).astype(np.uint32)
    hog[:, :, :21, :21] = 0
    hof[:, :, :21, :21] = 0
    hog[:, 0, 30, 40] = hog[:, 0, 35, 10] = hof[:, 1, 22, 22] = hof[:, 1, 38, 2] = 3000000000  # (no vote: the planes' sums wrap)
    hogI, hofI = so.integral(hog), so.integral(hof)
    assert int(hog[0, 0].astype(np.uint64).sum()) > 2 ** 32 and int(hogI[0, 0, -1, -1]) < 2 ** 31
    pts = [(24, 20, 4, 0, 0), (0, 0, 0, 5, 1), (47, 39, 8, 5, 1), (0, 39, 8, 2, 0), (47, 0, 0, 3, 1), (1, 1, 4, 0, 0),
           (-500, 3, 3, 0, 0), (3, 3, 40, 1, 1), (2, 2, 2, 0, 0), (30, 5, 1, 1, 0)]
    p = _params(over)
    got = _describe(pts, hogI, hofI, p)
    ref = so.describe(pts, hogI, hofI, op)
    assert _same(got, ref)
    assert (ref[6] == 0).all() and (ref[7] == 0).all() and (ref[0] != 0).any()  # zero descriptors beside others
    if not over:
        assert (ref[8] == 0).all()  # inside the volume, over the region without votes
        sums = so.cuboid_sums(pts[1], hogI, hofI, op)
        assert 0 in sums and max(sums) > 0  # empty cells beside full ones


# ---------------------------------------------------------------- end to end

def _check_extract(name, gray, flow, p_over, **kw):
    from video_analytics_amd import stip
    _, _, _, op, _, pts, resp, desc, _ = host.case(name)
    out = stip.space_time_interest_points(_dev(gray), None if flow is None else _dev(flow), **dict(p_over, **kw))
    assert out["count"] == len(pts) >= 20
    assert np.array_equal(out["points"].cpu().numpy(), pts)
    assert _same(out["response"], resp) and _same(out["desc"], desc)
    return out


@pytest.mark.parametrize("tiles", TILES[:2], ids=TILE_IDS[:2])
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
def test_extract_defaults_with_planted_flow(u8, tiles):
    """all twelve scale pairs on 48 x 40 x 12: radii up to 91, larger than every axis"""
    gray, flow = host.case("defaults")[:2]
    _check_extract("defaults", gray if u8 else gray.astype(np.float32), flow, tiles)


def test_extract_single_pair_with_planted_flow():
    gray, flow = host.case("single")[:2]
    out = _check_extract("single", gray, flow, host.SINGLE, max_points=64)
    assert out["points"][:, 3:].abs().max() == 0


def test_extract_with_farneback_flow():
    """flow=None computes Farneback on the frames, once; the oracle gets that field"""
    from video_analytics_amd import flow as vflow, stip
    gray = host.case("single")[0]
    op = host.case("single")[3]
    g = _dev(gray)
    fl = vflow.farneback_flow(g)
    pts, resp, desc = so.extract(gray, fl.cpu().numpy(), op)
    out = stip.space_time_interest_points(g, **host.SINGLE)
    assert out["count"] == len(pts) >= 20 and np.array_equal(out["points"].cpu().numpy(), pts)
    assert _same(out["response"], resp) and _same(out["desc"], desc)
    again = stip.space_time_interest_points(g, fl, **host.SINGLE)
    assert torch.equal(again["desc"], out["desc"]) and torch.equal(again["points"], out["points"])


def test_extract_refuses_by_name():
    from video_analytics_amd import _ffi, stip
    gray, flow = host.case("defaults")[:2]
    g, f = _dev(gray), _dev(flow)
    with pytest.raises(ValueError, match="found 3[0-9] points, more than max_points = 5"):
        stip.space_time_interest_points(g, f, max_points=5)
    with pytest.raises(ValueError, match="gray must be a CUDA tensor"):
        stip.space_time_interest_points(torch.from_numpy(gray), f)
    with pytest.raises(ValueError, match="uint8 or float32"):
        stip.space_time_interest_points(g.double(), f)
    with pytest.raises(ValueError, match="at least 2 frames"):
        stip.space_time_interest_points(g[:1], f)
    with pytest.raises(ValueError, match="flow must be a float32 \\[11,2,40,48\\]"):
        stip.space_time_interest_points(g, f[:5])
    with pytest.raises(ValueError, match="flow_params"):
        stip.space_time_interest_points(g, f, flow_params=_ffi.default_tvl1_params())
    with pytest.raises(ValueError, match="not both"):
        stip.space_time_interest_points(g, f, params=_ffi.default_stip_params(), bins=8)
    with pytest.raises(ValueError, match="unknown"):
        stip.space_time_interest_points(g, f, sigma=3)
    with pytest.raises(ValueError, match="max_points must be >= 1"):
        stip.space_time_interest_points(g, f, max_points=0)
    with pytest.raises(ValueError, match="MEMORY_BUDGET_BYTES"):
        stip.space_time_interest_points(torch.zeros((400, 240, 320), dtype=torch.uint8, device="cuda"),
                                        torch.zeros((1, 2, 240, 320), device="cuda").expand(399, 2, 240, 320))
    # the C entry itself
    L = _ffi.lib()
    p = _ffi.default_stip_params()
    cnt = ctypes.c_int(0)
    ws = torch.empty(256, dtype=torch.uint8, device="cuda")
    out = torch.empty(64, dtype=torch.float32, device="cuda")

    def call(pp, T=12, w=48, h=40, cap=1):
        return L.va_stip_extract(_ffi.ctx(0), _ffi.ptr(g), 1, _ffi.ptr(f), T, w, h, ctypes.byref(pp), _ffi.ptr(out), _ffi.ptr(out),
                                 _ffi.ptr(out), cap, ctypes.byref(cnt), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(torch.device("cuda", 0)))
    for kw, text in ((dict(T=1), "n_frames must be in \\[2,65535\\], got 1"), (dict(w=0), "frame size 0 x 40"),
                     (dict(cap=0), "capacity must be >= 1, got 0"), (dict(), "workspace of 256 bytes, need")):
        with pytest.raises(ValueError, match=text):
            _ffi.check(call(p, **kw))
    bad = _ffi.default_stip_params()
    bad.nx = 9
    with pytest.raises(ValueError, match="nx must be in \\[1,8\\], got 9"):
        _ffi.check(call(bad))
    bad = _ffi.default_stip_params()
    bad.struct_bytes = 8
    with pytest.raises(ValueError, match="struct_bytes is 8"):
        _ffi.check(call(bad))
