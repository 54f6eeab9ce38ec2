"""Dense trajectories on the GPU, bit for bit against the float32 / integer oracle (tests/dtraj_oracle.py):
every stage alone through its test entry (``va_dtraj_votes`` ... ``va_dtraj_finish``), then ``dense_trajectories`` end to end
under several chunk lengths and tile shapes.  Every comparison is ``torch.equal``."""
import ctypes

import numpy as np
import pytest
import torch

import dtraj_oracle as do
import dtraj_scenes as scenes

pytestmark = pytest.mark.gpu

TILES = [dict(), dict(votes_tile_w=23, votes_tile_h=3)]
TILE_IDS = ["default", "23x3"]


def _ffi_params(p, **tuning):
    from video_analytics_amd import _ffi
    return _ffi.default_dense_traj_params(**dict(p, **tuning))


def _call(name, *args):
    from video_analytics_amd import _ffi
    _ffi.check(getattr(_ffi.lib(), name)(_ffi.ctx(0), *args, _ffi.stream_ptr(torch.device("cuda", 0))))
    torch.cuda.synchronize()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(t):
    """a device tensor of 32-bit words as numpy uint32"""
    return t.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------- votes (S69-S71)

_vote_ref = {}


def _vote_case(n, w, h):
    """gray with a flat patch (zero gradients), ramps along x, along y and along the diagonal (the seams of the octants); flow
    from a texture with exact zeros, vectors at and one float on either side of min_flow, a NaN, an infinity, and vectors and
    flow gradients far beyond VMAX; the oracle's votes.  Computed once per shape, never changed."""
    key = (n, w, h)
    if key not in _vote_ref:
        p = do.params()
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
        gray = scenes.texture(n, w, h, 11 * w + h)
        gray[0, :h // 2, :w // 3] = 50.0
        gray[0, :h // 2, w // 3:2 * w // 3] = (3 * xs)[:h // 2, w // 3:2 * w // 3]
        gray[0, h // 2:, :w // 3] = (5 * ys)[h // 2:, :w // 3]
        gray[0, h // 2:, w // 3:2 * w // 3] = (2 * (xs + ys))[h // 2:, w // 3:2 * w // 3]
        flow = (scenes.texture(2 * n, w, h, 13 * w + h).reshape(n, 2, h, w) - 128.0) / np.float32(32.0)
        f = flow[0]
        mf = np.float32(p["min_flow"])
        f[:, 0:3, 0:4] = 0.0
        f[:, 5, 1:4] = np.float32([[mf, np.nextafter(mf, np.float32(0)), np.nextafter(mf, np.float32(1))], [0, 0, 0]])
        f[:, 7, 1:4] = np.float32([[0, 0, 0], [-mf, -np.nextafter(mf, np.float32(0)), -np.nextafter(mf, np.float32(1))]])
        f[:, 9, 2:6] = np.float32([[3, -3, 3, -3], [3, 3, -3, -3]])  # the diagonals
        f[:, 11, 2:6] = np.float32([[2, -2, 0, 0], [0, 0, 2, -2]])   # the axes
        f[0, h - 4, 3] = np.nan
        f[1, h - 4, w - 5] = np.inf
        f[:, h - 8, w - 6:w - 2] = np.float32([[100, -250, 40, 1e30], [30, 10, -40, 1e30]])  # votes beyond VMAX, a length beyond float32
        flow = np.ascontiguousarray(flow.astype(np.float32))
        ref = np.stack([do.votes(gray[i], flow[i, 0], flow[i, 1], p) for i in range(n)])
        top = int(do.FLOW_VMAX * 2 ** do.FLOW_SHIFT)
        assert (ref[:, 8:16] == top).any() and (ref[:, 17:33] == top).any() and (ref[0, 16] > 0).any()  # the clamp is reached
        _vote_ref[key] = (gray, flow, ref)
    return _vote_ref[key]


@pytest.mark.parametrize("tiles", TILES, ids=TILE_IDS)
@pytest.mark.parametrize("gray_u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("n,w,h", [(3, 37, 29), (1, 16, 16)])
def test_votes_are_the_oracle(n, w, h, gray_u8, tiles):
    """37 x 29: ragged tiles on all four sides, three frames (a wrong plane or frame stride shows); 16 x 16: the smallest"""
    from video_analytics_amd import _ffi
    gray, flow, ref = _vote_case(n, w, h)
    if gray_u8:
        gray = np.rint(gray).astype(np.uint8)
        ref = np.stack([do.votes(gray[i], flow[i, 0], flow[i, 1], do.params()) for i in range(n)])
    p = _ffi_params({}, **tiles)
    g, f = _dev(gray), _dev(flow)
    out = torch.full((n, 33, h, w), -1, dtype=torch.int32, device="cuda")
    _call("va_dtraj_votes", _ffi.ptr(g), int(gray_u8), _ffi.ptr(f), n, w, h, ctypes.byref(p), _ffi.ptr(out))
    assert torch.equal(out.cpu(), torch.from_numpy(ref.view(np.int32)))
    assert torch.equal(g.cpu(), torch.from_numpy(gray)) and np.array_equal(f.cpu().numpy().view(np.uint32), flow.view(np.uint32))


# ---------------------------------------------------------------- integral planes (S72)

@pytest.mark.parametrize("h", [1, 5, 67])
@pytest.mark.parametrize("w", [1, 63, 64, 65, 257])
def test_integral_planes_are_exact_mod_2_32(w, h):
    """widths on either side of a wave's 64 lanes and of the carried prefix, three planes of full-range words: every running
    sum wraps"""
    from video_analytics_amd import _ffi
    q = np.random.RandomState(100 * w + h).randint(0, 2 ** 32, size=(3, h, w), dtype=np.uint64).astype(np.uint32)
    ref = do.integral(q)
    assert w * h < 4 or int(q.astype(np.uint64).sum()) > 2 ** 32
    d = _dev(q.view(np.int32))
    out = torch.full((3, h + 1, w + 1), -1, dtype=torch.int32, device="cuda")
    _call("va_dtraj_integral", _ffi.ptr(d), 3, w, h, _ffi.ptr(out))
    assert torch.equal(out.cpu(), torch.from_numpy(ref.view(np.int32)))


# ---------------------------------------------------------------- the track table

class Table:
    """the state buffer of va_dtraj_state_layout, filled from and read back into the oracle's track dicts"""

    def __init__(self, w, h, p, fp):
        from video_analytics_amd import _ffi
        self.w, self.h, self.p, self.fp = w, h, p, fp
        self.nbytes, self.off = _ffi.dtraj_state_layout(w, h, fp)
        self.ncx = w // p["step"]
        self.cells = self.ncx * (h // p["step"])
        self.L = p["length"]
        self.slots = self.cells * self.L
        self.accn = p["nt"] * p["nxy"] ** 2 * 33
        # garbage everywhere except the counts and the occupancy marks, which are 0 between calls
        self.host = np.random.RandomState(1).randint(0, 256, size=self.nbytes).astype(np.uint8)
        self.region("counts", np.int32, 16)[:] = 0
        self.region("occupancy", np.int32, self.cells)[:] = 0
        self.buf = None

    def region(self, name, dtype, count, host=None):
        host = self.host if host is None else host
        return host[self.off[name]:self.off[name] + count * np.dtype(dtype).itemsize].view(dtype)

    def slot_of(self, t):
        x, y = t["pts"][0]
        return (t["start"] % self.L) * self.cells + (int(y) // self.p["step"]) * self.ncx + int(x) // self.p["step"]

    def put(self, tracks, stat=None, slots=None):
        """tracks (oracle dicts) into list 0; their slots are those of their first point unless given"""
        slots = [self.slot_of(t) for t in tracks] if slots is None else slots
        assert len(set(slots)) == len(slots) and max(slots, default=0) < self.slots
        self.region("counts", np.int32, 16)[:2] = (len(tracks), 0)
        self.region("lists", np.int32, 2 * self.slots)[:len(tracks)] = slots
        if stat is not None:
            self.region("status", np.int32, self.slots)[:len(tracks)] = stat
        start = self.region("start", np.int32, self.slots)
        pts = self.region("points", np.float32, self.slots * (self.L + 1) * 2).reshape(self.slots, self.L + 1, 2)
        acc = self.region("sums", np.uint64, self.slots * self.accn).reshape(self.slots, self.accn)
        for t, s in zip(tracks, slots):
            start[s] = t["start"]
            pts[s, :len(t["pts"])] = np.array(t["pts"], dtype=np.float32)
            acc[s] = t["acc"].reshape(-1)
        self.buf = torch.from_numpy(self.host).cuda()
        return slots

    def get(self):
        back = self.buf.cpu().numpy()
        counts = self.region("counts", np.int32, 16, back).copy()
        lists = self.region("lists", np.int32, 2 * self.slots, back).reshape(2, self.slots)
        return dict(counts=counts, live=lists[counts[1] & 1][:counts[0]].copy(),
                    status=self.region("status", np.int32, self.slots, back).copy(),
                    start=self.region("start", np.int32, self.slots, back).copy(),
                    points=self.region("points", np.float32, self.slots * (self.L + 1) * 2, back).reshape(self.slots, self.L + 1, 2).copy(),
                    sums=self.region("sums", np.uint64, self.slots * self.accn, back).reshape(self.slots, self.accn).copy(),
                    occupancy=self.region("occupancy", np.int32, self.cells, back).copy())


# ---------------------------------------------------------------- corner response and sampling (S73-S74)

@pytest.mark.parametrize("gray_u8", [True, False], ids=["u8", "f32"])
def test_corner_response_and_its_maximum(gray_u8):
    from video_analytics_amd import _ffi
    n, w, h = 2, 40, 30
    gray = scenes.texture(n, w, h, 21)
    gray[1, 10:, :] = 77.0  # a flat region: responses of exactly 0
    if gray_u8:
        gray = np.rint(gray).astype(np.uint8)
    refs = [do.corner(gray[i]) for i in range(n)]
    g = _dev(gray)
    resp = torch.full((n, h, w), float("nan"), dtype=torch.float32, device="cuda")
    mx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    _call("va_dtraj_corner", _ffi.ptr(g), int(gray_u8), n, w, h, _ffi.ptr(resp), _ffi.ptr(mx))
    assert np.array_equal(_u32(resp), np.stack([r[0] for r in refs]).view(np.uint32))
    assert _u32(mx).tolist() == [r[1] for r in refs]
    assert (refs[1][0] == 0).any() and all(r[1] > 0 for r in refs)


def test_sample_appends_the_free_cells_in_raster_order():
    """40 x 30 with step 5: live tracks hold some cells -- one sits exactly on a cell boundary (x = 9.5 belongs to pixel 10, the
    next cell), two share a cell, one has moved since it started -- and the new tracks follow them in raster order"""
    from video_analytics_amd import _ffi
    w, h, frame = 40, 30, 3
    p = do.params()
    fp = _ffi_params({})
    gray = np.rint(scenes.texture(1, w, h, 22)[0]).astype(np.uint8)
    gray[:12, 22:] = 90  # flat: these cells start nothing
    resp, mb = do.corner(gray)
    tracks = [do.new_track(2, 2, 2, p), do.new_track(2, 7, 2, p), do.new_track(2, 12, 12, p), do.new_track(1, 17, 12, p),
              do.new_track(1, 32, 27, p)]
    for t, pts in zip(tracks, ([(9.5, 2.0)], [(14.49, 3.0)], [(21.0, 17.0)], [(20.0, 17.2), (22.0, 18.0)], [(36.0, 27.0), (39.4, 29.4)])):
        t["pts"] += [(np.float32(x), np.float32(y)) for x, y in pts]
    tab = Table(w, h, p, fp)
    old = tab.put(tracks)
    want = do.sample(list(tracks), resp, mb, frame, p)
    new = want[len(tracks):]
    assert 10 <= len(new) < tab.cells - 4  # some cells are free and start a track, some are held, some are flat
    r, m = _dev(resp), _dev(np.array([mb], dtype=np.uint32).view(np.int32))
    _call("va_dtraj_sample", _ffi.ptr(r), _ffi.ptr(m), w, h, frame, ctypes.byref(fp), _ffi.ptr(tab.buf))
    got = tab.get()
    assert got["counts"][0] == len(want) and got["counts"][1] == 0
    assert got["live"].tolist() == old + [tab.slot_of(t) for t in new]
    cells_held = {(2, 0), (4, 3), (7, 5)}  # by (9.5, 2) and (14.49, 3); by the two at (21, 17), (22, 18); by (39.4, 29.4)
    assert {(int(t["pts"][0][0]) // 5, int(t["pts"][0][1]) // 5) for t in new}.isdisjoint(cells_held)
    for t in new:
        s = tab.slot_of(t)
        assert got["start"][s] == frame and got["points"][s, 0].tolist() == [float(t["pts"][0][0]), float(t["pts"][0][1])]
    assert not got["occupancy"].any()


# ---------------------------------------------------------------- step (S75)

_step_ref = {}


def _step_case(patch, nxy):
    key = (patch, nxy)
    if key not in _step_ref:
        w, h, frame = 40, 30, 7
        p = do.params(length=6, nt=3, patch=patch, nxy=nxy)
        rs = np.random.RandomState(patch)
        gray = scenes.texture(1, w, h, 31)[0]
        flow = ((scenes.texture(2, w, h, 32) - 128.0) / 40.0).astype(np.float32)
        I = do.integral(do.votes(gray, flow[0], flow[1], p))
        med = np.zeros((2, h, w), dtype=np.float32)
        # (current point, median flow there, steps done): corners and edges, leaving on each side, a NaN, the last step
        spec = [((0, 0), (0.5, 0.25), 0), ((39, 0), (-1.5, 1.0), 1), ((0, 29), (1.0, -1.0), 2), ((39, 29), (-0.5, -0.5), 3),
                ((20, 0), (0.0, 0.0), 4), ((0, 15), (2.0, 0.0), 0), ((39, 14), (-3.0, 1.0), 1), ((19, 29), (0.0, -2.0), 5),
                ((1, 10), (-1.5, 0.0), 2), ((38, 11), (1.5, 0.0), 3), ((10, 1), (0.0, -1.5), 4), ((11, 28), (0.0, 1.5), 5),
                ((25, 20), (np.nan, 0.0), 1), ((26, 9), (0.0, np.inf), 2), ((15.5, 15.5), (1.25, -0.75), 5), ((30.49, 5.51), (39.0 - 30.49, 0.0), 0)]
        tracks, slots = [], []
        for i, ((x, y), (mu, mv), k) in enumerate(spec):
            t = do.new_track(frame - k, 0, 0, p)
            t["pts"] = [(np.float32(rs.rand() * 39), np.float32(rs.rand() * 29)) for _ in range(k)] + [(np.float32(x), np.float32(y))]
            t["acc"][:k // 2 + (1 if k % 2 else 0)] = rs.randint(0, 2 ** 40, size=t["acc"][:k // 2 + (1 if k % 2 else 0)].shape).astype(np.uint64)
            rx, ry = do.nearest(x, w), do.nearest(y, h)
            med[:, ry, rx] = (mu, mv)
            tracks.append(t)
            slots.append(((frame - k) % 6) * 48 + 3 * i)
        before = [dict(t, pts=list(t["pts"]), acc=t["acc"].copy()) for t in tracks]
        stat = do.step(tracks, I, med, frame, p)
        assert {do.ALIVE, do.LEFT, do.DONE} == set(stat) and stat.count(do.LEFT) >= 6
        _step_ref[key] = (w, h, frame, p, I, med, before, slots, tracks, stat)
    return _step_ref[key]


@pytest.mark.parametrize("patch,nxy", [(16, 2), (12, 3)])
def test_step_adds_the_slice_and_moves(patch, nxy):
    from video_analytics_amd import _ffi
    w, h, frame, p, I, med, before, slots, after, stat = _step_case(patch, nxy)
    fp = _ffi_params(dict(length=6, nt=3, patch=patch, nxy=nxy))
    tab = Table(w, h, p, fp)
    # the temporal cell a track enters at this step holds garbage on the device: the step must store, not add
    dirty = [dict(t, acc=t["acc"].copy()) for t in before]
    for t in dirty:
        k = frame - t["start"]
        if k % 2 == 0:
            t["acc"][k // 2:] = np.uint64(0xDEADBEEFDEADBEEF)
    tab.put(dirty, slots=slots)
    dI, dm = _dev(I.view(np.int32)), _dev(med)
    _call("va_dtraj_step", _ffi.ptr(dI), _ffi.ptr(dm), w, h, frame, ctypes.byref(fp), _ffi.ptr(tab.buf))
    got = tab.get()
    assert got["status"][:len(stat)].tolist() == stat and got["counts"][0] == len(stat)
    for t, s, st in zip(after, slots, stat):
        k = frame - t["start"]
        tc = k // 2
        n = (tc + 1) * nxy * nxy * 33
        assert np.array_equal(got["sums"][s][:n], t["acc"].reshape(-1)[:n]), (s, k)
        if st != do.LEFT:
            assert got["points"][s, :k + 2].view(np.uint32).tolist() == np.array(t["pts"], dtype=np.float32).view(np.uint32).tolist()
    assert np.array_equal(_u32(dI), I) and np.array_equal(_u32(dm), med.view(np.uint32))


# ---------------------------------------------------------------- finish (S76)

_finish_ref = {}


def _finish_case():
    if not _finish_ref:
        w, h = 160, 160
        p = do.params(length=6, nt=3, patch=16)
        rs = np.random.RandomState(4)

        def walk(x0, y0, steps):
            pts = [(np.float32(x0), np.float32(y0))]
            for dx, dy in steps:
                pts.append((np.float32(pts[-1][0] + np.float32(dx)), np.float32(pts[-1][1] + np.float32(dy))))
            return pts

        paths = [
            ("valid", walk(10, 10, [(2, 1)] * 6)), ("static", walk(30, 30, [(0.1, -0.1)] * 6)), ("alive", walk(5, 5, [(1, 1)] * 3)),
            ("erratic", walk(2, 80, [(19.5, 0.25)] * 6)), ("valid", walk(50, 50, [(1.5, -2.25), (2.5, 0.5), (0.75, 3), (3, 3), (1, 2), (2, 2)])),
            ("left", walk(1, 1, [(1, 0)] * 2)), ("jump", walk(60, 20, [(1, 1), (1, 1), (21, 0), (1, 1), (1, 1), (1, 1)])),
            ("jump", walk(70, 90, [(0.5, 0), (0.5, 0), (0.5, 0), (10, 0), (0.5, 0), (0.5, 0)])), ("alive", walk(100, 100, [(0, 1)] * 5)),
            ("valid", walk(120, 40, [(-3, 0.5)] * 6)), ("static", walk(9, 140, [(0, 0)] * 6)), ("valid", walk(140, 140, [(0.3, 3.1)] * 6)),
        ]
        tracks, stat = [], []
        for i, (kind, pts) in enumerate(paths):
            t = do.new_track(20 - (len(pts) - 1), 0, 0, p)
            t["pts"] = pts
            t["acc"][:] = rs.randint(0, 2 ** 34, size=t["acc"].shape).astype(np.uint64)
            if i == 4:
                t["acc"][:, :, 8:17] = 0  # a flow histogram of nothing: the block stays zero
            tracks.append(t)
            stat.append({"alive": do.ALIVE, "left": do.LEFT}.get(kind, do.DONE))
        slots = [((t["start"]) % 6) * 1024 + 5 * i for i, t in enumerate(tracks)]
        found, rej = [], [0, 0, 0, 0, 0]
        alive = do.finish(tracks, stat, p, found, rej)
        # the conditions of the test, on the oracle's answer: every rule fires, the share rule on its own, three or more pass
        assert rej == [1, 2, 1, 2, 0] and len(found) == 4 and len(alive) == 2
        assert do.classify(paths[7][1], p)[0] == 3 and max(abs(b[0] - a[0]) for a, b in zip(paths[7][1], paths[7][1][1:])) < p["max_dis"]
        assert not found[1][0][12 + 96:12 + 204].any() and found[1][0][12:12 + 96].any()
        _finish_ref["case"] = (w, h, p, tracks, stat, slots, found, rej, [slots[2], slots[8]])
    return _finish_ref["case"]


def test_finish_tests_normalises_and_compacts():
    from video_analytics_amd import _ffi
    w, h, p, tracks, stat, slots, found, rej, alive_slots = _finish_case()
    fp = _ffi_params(dict(length=6, nt=3, patch=16))
    tab = Table(w, h, p, fp)
    tab.region("counts", np.int32, 16)[2] = 3  # three trajectories were found before this frame
    tab.put(tracks, stat=stat, slots=slots)
    cap, dim = 8, do.descriptor_length(p)
    desc = torch.full((cap, dim), float("nan"), dtype=torch.float32, device="cuda")
    pts = torch.full((cap, 7, 2), float("nan"), dtype=torch.float32, device="cuda")
    starts = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    _call("va_dtraj_finish", w, h, ctypes.byref(fp), _ffi.ptr(tab.buf), _ffi.ptr(desc), _ffi.ptr(pts), _ffi.ptr(starts), cap)
    got = tab.get()
    assert got["counts"][:8].tolist() == [2, 1, 3 + len(found), 3] + rej[:4]
    assert got["live"].tolist() == alive_slots
    assert torch.equal(desc[3:7].cpu(), torch.from_numpy(np.stack([f[0] for f in found])))
    assert torch.equal(pts[3:7].cpu(), torch.from_numpy(np.stack([f[1] for f in found])))
    assert starts[3:7].cpu().tolist() == [f[2] for f in found]
    assert torch.isnan(desc[:3]).all() and torch.isnan(desc[7:]).all() and starts[7].item() == -1  # nothing else is written


# ---------------------------------------------------------------- end to end

PLANTED = dict(length=6, nt=3, patch=16)
_e2e = {}


def _planted_reference():
    if "planted" not in _e2e:
        gray, flow, _ = scenes.planted()
        ref = do.extract(gray, flow, do.median3(flow), do.params(**PLANTED))
        _e2e["planted"] = (gray, flow, ref)
    return _e2e["planted"]


def _same(out, ref):
    assert out["count"] == ref["count"] and out["rejected"] == ref["rejected"]
    assert torch.equal(out["desc"].cpu(), torch.from_numpy(ref["desc"]))
    assert torch.equal(out["points"].cpu(), torch.from_numpy(ref["points"]))
    assert torch.equal(out["start"].cpu(), torch.from_numpy(ref["start"]))


@pytest.mark.parametrize("tiles", TILES, ids=TILE_IDS)
@pytest.mark.parametrize("chunk", [0, 1, 4], ids=["chunk-default", "chunk-1", "chunk-4"])
def test_end_to_end_with_planted_flow(chunk, tiles):
    """12 frames of 80 x 64; chunks of 8 + 3 (the default), of 1, and of 4 + 4 + 3 frames: the same bits"""
    from video_analytics_amd import trajectories
    gray, flow, ref = _planted_reference()
    assert ref["count"] >= 50 and len(ref["started_frames"]) >= 3  # conditions of the test, not measurements
    assert len(set((ref["start"]).tolist())) >= 2                    # trajectories end at different frames: the output order shows
    g, f = _dev(gray), _dev(flow)
    out = trajectories.dense_trajectories(g, f, params=_ffi_params(PLANTED, chunk_frames=chunk, **tiles))
    _same(out, ref)
    assert out["desc"].shape == (ref["count"], 2 * 6 + 33 * 12)
    assert torch.equal(g.cpu(), torch.from_numpy(gray)) and torch.equal(f.cpu(), torch.from_numpy(flow))  # inputs untouched


def test_end_to_end_with_farneback_flow():
    """flow=None: Farneback flow of the frames; the oracle receives the device's flow and filters it itself (S55's rule)"""
    from video_analytics_amd import flow as vflow
    from video_analytics_amd import trajectories
    gray, _, _ = _planted_reference()
    g = _dev(gray)
    out = trajectories.dense_trajectories(g, **PLANTED)
    fl = vflow.farneback_flow(g).cpu().numpy()
    ref = do.extract(gray, fl, do.median3(fl), do.params(**PLANTED))
    print("Farneback flow: %d trajectories, rejected %s" % (ref["count"], ref["rejected"]))
    _same(out, ref)
    assert sum(ref["rejected"].values()) + ref["count"] > 100  # tracks were followed


def test_capacity_is_never_exceeded_silently():
    from video_analytics_amd import trajectories
    gray, flow, ref = _planted_reference()
    g, f = _dev(gray), _dev(flow)
    with pytest.raises(ValueError, match="found %d trajectories" % ref["count"]):
        trajectories.dense_trajectories(g, f, max_trajectories=ref["count"] - 1, **PLANTED)
    _same(trajectories.dense_trajectories(g, f, max_trajectories=ref["count"], **PLANTED), ref)


def test_uint8_and_float32_frames_give_the_same_result():
    from video_analytics_amd import trajectories
    gray, flow, ref = _planted_reference()
    g8, f = _dev(gray), _dev(flow)
    g32 = g8.float()
    keep = g32.clone()
    _same(trajectories.dense_trajectories(g32, f, **PLANTED), ref)
    _same(trajectories.dense_trajectories(g8, f, **PLANTED), ref)
    assert torch.equal(g32, keep) and torch.equal(g8.cpu(), torch.from_numpy(gray))


def test_wrong_inputs_are_refused_by_name(monkeypatch):
    from video_analytics_amd import _ffi, trajectories
    gray, flow, _ = _planted_reference()
    g, f = _dev(gray), _dev(flow)
    assert trajectories.trajectory_bound(80, 64, 12, _ffi_params(PLANTED)) == 16 * 12 * 6
    with monkeypatch.context() as m:  # the outputs of the bound (1152 trajectories) do not fit: said by name, nothing is launched
        m.setattr(trajectories, "MEMORY_BUDGET_BYTES", 1 << 20)
        with pytest.raises(ValueError, match="MEMORY_BUDGET_BYTES.*max_trajectories"):
            trajectories.dense_trajectories(g, f, **PLANTED)
        assert trajectories.dense_trajectories(g, f, max_trajectories=200, **PLANTED)["count"] > 0
    for args, kw, msg in (((g.cpu(), f), {}, "CUDA"), ((g[:1], None), {}, "at least 2 frames"), ((g, f[:-1]), {}, "flow must be"),
                          ((g, f), dict(flow_params=_ffi.default_farneback_params()), "flow_params"),
                          ((g, f), dict(params=_ffi.default_dense_traj_params(), length=6), "not both"),
                          ((g, f), dict(max_trajectories=0), "max_trajectories"), ((g, f), dict(length=7), "length")):
        with pytest.raises(ValueError, match=msg):
            trajectories.dense_trajectories(*args, **kw)
