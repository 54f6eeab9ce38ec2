"""Farneback optical flow on the GPU AWAY from the parameters of tests/test_farneback_gpu.py and AT every limit of its two
kernels: windows of 3 and 5 (narrower than the border weights) and of 59, 61 and 63 (the LDS limit and the halved tile),
tiles of 1 x 1, the polynomial expansion with more than 64 KB of LDS and with poly_sigma 0.6 and 3, odd iteration counts
(the flow upsampled from planes 2, 3), pyr_scale with an inexact inverse, one to sixteen levels, the frame mapping with two
and four frames per sequence, and frame content the synthetic clips never produce.

Same bar as tests/test_farneback_gpu.py: BIT-EXACT against the float32 oracle (tests/farneback_oracle.py) under every tile
shape.  The oracle is pinned to its float64 witness at these parameters in tests/test_farneback_host.py.  Every test first
asserts that the oracle's result is finite, so that no NaN can sit on both sides of a comparison, and asserts through
tests/flow_shapes.py that the case runs the tile it is named for.
"""
import ctypes

import numpy as np
import pytest
import torch

import farneback_oracle as fo
import flow_shapes as fs
from test_farneback_gpu import BASE, _incoming, _texture

pytestmark = pytest.mark.gpu

N = 3  # fields or pairs per stage call: a wrong stride shows


def _tiles(prefix, tile):
    return {prefix + "_tile_w": tile[0], prefix + "_tile_h": tile[1]} if tile != (0, 0) else {}


# ------------------------------------------------------------------------------------------------ a. one pass

_pass_in = {}
_pass_ref = {}


def _pass_reference(w, h, winsize, gaussian, kind):
    """coefficient planes the oracle produced (shared by every window), an incoming flow, and the oracle's pass on them"""
    if (w, h) not in _pass_in:
        f = _texture(2 * N, w, h, 5 * w + h)
        r = np.stack([fo.polyexp(f[i], fo.params(**BASE)) for i in range(2 * N)])
        _pass_in[(w, h)] = (np.ascontiguousarray(r[:N]), np.ascontiguousarray(r[N:]))
    key = (w, h, winsize, gaussian, kind)
    if key not in _pass_ref:
        r0, r1 = _pass_in[(w, h)]
        fl = _incoming(kind, N, w, h)
        p = fo.params(**dict(BASE, winsize=winsize, gaussian=gaussian))
        ref = np.stack([np.stack(fo.one_pass(r0[i], r1[i], fl[i, 0], fl[i, 1], p)) for i in range(N)]).astype(np.float32)
        assert np.isfinite(ref).all(), "the oracle's pass is not finite: %r" % (key,)
        _pass_ref[key] = (fl, ref)
    return _pass_in[(w, h)] + _pass_ref[key]


PASS_CASES = [(ws, tile, run, lds, w, h) for ws, tile, run, lds, fields in fs.FB_PASS_CASES for w, h in fields]


@pytest.mark.parametrize("kind", ["zero", "leaving"])
@pytest.mark.parametrize("gaussian", [0, 1])
@pytest.mark.parametrize("winsize,tile,run,lds,w,h", PASS_CASES,
                         ids=["win%d_%s_%dx%d" % (c[0], "own" if c[1] == (0, 0) else "%dx%d" % c[1], c[4], c[5]) for c in PASS_CASES])
def test_one_pass_at_the_limits_of_the_window(winsize, tile, run, lds, w, h, gaussian, kind):
    """83 x 67: several ragged tiles; 20 x 16: the windows of 59 to 63 are wider than the field, every tap clamps.  Incoming
    flow of zero and of +-40 px (S65's rule for positions that leave the frame, on each side)."""
    from video_analytics_amd import _ffi
    assert fs.pass_tile(winsize, *tile) == run + (lds,) and lds <= fs.MAX_LDS
    r0, r1, fl, ref = _pass_reference(w, h, winsize, gaussian, kind)
    if kind == "leaving":
        assert fs.leaves_on_all_sides(fl)
    p = _ffi.default_farneback_params(**dict(BASE, winsize=winsize, gaussian=gaussian, levels=1, **_tiles("pass", tile)))
    assert _ffi.lib().va_farneback_workspace_bytes(w, h, 1, 2, ctypes.byref(p)) > 0, _ffi.lib().va_last_error()
    d0, d1, din = (torch.from_numpy(a).cuda() for a in (r0, r1, fl))
    out = torch.full(tuple(fl.shape), float("nan"), dtype=torch.float32, device="cuda")
    _ffi.check(_ffi.lib().va_farneback_pass(_ffi.ctx(0), _ffi.ptr(d0), _ffi.ptr(d1), _ffi.ptr(din), _ffi.ptr(out), N, w, h,
                                            ctypes.byref(p), _ffi.stream_ptr(out.device)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, ref), "%d values differ, max abs diff %g" % (int((got != ref).sum()), np.nanmax(np.abs(got - ref)))
    for d, a in ((d0, r0), (d1, r1), (din, fl)):
        assert torch.equal(d.cpu(), torch.from_numpy(a))  # inputs untouched


# ------------------------------------------------------------------------------------------------ b. polynomial expansion

_poly_ref = {}


def _poly_reference(w, h, poly_n, poly_sigma):
    key = (w, h, poly_n, poly_sigma)
    if key not in _poly_ref:
        f = _texture(N, w, h, 100 * w + h)
        p = fo.params(**dict(BASE, poly_n=poly_n, poly_sigma=poly_sigma))
        ref = np.stack([fo.polyexp(f[i], p) for i in range(N)])
        assert np.isfinite(ref).all(), "the oracle's expansion is not finite: %r" % (key,)
        _poly_ref[key] = (f, ref)
    return _poly_ref[key]


@pytest.mark.parametrize("poly_n,poly_sigma,tile,lds,wh", fs.FB_POLY_CASES,
                         ids=["n%d_sigma%g_%s_%dx%d" % (c[0], c[1], "own" if c[2] == (0, 0) else "%dx%d" % c[2], c[4][0], c[4][1])
                              for c in fs.FB_POLY_CASES])
def test_polyexp_at_its_limits(poly_n, poly_sigma, tile, lds, wh):
    """poly_sigma 0.6 (the outer taps underflow towards 0) and 3.0 (nearly flat over the window); tiles of 128 x 64, the
    first to need more than 64 KB of LDS in this kernel; a tile of 256 x 8, wider than the field; tiles of 1 x 1"""
    from video_analytics_amd import _ffi
    w, h = wh
    t = fs.poly_tile(poly_n, *tile)
    assert t is not None and t[2] == lds <= fs.MAX_LDS and (lds > 64 * 1024) == (tile == (128, 64))
    f, ref = _poly_reference(w, h, poly_n, poly_sigma)
    p = _ffi.default_farneback_params(**dict(BASE, poly_n=poly_n, poly_sigma=poly_sigma, levels=1, **_tiles("poly", tile)))
    assert _ffi.lib().va_farneback_workspace_bytes(w, h, 1, 2, ctypes.byref(p)) > 0, _ffi.lib().va_last_error()
    d = torch.from_numpy(f).cuda()
    out = torch.full((N, 5, h, w), float("nan"), dtype=torch.float32, device="cuda")
    _ffi.check(_ffi.lib().va_farneback_polyexp(_ffi.ctx(0), _ffi.ptr(d), N, w, h, ctypes.byref(p), _ffi.ptr(out), _ffi.stream_ptr(d.device)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, ref), "%d values differ, max abs diff %g" % (int((got != ref).sum()), np.nanmax(np.abs(got - ref)))
    assert torch.equal(d.cpu(), torch.from_numpy(f))  # input untouched


# ------------------------------------------------------------------------------------------------ c. end to end

OWN_TILES = dict(poly_tile_w=23, poly_tile_h=11, pass_tile_w=24, pass_tile_h=8)  # (24 x 8 fits beside a window of 63: 134,160 B)

# (overrides of BASE, levels of the 83 x 67 pyramid, also under OWN_TILES)
FLOW_CASES = [
    (dict(iterations=1), 3, False), (dict(iterations=3), 3, True),     # the coarse flow is upsampled from planes (2, 3)
    (dict(pyr_scale=0.8, levels=5), 5, False), (dict(pyr_scale=0.65, levels=4), 4, False), (dict(pyr_scale=0.3), 2, False),
    (dict(levels=1), 1, False), (dict(levels=40), 3, False),           # clipped by S1's smallest level
    (dict(levels=40, pyr_scale=0.95), 16, False),                      # clipped by the sixteen levels the library holds
    (dict(winsize=63, gaussian=0), 3, True), (dict(winsize=63, gaussian=1), 3, True),  # wider than the coarse levels
    (dict(winsize=3), 3, False), (dict(poly_n=7, poly_sigma=1.5), 3, False),
]
FLOW_PARAMS = [pytest.param(over, levels, tiles, id=",".join("%s=%g" % kv for kv in over.items()) + ("-own_tiles" if tiles else ""))
               for over, levels, both in FLOW_CASES for tiles in ((dict(), OWN_TILES) if both else (dict(),))]

_flow_ref = {}


def _frames(n_seq=2, n_frames=3):
    from video_analytics_amd import synth
    _, gray, _ = synth.synth_clips(n_seq, seed=4, H=67, W=83, n_gray=n_frames)  # uint8: rows of 83 in a pitch of 84
    return gray


def _flow_reference(key, frames, kw):
    """the oracle's flow: computed once per case, shared by the tile shapes, asserted finite"""
    if key not in _flow_ref:
        ref = fo.farneback_flow(frames.numpy(), fo.params(**kw))
        assert np.isfinite(ref).all(), "the oracle's flow is not finite: %r" % (kw,)
        _flow_ref[key] = ref
    return _flow_ref[key]


def _check_flow(frames, ref, kw, tiles):
    from video_analytics_amd import flow as vflow
    d = frames.cuda()
    keep = d.clone()
    out = torch.full(tuple(ref.shape), float("nan"), dtype=torch.float32, device="cuda")
    assert vflow.farneback_flow(d, out=out, **kw, **tiles) is out
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, ref), "%r %r: %d values differ, max abs diff %g" % (kw, tiles, int((got != ref).sum()), np.nanmax(np.abs(got - ref)))
    assert torch.equal(d, keep)  # input untouched


@pytest.mark.parametrize("over,levels,tiles", FLOW_PARAMS)
def test_farneback_flow_one_parameter_at_a_time(over, levels, tiles):
    """[2,3,67,83] uint8, four pairs"""
    from video_analytics_amd import _ffi, flow as vflow
    from oracle import tvl1_oracle
    kw = dict(BASE, **over)
    sizes = vflow.pyramid_sizes(83, 67, _ffi.default_farneback_params(**kw))
    assert len(sizes) == levels and sizes == tvl1_oracle.pyramid_sizes(83, 67, kw["levels"], kw["pyr_scale"])
    if kw["winsize"] == 63:
        assert min(sizes[-1]) < 63 and fs.pass_tile(63) == (16, 16, 146640) and fs.pass_tile(63, 24, 8) == (24, 8, 134160)
    frames = _frames()
    _check_flow(frames, _flow_reference(tuple(sorted(over.items())), frames, kw), kw, tiles)


@pytest.mark.parametrize("n_seq,n_frames", [(3, 2), (2, 4)])
def test_farneback_flow_maps_pairs_to_frames(n_seq, n_frames):
    """frame(n) = n + n / (fps - 1) with one pair per sequence (every pair skips a frame) and with three (4 frames: pairs
    0, 1, 2 read frames 0 ... 3, pairs 3, 4, 5 frames 4 ... 7); iterations 3 as well, since the mapping and the odd
    iteration count meet in the same launch"""
    frames = _frames(n_seq, n_frames)
    assert frames.shape == (n_seq, n_frames, 67, 83)
    for over in (dict(), dict(iterations=3)):
        kw = dict(BASE, **over)
        ref = _flow_reference((n_seq, n_frames) + tuple(over.items()), frames, kw)
        assert ref.shape[0] == n_seq * (n_frames - 1)
        _check_flow(frames, ref, kw, dict())


@pytest.mark.parametrize("name", fs.CONTENTS)
def test_farneback_flow_on_content_the_clips_do_not_produce(name):
    """three pairs of 83 x 67 each: identical constant frames (the oracle's flow is exactly 0), saturated checkerboards
    moved by one pixel, and magnified textures whose flow leaves the frame on all four sides"""
    frames = torch.from_numpy(fs.content_pairs(name, 67, 83))
    ref = _flow_reference(name, frames, BASE)
    if name == "constant":
        assert np.all(ref == 0.0)
    if name == "leaving":
        assert fs.leaves_on_all_sides(ref)
    _check_flow(frames, ref, BASE, dict())
