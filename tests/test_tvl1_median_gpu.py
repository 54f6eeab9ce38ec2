"""The median option of TV-L1 on the GPU: ``flow.median_filter`` against a numpy filter, ``tvl1_flow`` with
the option bit-equal to the flows of the median oracle (tests/golden/tvl1_median.npz) under every iteration plan, the
option off bit-equal to ``va_tvl1_flow``, and the option reaching the pipeline's entry points through ``tvl1_params``."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tvl1_median_oracle as mo

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHORT = dict(epsilon=0.0, iters=30, warps=3)
# iteration plans the result must not depend on: register tiles of either size class, the row pipeline on every level in
# its four-wave, one-wave and two-wave forms, the shallowest and a deeper block
PLANS = [dict(), dict(tile_mask=0xFF), dict(tile_mask=1 << 8), dict(tile_mask=1 << 8, stream_waves=1),
         dict(tile_mask=1 << 8, stream_waves=2), dict(block_iters=1), dict(block_iters=6)]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(os.path.join(GOLD, "tvl1_median.npz")))
    g["gray"] = np.load(os.path.join(GOLD, "tvl1_64x48.npz"))["gray"]
    return g


# ---------------------------------------------------------------- the filter alone

def _fields(w, h, n=3):
    rs = np.random.RandomState(1000 * w + h)
    rnd = (rs.standard_normal((n, 2, h, w)) * 7.0).astype(np.float32)
    ties = rs.randint(-2, 3, size=(n, 2, h, w)).astype(np.float32) * np.float32(0.25)
    zeros = np.where(rs.rand(n, 2, h, w) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    zeros = np.where(rs.rand(n, 2, h, w) < 0.3, rnd, zeros).astype(np.float32)
    return {"random": rnd, "ties": ties, "zeros": zeros}


@pytest.mark.parametrize("ksize", [3, 5])
@pytest.mark.parametrize("w,h", [(1, 1), (2, 3), (4, 4), (5, 7), (37, 19), (130, 3), (257, 9), (67, 33)])
def test_median_filter_is_the_numpy_filter(w, h, ksize):
    from video_analytics_amd import flow as vflow
    for name, f in _fields(w, h).items():
        got = vflow.median_filter(torch.from_numpy(f).cuda(), ksize)
        assert same_bits(got.cpu().numpy(), mo.flow_median_np(f, ksize)), name


def test_median_filter_refuses_overlap_and_other_sizes():
    from video_analytics_amd import flow as vflow
    buf = torch.zeros((3, 2, 8, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        vflow.median_filter(buf[:2], 5, out=buf[1:])
    with pytest.raises(ValueError, match="overlap"):
        vflow.median_filter(buf, 3, out=buf)
    with pytest.raises(ValueError, match="ksize"):
        vflow.median_filter(buf, 4)
    out = torch.empty_like(buf)
    assert vflow.median_filter(buf, 5, out=out) is out


# ---------------------------------------------------------------- tvl1_flow with the option

@pytest.mark.parametrize("plan", PLANS, ids=lambda p: ",".join("%s=%s" % kv for kv in p.items()) or "default")
@pytest.mark.parametrize("median,every,key", [(5, 10, "flow_m5_e10"), (3, 7, "flow_m3_e7"), (5, 0, "flow_m5_e0")])
def test_fixed_mode_equals_the_golden_under_every_plan(golden, median, every, key, plan):
    from video_analytics_amd import flow as vflow
    ref = golden[key]
    gray = torch.from_numpy(golden["gray"][:ref.shape[0] // 2]).cuda()
    out = vflow.tvl1_flow(gray, median=median, median_every=every, **SHORT, **plan).cpu().numpy()
    assert same_bits(out, ref), "max abs diff %g" % np.abs(out - ref).max()


def test_epsilon_mode_equals_the_golden(golden):
    from video_analytics_amd import flow as vflow
    gray = torch.from_numpy(golden["gray"][:1]).cuda()
    out = vflow.tvl1_flow(gray, epsilon=0.01, iters=300, median=5, median_every=30).cpu().numpy()
    assert same_bits(out, golden["flow_eps_m5_e30"]), "max abs diff %g" % np.abs(out - golden["flow_eps_m5_e30"]).max()
    plain = vflow.tvl1_flow(gray, epsilon=0.01, iters=300).cpu().numpy()
    assert np.abs(out - plain).max() > 1.0


@pytest.fixture(scope="module")
def wide(golden, oracle_tvl1):
    """Three sequences 200 wide x 40 high from the golden pair (A, B): (A, B), (B, A) and both frames upside down; the
    median oracle's flow of each, the first being the golden's."""
    A, B = golden["wide_gray"][0]
    gray = np.ascontiguousarray(np.stack([np.stack([A, B]), np.stack([B, A]), np.stack([A[::-1], B[::-1]])]))
    ref = mo.tvl1_flow(gray, oracle_tvl1.default_params(**SHORT), 5, 10)
    assert same_bits(ref[:1], golden["wide_flow_m5_e10"])
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[0], ref[2])
    return gray, ref


@pytest.mark.parametrize("plan", [dict(), dict(tile_mask=0xFF), dict(tile_mask=1 << 8), dict(tile_mask=1 << 8, stream_waves=1),
                                  dict(tile_mask=1 << 8, stream_chunks=1), dict(block_iters=4)],
                         ids=lambda p: ",".join("%s=%s" % kv for kv in p.items()) or "default")
def test_wide_pairs_equal_the_oracle(wide, plan):
    """Level 0 is two strips of the row pipeline, the two coarsest levels (102 and 82 wide) have a row pitch that differs
    from their width, and the coarsest, 82 x 17, is barely taller than the window."""
    from video_analytics_amd import flow as vflow
    gray, ref = wide
    assert vflow.pyramid_sizes(200, 40) == [(200, 40), (160, 32), (128, 26), (102, 21), (82, 17)]
    out = vflow.tvl1_flow(torch.from_numpy(gray).cuda(), median=5, median_every=10, **SHORT, **plan).cpu().numpy()
    assert same_bits(out, ref), "max abs diff %g" % np.abs(out - ref).max()


# ---------------------------------------------------------------- the option off

def test_option_off_is_va_tvl1_flow(golden):
    from video_analytics_amd import _ffi
    from video_analytics_amd import flow as vflow
    L, c = _ffi.lib(), _ffi.ctx(0)
    gray = torch.from_numpy(golden["gray"]).cuda()
    S, F, H, W = gray.shape
    size = ctypes.sizeof(_ffi.Tvl1Options)
    for kw in (SHORT, dict(epsilon=0.01, iters=300)):
        p = _ffi.default_tvl1_params(**kw)
        parent = vflow.tvl1_flow(gray, p)
        nbytes = L.va_tvl1_workspace_bytes(W, H, S, F, ctypes.byref(p))
        for opt in (None, _ffi.Tvl1Options(size, 0, 0), _ffi.Tvl1Options(size, 0, 7)):
            ref = ctypes.byref(opt) if opt is not None else None
            assert L.va_tvl1_workspace_bytes_opt(W, H, S, F, ctypes.byref(p), ref) == nbytes
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            out = torch.empty_like(parent)
            _ffi.check(L.va_tvl1_flow_opt(c, _ffi.ptr(gray), 1, S, F, W, H, ctypes.byref(p), ref, _ffi.ptr(out), _ffi.ptr(ws),
                                          ws.numel(), _ffi.stream_ptr(gray.device)))
            assert torch.equal(out, parent)
    with pytest.raises(ValueError, match="median"):
        vflow.tvl1_flow(gray, median=4)
    with pytest.raises(ValueError, match="median_every"):
        vflow.tvl1_flow(gray, median=5, median_every=-1)


# ---------------------------------------------------------------- the pipeline carries the option in tvl1_params

SCHEDULE = dict(epsilon=0.0, iters=30, warps=2)


@pytest.fixture(scope="module")
def clips():
    from video_analytics_amd import synth
    return synth.synth_clips(2, seed=131)[1].cuda()  # gray u8 [2, 11, 224, 224]


def test_pipeline_flow_volume_and_extract_flow_are_filtered(clips):
    from video_analytics_amd import _ffi, pipeline
    from video_analytics_amd import flow as vflow
    params = _ffi.default_tvl1_params(median=5, median_every=10, **SCHEDULE)
    B, F, H, W = clips.shape
    want = vflow.tvl1_flow(clips, params).clone()
    plain = vflow.tvl1_flow(clips, _ffi.default_tvl1_params(**SCHEDULE)).clone()
    assert not torch.equal(want, plain)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    other = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(**SCHEDULE))
    try:
        vol = pipe.flow_volume(clips)
        assert torch.equal(vol, vflow.flow_to_stack(want).view(B, 2 * (F - 1), H, W))
        assert not torch.equal(vol, other.flow_volume(clips))
        store = pipe.extract_flow(clips[0], dtype=torch.float32)
        assert torch.equal(store, want[:F - 1])
        assert not torch.equal(store, other.extract_flow(clips[0], dtype=torch.float32))
    finally:
        pipe.close()
        other.close()


def test_pipeline_rerun_form_filters_the_second_pass(clips):
    from video_analytics_amd import _ffi, pipeline
    from video_analytics_amd import flow as vflow
    params = _ffi.default_tvl1_params(median=5, median_every=10, **SCHEDULE)
    B, F, H, W = clips.shape
    first = vflow.tvl1_flow(clips, params).clone()
    field = vflow.rerun_camera(clips, first, params)[0].clone()
    assert not torch.equal(field, first)
    unfiltered = vflow.rerun_camera(clips, first, _ffi.default_tvl1_params(**SCHEDULE))[0].clone()
    assert not torch.equal(field, unfiltered)  # the second pass is filtered too
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params, camera="homography", camera_form="rerun")
    try:
        assert torch.equal(pipe.flow_volume(clips), vflow.flow_to_stack(field).view(B, 2 * (F - 1), H, W))
        one = vflow.tvl1_flow(clips[:1], params).clone()
        assert torch.equal(pipe.extract_flow(clips[0], dtype=torch.float32), vflow.rerun_camera(clips[:1], one, params)[0])
    finally:
        pipe.close()
