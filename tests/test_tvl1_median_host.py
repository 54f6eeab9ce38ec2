"""The median option of TV-L1 on the CPU: the C filter of tests/tvl1_median_oracle.c against a numpy
filter, the median oracle with the option off against the stock oracle, the median oracle against the float64 witness with
the filter (the bounds tests/test_oracle_tvl1.py states for the stock oracle), the committed golden, and the argument
checks of the ``_opt`` entry points that need no device."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import tvl1_median_oracle as mo

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
SIZES = [(1, 1), (2, 3), (4, 4), (5, 7), (37, 19)]  # (w, h)


@pytest.fixture(scope="module")
def gray():
    return np.load(os.path.join(GOLD, "tvl1_64x48.npz"))["gray"]


def fields(w, h, n=3):
    """{name: float32 [n,2,h,w]}: random values, values quantised to five levels (ties), and signed zeros among others."""
    rs = np.random.RandomState(1000 * w + h)
    rnd = (rs.standard_normal((n, 2, h, w)) * 7.0).astype(np.float32)
    ties = rs.randint(-2, 3, size=(n, 2, h, w)).astype(np.float32) * np.float32(0.25)
    zeros = np.where(rs.rand(n, 2, h, w) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    zeros = np.where(rs.rand(n, 2, h, w) < 0.3, rnd, zeros).astype(np.float32)
    return {"random": rnd, "ties": ties, "zeros": zeros}


@pytest.mark.parametrize("ksize", [3, 5])
@pytest.mark.parametrize("w,h", SIZES)
def test_c_filter_is_the_numpy_filter(w, h, ksize):
    for name, f in fields(w, h).items():
        assert np.array_equal(mo.flow_median(f, ksize), mo.flow_median_np(f, ksize)), name


def test_c_filter_refuses_bad_arguments():
    f = np.zeros((1, 2, 4, 4), np.float32)
    with pytest.raises(ValueError):
        mo.flow_median(f, 4)


def test_median_off_is_the_stock_oracle(oracle_tvl1, gray):
    short = oracle_tvl1.default_params(epsilon=0.0, iters=30, warps=3)
    assert np.array_equal(mo.tvl1_flow(gray, short, 0, 0), oracle_tvl1.tvl1_flow(gray, short))
    assert np.array_equal(mo.tvl1_flow(gray, short, 0, 7), oracle_tvl1.tvl1_flow(gray, short))
    eps = oracle_tvl1.default_params(epsilon=0.01, iters=300)
    a, ia = mo.tvl1_flow(gray, eps, 0, 0, return_iters=True)
    b, ib = oracle_tvl1.tvl1_flow(gray, eps, return_iters=True)
    assert np.array_equal(a, b) and np.array_equal(ia, ib)


def _witness_errors(oracle_tvl1, gray, median, every, **kw):
    """Per-pixel |median C oracle - float64 witness with the filter| (max over the two components) of every golden pair,
    and the oracle's flow."""
    ref = mo.tvl1_flow(gray, oracle_tvl1.default_params(epsilon=0.0, **kw), median, every)
    errs, k = [], 0
    for s in range(gray.shape[0]):
        for j in range(gray.shape[1] - 1):
            u1, u2 = mo.tvl1_flow_pair_f64(gray[s, j], gray[s, j + 1], median, every, **kw)
            errs.append(np.maximum(np.abs(u1 - ref[k, 0]), np.abs(u2 - ref[k, 1])))
            k += 1
    return np.stack(errs), ref


@pytest.mark.parametrize("median,every", [(5, 10), (3, 7), (5, 0)])
def test_median_oracle_against_float64_witness_short_schedule(oracle_tvl1, gray, median, every):
    """5 levels x 3 warps x 30 iterations, the bounds of test_independent_float64_ipol_witness_short_schedules: max 5e-3 px,
    median 1e-5 px.  Measured: (5,10) max 5.3e-4, median 5.9e-7; (3,7) 1.5e-3, 6.2e-7; (5,0) 1.8e-3, 5.6e-7.  The filter
    acts: the flow differs from the unfiltered one by more than 1 px."""
    e, ref = _witness_errors(oracle_tvl1, gray, median, every, iters=30, warps=3)
    print("median %d every %d: max %.3g median %.3g" % (median, every, e.max(), np.median(e)))
    assert e.max() < 5e-3 and np.median(e) < 1e-5, (e.max(), np.median(e))
    plain = oracle_tvl1.tvl1_flow(gray, oracle_tvl1.default_params(epsilon=0.0, iters=30, warps=3))
    assert np.abs(ref - plain).max() > 1.0


def test_median_oracle_against_float64_witness_full_schedule(oracle_tvl1, gray):
    """5 x 5 x 300 with OpenCV's CPU defaults (median 5 every 30), the bounds of
    test_independent_float64_ipol_witness_full_schedule: median 1e-4 px, at least 96 % of the pixels within 1e-3 px, every
    pixel further than 8 px from the border within 1e-2 px.  Measured: median 9.9e-7, 97.2 %, interior max 3.5e-3."""
    e, ref = _witness_errors(oracle_tvl1, gray, 5, 30, iters=300, warps=5)
    print("full schedule: median %.3g share %.4f interior max %.3g" % (np.median(e), (e < 1e-3).mean(), e[:, 8:-8, 8:-8].max()))
    assert np.median(e) < 1e-4, np.median(e)
    assert (e < 1e-3).mean() > 0.96, (e < 1e-3).mean()
    assert e[:, 8:-8, 8:-8].max() < 1e-2, e[:, 8:-8, 8:-8].max()
    plain = oracle_tvl1.tvl1_flow(gray, oracle_tvl1.default_params(epsilon=0.0, iters=300, warps=5))
    assert np.abs(ref - plain).max() > 1.0


def test_golden_regenerates(oracle_tvl1):
    spec = importlib.util.spec_from_file_location("make_tvl1_median_golden", os.path.join(GOLD, "make_tvl1_median_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert os.path.getsize(gen.OUT) < 300 * 1024
    stored = np.load(gen.OUT)
    fresh = gen.arrays()
    assert sorted(stored.files) == sorted(fresh)
    for k, v in fresh.items():
        assert stored[k].dtype == v.dtype and np.array_equal(stored[k], v), k
    assert stored["iters_eps_m5_e30"].max() < 5 * 5 * 300  # the stopping rule fires with the filter in the loop


# ---------------------------------------------------------------- argument checks (no device)

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    from video_analytics_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        __graft_entry__.build()
    return _ffi.lib()


def _bytes(lib, p, opt):
    return lib.va_tvl1_workspace_bytes_opt(64, 48, 2, 3, ctypes.byref(p), ctypes.byref(opt) if opt is not None else None)


def test_options_leave_the_workspace_size_alone(lib):
    from video_analytics_amd import _ffi
    for kw in (dict(), dict(epsilon=0.0, iters=30, warps=3), dict(epsilon=0.0, tile_mask=1 << 8)):
        p = _ffi.default_tvl1_params(**kw)
        parent = lib.va_tvl1_workspace_bytes(64, 48, 2, 3, ctypes.byref(p))
        assert parent > 0
        assert _bytes(lib, p, None) == parent
        size = ctypes.sizeof(_ffi.Tvl1Options)
        assert _bytes(lib, p, _ffi.Tvl1Options(size, 0, 0)) == parent
        assert _bytes(lib, p, _ffi.Tvl1Options(size, 0, 30)) == parent
        assert _bytes(lib, p, _ffi.Tvl1Options(size, 5, 30)) == parent  # the filter goes through the pyramid's scratch
        assert _bytes(lib, p, _ffi.Tvl1Options(size + 8, 3, 0)) == parent  # a longer structure of a later version


@pytest.mark.parametrize("fields,word", [((12, 4, 0), b"median"), ((12, 7, 0), b"median"), ((12, -3, 0), b"median"),
                                         ((12, 5, -1), b"median_every"), ((8, 5, 30), b"struct_bytes"),
                                         ((0, 0, 0), b"struct_bytes")])
def test_bad_options_give_zero_bytes_and_a_message(lib, fields, word):
    from video_analytics_amd import _ffi
    p = _ffi.default_tvl1_params()
    assert _bytes(lib, p, _ffi.Tvl1Options(*fields)) == 0
    assert word in lib.va_last_error(), lib.va_last_error()


def test_python_attributes_travel_beside_the_structure():
    from video_analytics_amd import _ffi
    p = _ffi.default_tvl1_params(median=5, median_every=30)
    assert (p.median, p.median_every) == (5, 30)
    assert ctypes.sizeof(p) == 76  # va_tvl1_params does not grow (tests/reference_binding_stub.py mirrors it)
    o = _ffi.tvl1_options(p)
    assert (o.struct_bytes, o.median, o.median_every) == (12, 5, 30)
    q = _ffi.default_tvl1_params()
    assert (q.median, q.median_every) == (0, 0) and _ffi.tvl1_options(q) is None
    with pytest.raises(ValueError):
        _ffi.default_tvl1_params(medain=5)
