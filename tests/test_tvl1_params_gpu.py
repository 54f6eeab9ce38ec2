"""GPU parity of the TV-L1 HIP path against the C oracle AWAY from va_tvl1_default_params: scale steps 0.1 ... 0.95 (zoom-out
radii 1 ... 7 and the clamp to 8), pyramids of 12 and 16 levels, tau / lambda / theta sets, and frame content the synthetic
clips never produce (fractional floats, constants, saturated patterns, edges, flow that leaves the frame, displacement
fields that defeat the warp's lane shuffle).

Same bar as tests/test_tvl1_gpu.py: BIT-EXACT flow under every kernel choice.  The oracle itself is pinned to its float64
witness at these parameters in tests/test_oracle_tvl1.py.  Every test first asserts that the oracle's flow is finite, so
that no NaN can sit on both sides of a comparison.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# tuning fields of va_tvl1_params the oracle has no counterpart for (results must not depend on them)
PRODUCT_ONLY = ("block_iters", "tile_mask", "stream_levels", "stream_waves", "stream_chunks", "stream_slots", "stream_ppl", "stream_queue",
                "rows_levels", "rows_cfg", "fast_math")

STREAM = 1 << 8  # tile_mask bit: the row pipeline k_iter_stream on every level
# "kernel choices": the library's own pick per level, the register tiles, the row pipeline in its default (four-wave), two-wave
# and 4 x 5 forms
KERNELS = [dict(), dict(tile_mask=0xFF), dict(tile_mask=STREAM), dict(tile_mask=STREAM, stream_waves=2), dict(tile_mask=STREAM, stream_waves=8)]
# with the stopping rule every level runs on the register tiles (one iteration per launch): the library's pick and two fixed
# candidates (128 x 64 with eight waves, 84 x 48 with four)
EPS_KERNELS = [dict(), dict(tile_mask=1 << 1), dict(tile_mask=1 << 6)]
# switches of retired kernel families (the persistent row pipeline, the 3 x 5, 3 x 6 and 4 x 6 row pipelines): refused
RETIRED_KERNELS = [dict(tile_mask=1 << 9)] + [dict(tile_mask=STREAM, stream_waves=w) for w in (10, 11, 12)]


def _frames(n_seq, n_frames, H, W, seed):
    from video_analytics_amd import synth
    _, gray, _ = synth.synth_clips(n_seq, seed=seed, H=H, W=W, n_gray=n_frames)
    return gray


def _oracle(oracle_tvl1, gray, return_iters=False, **kw):
    okw = {("lambda_" if k == "lambda" else k): v for k, v in kw.items() if k not in PRODUCT_ONLY}
    out = oracle_tvl1.tvl1_flow(gray.numpy(), oracle_tvl1.default_params(**okw), nthreads=8, return_iters=return_iters)
    ref = out[0] if return_iters else out
    assert np.isfinite(ref).all(), "the oracle's flow is not finite: %r" % (kw,)
    return out


def _gpu(gray, **kw):
    from video_analytics_amd import flow as vflow
    out = vflow.tvl1_flow(gray.cuda(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_kernels(ref, gray, kernels, **kw):
    """The GPU flow under every kernel choice equals ``ref`` bit for bit."""
    for kern in kernels:
        out = _gpu(gray, **kw, **kern)
        assert np.array_equal(out, ref), "%r %r: %d values differ, max abs diff %g" % (kw, kern, int((out != ref).sum()), np.nanmax(np.abs(out - ref)))


# ------------------------------------------------------------------------------------------------ a. scale_step

# step -> zoom-out radius (int)(3 sigma) + 1 before the clamp to 8, levels of the 333 x 170 pyramid with nscales = 5
STEPS = [(0.95, 1, 5), (0.9, 1, 5), (0.65, 3, 5), (0.5, 4, 4), (0.4, 5, 3), (0.3, 6, 2), (0.25, 7, 2), (0.2, 9, 2), (0.1, 18, 2)]


@pytest.mark.parametrize("step,radius,levels", STEPS)
def test_scale_step_bit_exact(oracle_tvl1, step, radius, levels):
    # 333 x 170: at step 0.1 the second level is 33 x 17, so every step has at least two levels and runs k_gauss (radius 1 ... 7,
    # then 8 for the steps whose radius is clamped), k_resample and k_upsample (1 / step from 1.05 to 10)
    from video_analytics_amd import _ffi
    from video_analytics_amd import flow as vflow
    sizes = vflow.pyramid_sizes(333, 170, _ffi.default_tvl1_params(scale_step=step))
    assert sizes == oracle_tvl1.pyramid_sizes(333, 170, 5, step) and len(sizes) == levels
    assert oracle_tvl1.zoom_taps(step)[0] == min(radius, 8)
    gray = _frames(2, 2, 170, 333, seed=int(step * 100))
    kw = dict(epsilon=0.0, iters=17, warps=2, nscales=5, scale_step=step)
    _check_kernels(_oracle(oracle_tvl1, gray, **kw), gray, KERNELS, **kw)
    kw = dict(epsilon=0.02, iters=40, warps=1, nscales=5, scale_step=step)
    _check_kernels(_oracle(oracle_tvl1, gray, **kw), gray, EPS_KERNELS[:2], **kw)


# ------------------------------------------------------------------------------------------------ b. deep pyramids

@pytest.mark.parametrize("nscales", [16, 40])
def test_sixteen_level_pyramid_bit_exact(oracle_tvl1, nscales):
    # 56 x 40 at step 0.95: 16 levels down to 28 x 20, asked for as 16 and as 40 (clamped to kMaxScales); the level bit sets carry
    # bit 15; 0xAAAA / 0x5555 alternate the two state layouts, a conversion at every one of the 15 transitions
    from video_analytics_amd import _ffi
    from video_analytics_amd import flow as vflow
    sizes = vflow.pyramid_sizes(56, 40, _ffi.default_tvl1_params(scale_step=0.95, nscales=nscales))
    assert len(sizes) == 16 and sizes == oracle_tvl1.pyramid_sizes(56, 40, nscales, 0.95)
    gray = _frames(3, 2, 40, 56, seed=40 + nscales)
    kw = dict(epsilon=0.0, iters=11, warps=1, nscales=nscales, scale_step=0.95)
    ref = _oracle(oracle_tvl1, gray, **kw)
    _check_kernels(ref, gray, KERNELS[:3] + [dict(stream_levels=b) for b in (0x8000, 0xAAAA, 0x5555, 0xFFFF)], **kw)


@pytest.mark.parametrize("nch", [0, 2])
def test_twelve_level_pyramid_bit_exact(oracle_tvl1, nch):
    from video_analytics_amd import _ffi
    from video_analytics_amd import flow as vflow
    assert len(vflow.pyramid_sizes(131, 57, _ffi.default_tvl1_params(scale_step=0.9, nscales=12))) == 12
    gray = _frames(3, 2, 57, 131, seed=12 + nch)
    kw = dict(epsilon=0.0, iters=11, warps=1, nscales=12, scale_step=0.9)
    ref = _oracle(oracle_tvl1, gray, **kw)
    _check_kernels(ref, gray, [dict(k, stream_chunks=nch) for k in KERNELS] + [dict(stream_levels=0xAAA, stream_chunks=nch)], **kw)


# ------------------------------------------------------------------------------------------------ c. tau, lambda, theta

# (tau, lambda, theta, scale_step or None: the shape's).  The third and fourth have a large lambda * theta against theta:
# ill-conditioned at the frame border (tests/test_oracle_tvl1.py), where one differing bit grows to pixels within a few
# warps -- the sets on which a bit comparison is most sensitive.
PARAM_SETS = [(0.125, 0.05, 0.5, None), (0.25, 0.02, 1.0, None), (0.25, 0.6, 0.3, None), (0.1, 0.3, 0.15, None), (0.25, 1.0, 0.3, 0.9),
              (0.05, 0.15, 0.3, None)]
# 131 x 57: one strip, shared last strips; 225 x 129: two strips; 300 x 150: three strips, register tiles with x and y halos
PARAM_SHAPES = [(57, 131, 0.5), (129, 225, 0.8), (150, 300, 0.5)]
_set_id = lambda s: "tau%g-lam%g-th%g" % s[:3]


def _set_kw(pset, shape_step):
    tau, lam, theta, step = pset
    return {"tau": tau, "lambda": lam, "theta": theta, "scale_step": step if step is not None else shape_step}


@pytest.mark.parametrize("H,W,step", PARAM_SHAPES)
@pytest.mark.parametrize("pset", PARAM_SETS, ids=_set_id)
def test_tau_lambda_theta_bit_exact(oracle_tvl1, pset, H, W, step):
    gray = _frames(3, 2, H, W, seed=H + W)
    for iters, warps, nscales in ((23, 2, 3), (44, 1, 2)):
        kw = dict(epsilon=0.0, iters=iters, warps=warps, nscales=nscales, **_set_kw(pset, step))
        _check_kernels(_oracle(oracle_tvl1, gray, **kw), gray, KERNELS, **kw)


@pytest.mark.parametrize("pset", PARAM_SETS, ids=_set_id)
def test_tau_lambda_theta_experiment_kernels_bit_exact(oracle_tvl1, pset):
    # the kernel families these cases drove were removed: with every parameter set their switches
    # are refused loudly instead of running another kernel
    from video_analytics_amd import flow as vflow
    for H, W, step in PARAM_SHAPES:
        gray = _frames(3, 2, H, W, seed=H + W)
        for k in RETIRED_KERNELS:
            with pytest.raises(ValueError, match="retired"):
                vflow.tvl1_flow(gray.cuda(), epsilon=0.0, iters=23, warps=2, nscales=3, **_set_kw(pset, step), **k)


EPS_SEED = 2


def _eps_frames(H, W):
    """Five pairs that stop at different times: frame 1 = frame 0 + a (next synthetic frame - frame 0) with a = 0 (stops after
    one iteration per warp), 0.002, 0.004, 0.02 and 1 (the full 2 ... 4 px motion, which 60 iterations never settle to 1e-3 px
    per iteration).  float32 frames off the integers.  Iteration totals of the oracle at epsilon = 0.001 for this seed:
    6 / 150 ... 270 / 340 ... 360 / 360 / 360 of 360, depending on the parameter set."""
    g = _frames(5, 2, H, W, seed=EPS_SEED).float()
    a = torch.tensor([0.0, 0.002, 0.004, 0.02, 1.0]).view(5, 1, 1)
    g[:, 1] = g[:, 0] + a * (g[:, 1] - g[:, 0])
    return g


@pytest.mark.parametrize("pset", PARAM_SETS, ids=_set_id)
def test_tau_lambda_theta_stopping_rule_bit_exact(oracle_tvl1, pset):
    # the stopping rule compares the mean squared update of a pair with epsilon^2: at 0.001 the pairs stop one by one or not at
    # all, 0.05 stops early, 0.5 within the first iterations of every warp
    gray = _eps_frames(129, 225)
    for epsilon in (0.001, 0.05, 0.5):
        kw = dict(epsilon=epsilon, iters=60, warps=2, nscales=3, **_set_kw(pset, 0.8))
        ref, n_it = _oracle(oracle_tvl1, gray, return_iters=True, **kw)
        if epsilon == 0.001:  # otherwise the case degenerates to "all pairs stop together"
            assert len(set(n_it.tolist())) >= 3, n_it
        if epsilon == 0.5:
            assert n_it.min() == 3 * 2 and n_it.max() <= 3 * 2 * 3, n_it  # 3 levels x 2 warps x the first one to three iterations
        _check_kernels(ref, gray, EPS_KERNELS, **kw)


@pytest.mark.parametrize("pset,step", [((0.125, 0.05, 0.5, None), 0.5), ((0.25, 0.02, 1.0, None), 0.8)], ids=["tau0.125-lam0.05-th0.5", "tau0.25-lam0.02-th1"])
def test_fast_math_at_non_default_parameters(pset, step):
    """fast_math = 1 has no oracle.  As test_streaming_kernel_fast_math_and_mixed_levels at the defaults: the row pipeline and
    the register tiles give the same bits (the same 1-ulp operations in both), and the result differs from the exact mode by
    more than 0 and by less than 1e-3 px over this short schedule (the two well-conditioned sets: the iteration is
    non-expansive there, rounding-level perturbations stay rounding-level)."""
    from video_analytics_amd import flow as vflow
    gray = _frames(2, 2, 224, 224, seed=77).cuda()
    kw = dict(epsilon=0.0, iters=25, warps=2, nscales=4, **_set_kw(pset, step))
    exact = vflow.tvl1_flow(gray, tile_mask=STREAM, **kw)
    fast = vflow.tvl1_flow(gray, tile_mask=STREAM, fast_math=1, **kw)
    tiles = vflow.tvl1_flow(gray, tile_mask=0xFF, fast_math=1, **kw)
    assert bool(torch.isfinite(exact).all()) and bool(torch.isfinite(fast).all())
    assert torch.equal(fast, tiles)
    d = (fast - exact).abs().max().item()
    assert 0.0 < d < 1e-3, d


# ------------------------------------------------------------------------------------------------ d. input content

def _texture(H, W, seed, margin):
    """A uint8 texture [H + 2 margin, W + 2 margin] (numpy)."""
    return _frames(1, 1, H + 2 * margin, W + 2 * margin, seed)[0, 0].numpy()


def _pair(f0, f1):
    return torch.from_numpy(np.ascontiguousarray(np.stack([f0, f1])[None]))


def _content(name, H, W):
    """[S,2,H,W] frames (uint8 or float32) of one content class."""
    rng = np.random.default_rng(H * 1000 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    if name == "fractional_f32":  # float frames with values off the integers
        g = _frames(2, 2, H, W, seed=H + W).numpy().astype(np.float32)
        return torch.from_numpy(g + rng.uniform(0.0, 1.0, g.shape).astype(np.float32))
    if name == "constant_0_255":  # no gradient anywhere: grad < 1e-10 on every pixel of every warp
        return _pair(np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8))
    if name == "constant_f32":
        return _pair(np.full((H, W), 100.25, np.float32), np.full((H, W), 100.75, np.float32))
    if name in ("checker_2", "checker_7"):  # saturated 0 / 255 cells of 1 x 1 / of 3 and 4 pixels, moved by one pixel
        n = int(name[-1])
        cell = lambda x, y: ((((x % n) * 2) // n + ((y % n) * 2) // n) % 2 * 255).astype(np.uint8)
        return _pair(cell(xx, yy), cell(xx + 1, yy))
    if name == "edge_vertical":
        return _pair(np.where(xx < W // 2, 20, 230).astype(np.uint8), np.where(xx < W // 2 + 2, 20, 230).astype(np.uint8))
    if name == "edge_horizontal":
        return _pair(np.where(yy < H // 3, 240, 10).astype(np.uint8), np.where(yy < H // 3 - 1, 240, 10).astype(np.uint8))
    m = 24
    big = _texture(H, W, seed=H + 3 * W, margin=m)
    f0 = big[m:m + H, m:m + W]
    if name == "translate_24_-19":  # I1(x, y) = I0(x - 24, y + 19): wide bands of warp targets clamp on every level
        return _pair(f0, big[m + 19:m + 19 + H, m - 24:m - 24 + W])
    if name == "translate_3_0":  # smooth flow: the neighbouring lane supplies the right taps nearly everywhere
        return _pair(f0, big[m:m + H, m - 3:m - 3 + W])
    if name == "random_displacement":  # every pixel displaced by its own (dx, dy) in -6 .. 6: it almost never does
        dx, dy = rng.integers(-6, 7, (H, W)), rng.integers(-6, 7, (H, W))
        return _pair(f0, big[yy + m + dy, xx + m + dx])
    raise KeyError(name)


CONTENTS = ["fractional_f32", "constant_0_255", "constant_f32", "checker_2", "checker_7", "edge_vertical", "edge_horizontal",
            "translate_24_-19", "translate_3_0", "random_displacement"]


@pytest.mark.parametrize("H,W", [(64, 96), (57, 131)])
@pytest.mark.parametrize("name", CONTENTS)
def test_input_content_bit_exact(oracle_tvl1, name, H, W):
    gray = _content(name, H, W)
    assert gray.shape[1:] == (2, H, W)
    for over in (dict(), {"tau": 0.25, "lambda": 0.3, "theta": 0.3, "scale_step": 0.65}):
        kw = dict(epsilon=0.0, iters=23, warps=3, nscales=4, **over)
        ref = _oracle(oracle_tvl1, gray, **kw)
        if name == "translate_24_-19":
            assert float(np.abs(ref).max()) > 8.0, float(np.abs(ref).max())
        if name.startswith("constant"):
            assert float(np.abs(ref).max()) == 0.0  # no gradient, no data step
        _check_kernels(ref, gray, KERNELS, **kw)


# ------------------------------------------------------------------------------------------------ e. workspace bounds

@pytest.mark.parametrize("H,W,kw", [
    (40, 56, dict(scale_step=0.95, nscales=16, iters=11, warps=1)),
    (40, 56, dict(scale_step=0.95, nscales=40, iters=11, warps=1, stream_levels=0x5555)),
    (40, 56, dict(scale_step=0.95, nscales=16, iters=11, warps=1, tile_mask=STREAM)),
    (57, 131, dict(scale_step=0.9, nscales=12, iters=11, warps=1)),
    (57, 131, dict(scale_step=0.9, nscales=12, iters=11, warps=1, tile_mask=STREAM, stream_chunks=2)),
    (170, 333, dict(scale_step=0.1, iters=17, warps=2)),
    (170, 333, dict(scale_step=0.95, iters=17, warps=2)),
    (170, 333, dict(scale_step=0.95, iters=17, warps=2, tile_mask=0xFF)),
], ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_declared_workspace_is_not_exceeded(oracle_tvl1, H, W, kw):
    """va_tvl1_flow through the ABI with a workspace of exactly va_tvl1_workspace_bytes, inside an allocation that is 4096
    bytes longer and filled with 0xA5: the tail keeps its pattern and the flow equals the oracle's (the sizing by the largest
    plane of the pyramid, with pitches and level counts the other tests do not produce)."""
    from video_analytics_amd import _ffi
    gray = _frames(2, 3, H, W, seed=H + W)
    kw = dict(epsilon=0.0, **kw)
    ref = _oracle(oracle_tvl1, gray, **kw)
    p = _ffi.default_tvl1_params(**kw)
    L = _ffi.lib()
    S, F = gray.shape[:2]
    nbytes = L.va_tvl1_workspace_bytes(W, H, S, F, ctypes.byref(p))
    assert nbytes > 0, L.va_last_error()
    frames = gray.cuda()
    buf = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    flow = torch.empty((S * (F - 1), 2, H, W), dtype=torch.float32, device="cuda")
    _ffi.check(L.va_tvl1_flow(_ffi.ctx(0), _ffi.ptr(frames), 1, S, F, W, H, ctypes.byref(p), _ffi.ptr(flow), _ffi.ptr(buf), nbytes,
                              _ffi.stream_ptr(frames.device)))
    torch.cuda.synchronize()
    assert bool((buf[nbytes:] == 0xA5).all()), "bytes past the declared workspace were written"
    assert np.array_equal(flow.cpu().numpy(), ref), "max abs diff %g" % np.nanmax(np.abs(flow.cpu().numpy() - ref))


# ------------------------------------------------------------------------------------------------ rejected parameters

@pytest.mark.parametrize("over", [
    dict(scale_step=0.0), dict(scale_step=1.0), dict(scale_step=float("nan")),
    dict(tau=0.0), dict(tau=-0.25), dict(tau=float("nan")), dict(lambda_=0.0), dict(lambda_=-0.15), dict(lambda_=float("nan")),
    dict(theta=0.0), dict(theta=-0.3), dict(theta=float("nan")),
    dict(tau=1.0, theta=0.0005), dict(lambda_=100.0, theta=20.0), dict(nscales=0),
], ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_bad_parameters_raise_value_error(over):
    # the wrapper turns va_tvl1_workspace_bytes == 0 into ValueError before anything is launched (tests/test_abi.py checks the
    # messages on the host); `lambda` is also accepted under its C name
    from video_analytics_amd import flow as vflow
    fr = torch.zeros(1, 2, 64, 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        vflow.tvl1_flow(fr, **over)
    if "lambda_" in over:
        with pytest.raises(ValueError):
            vflow.tvl1_flow(fr, **{("lambda" if k == "lambda_" else k): v for k, v in over.items()})
