"""Pins of the TV-L1 CPU oracle (oracle/tvl1_oracle.c).  PARITY UNPINNED against the reference: it
has no TV-L1 code or fixtures.  The pins are (1) analytic known answers of the
published algorithm, (2) direct numpy restatements of single steps, (3) the committed outputs in
tests/golden/tvl1_64x48.npz (tests/golden/make_golden.py)."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _texture(H, W, seed=0, margin=16):
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    big = gaussian_filter(rng.uniform(0, 1, (H + 2 * margin, W + 2 * margin)), 2.0)
    return (big - big.min()) / (big.max() - big.min()) * 255.0


def _shift(big, H, W, dx, dy, margin=16):
    from scipy.ndimage import map_coordinates
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return map_coordinates(big, [yy + margin + dy, xx + margin + dx], order=3).astype(np.float32)


def test_zero_motion_gives_exactly_zero_flow(oracle_tvl1):
    big = _texture(64, 80)
    f = _shift(big, 64, 80, 0, 0)
    fl = oracle_tvl1.tvl1_flow(np.stack([f, f])[None])
    assert fl.shape == (1, 2, 64, 80) and np.all(fl == 0.0)


@pytest.mark.parametrize("d", [(1.5, -0.75), (-2.0, 1.0)])
def test_constant_translation_is_recovered(oracle_tvl1, d):
    H, W = 96, 128
    big = _texture(H, W, seed=1)
    f0 = _shift(big, H, W, 0, 0)
    f1 = _shift(big, H, W, -d[0], -d[1])  # I1(x) = I0(x - d)  =>  flow = d
    fl = oracle_tvl1.tvl1_flow(np.stack([f0, f1])[None], oracle_tvl1.default_params(epsilon=0.0, iters=100))
    c = fl[0][:, 16:-16, 16:-16]
    assert abs(c[0].mean() - d[0]) < 0.02 and abs(c[1].mean() - d[1]) < 0.02
    assert c[0].std() < 0.05 and c[1].std() < 0.05


def test_pyramid_sizes_known_answers(oracle_tvl1):
    assert oracle_tvl1.pyramid_sizes(224, 224) == [(224, 224), (179, 179), (143, 143), (114, 114), (91, 91)]
    assert oracle_tvl1.pyramid_sizes(1280, 720) == [(1280, 720), (1024, 576), (819, 461), (655, 369), (524, 295)]
    assert oracle_tvl1.pyramid_sizes(20, 20) == [(20, 20), (16, 16)]  # stops before min(w,h) < 16
    assert oracle_tvl1.pyramid_sizes(64, 48, nscales=1) == [(64, 48)]


def test_zoom_out_preserves_constants_and_ramps(oracle_tvl1):
    const = np.full((40, 50), 37.0, dtype=np.float32)
    out = oracle_tvl1.zoom_out(const)
    assert out.shape == (32, 40) and np.allclose(out, 37.0, atol=1e-4)
    ramp = np.tile(np.arange(50, dtype=np.float32), (40, 1))
    out = oracle_tvl1.zoom_out(ramp)
    # a linear ramp survives a symmetric smoothing; sampling at x * (50/40)
    assert np.allclose(out[5, 5:35], np.arange(5, 35) * np.float32(50.0 / 40.0), atol=1e-3)


def test_single_iteration_against_numpy_restatement(oracle_tvl1):
    """One level, one warp, one inner iteration from u = 0, p = 0, restated in float64 numpy."""
    import ctypes
    rng = np.random.default_rng(3)
    H, W = 20, 24
    I0 = rng.uniform(0, 255, (H, W)).astype(np.float32)
    I1 = rng.uniform(0, 255, (H, W)).astype(np.float32)
    Ix = np.empty_like(I1); Iy = np.empty_like(I1)
    L = oracle_tvl1.lib()
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    L.ora_tvl1_centered_gradient(fp(I1), W, H, fp(Ix), fp(Iy))
    gx = 0.5 * (I1[:, np.minimum(np.arange(W) + 1, W - 1)] - I1[:, np.maximum(np.arange(W) - 1, 0)])
    assert np.allclose(Ix, gx, atol=1e-5)
    u1 = np.zeros((H, W), np.float32); u2 = np.zeros((H, W), np.float32)
    P = oracle_tvl1.default_params(epsilon=0.0, iters=1, warps=1)
    n = L.ora_tvl1_level(fp(I0), fp(I1), fp(Ix), fp(Iy), W, H, ctypes.byref(P), fp(u1), fp(u2))
    assert n == 1
    # u = 0, p = 0: rho = I1 - I0, u' = clamp(-rho/grad, -l_t, l_t) * grad I1  (div p = 0)
    l_t = 0.15 * 0.3
    rho = I1.astype(np.float64) - I0
    grad = Ix.astype(np.float64) ** 2 + Iy.astype(np.float64) ** 2
    fi = np.clip(-rho / np.maximum(grad, 1e-30), -l_t, l_t) * (grad >= 1e-10)
    assert np.allclose(u1, fi * Ix, atol=1e-5) and np.allclose(u2, fi * Iy, atol=1e-5)


def test_flow_to_stack_known_answers(oracle_tvl1):
    fl = np.array([-25.0, -20.0, 0.0, 20.0, 30.0, 0.07843], dtype=np.float32).reshape(1, 2, 1, 3)
    st = oracle_tvl1.flow_to_stack(fl, bound=20.0, mean=0.485, std=0.229).reshape(-1)
    q = np.array([0, 0, 128, 255, 255, 128], dtype=np.float64)  # rint(127.5)=128 (half to even), rint(127.99..)=128
    assert np.allclose(st, (q / 255.0 - 0.485) / 0.229, atol=1e-6)


def test_golden_vectors(oracle_tvl1):
    g = np.load(os.path.join(GOLD, "tvl1_64x48.npz"))
    fixed = oracle_tvl1.tvl1_flow(g["gray"], oracle_tvl1.default_params(epsilon=0.0, iters=30, warps=3))
    assert np.array_equal(fixed, g["flow_fixed"])
    eps, iters = oracle_tvl1.tvl1_flow(g["gray"], oracle_tvl1.default_params(epsilon=0.01, iters=300), return_iters=True)
    assert np.array_equal(eps, g["flow_eps"]) and np.array_equal(iters, g["iters_eps"])
    assert np.array_equal(oracle_tvl1.flow_to_stack(fixed), g["stack_fixed"])
    # thread count does not change results (OpenMP is across pairs only)
    assert np.array_equal(oracle_tvl1.tvl1_flow(g["gray"], oracle_tvl1.default_params(epsilon=0.0, iters=30, warps=3), nthreads=1), fixed)


def test_bad_arguments(oracle_tvl1):
    with pytest.raises(ValueError):
        oracle_tvl1.tvl1_flow(np.zeros((1, 1, 32, 32), np.float32))  # a single frame
    with pytest.raises(ValueError):
        oracle_tvl1.tvl1_flow(np.zeros((1, 2, 32, 32), np.float32), oracle_tvl1.default_params(scale_step=1.2))


def _synth_gray(n_seq, n_frames, H, W, seed):
    from video_analytics_amd import synth
    return synth.synth_clips(n_seq, seed=seed, H=H, W=W, n_gray=n_frames)[1].numpy()


def _witness_errors(oracle_tvl1, gray=None, tau=0.25, lam=0.15, theta=0.3, step=0.8, nscales=5, **kw):
    """Per-pixel |C oracle - float64 IPOL witness| (max over the two flow components) for every pair of ``gray``
    [S,F,H,W] (default: the golden pairs), both sides at the same tau / lambda / theta / scale step / nscales."""
    from oracle import tvl1_ipol_f64 as W
    if gray is None:
        gray = np.load(os.path.join(GOLD, "tvl1_64x48.npz"))["gray"]
    ref = oracle_tvl1.tvl1_flow(gray, oracle_tvl1.default_params(epsilon=0.0, tau=tau, lambda_=lam, theta=theta, scale_step=step,
                                                                 nscales=nscales, **kw))
    errs, k = [], 0
    for s in range(gray.shape[0]):
        for j in range(gray.shape[1] - 1):
            u1, u2 = W.tvl1_flow_pair(gray[s, j], gray[s, j + 1], tau=tau, lam=lam, theta=theta, step=step, nscales=nscales, **kw)
            errs.append(np.maximum(np.abs(u1 - ref[k, 0]), np.abs(u2 - ref[k, 1])))
            k += 1
    return np.stack(errs), ref


def test_independent_float64_ipol_witness_short_schedules(oracle_tvl1):
    """oracle/tvl1_ipol_f64.py restates IPOL Algorithm 1 as published (three-case TH, one division per flow component,
    no regulariser, float64, vectorised) over the whole multi-level schedule; the C oracle (float32, one division per
    pixel, 2^-100 regulariser, clamp-form TH with 1/|grad|^2 := 0) must give the same flow.  Stated tolerances, px:
    golden schedule (5 levels x 3 warps x 30 iterations): max 5e-3, median 1e-5;
    one warp of 300 iterations per level: max 2e-3."""
    e, ref = _witness_errors(oracle_tvl1, iters=30, warps=3)
    assert float(np.abs(ref).max()) > 5.0  # the pairs carry real motion
    assert e.max() < 5e-3 and np.median(e) < 1e-5, (e.max(), np.median(e))
    e, _ = _witness_errors(oracle_tvl1, iters=300, warps=1)
    assert e.max() < 2e-3, e.max()


def test_independent_float64_ipol_witness_full_schedule(oracle_tvl1):
    """The benchmark schedule (5 x 5 x 300).  Stated tolerances: median 1e-4 px, at least 96 % of the pixels within
    1e-3 px, every pixel further than 8 px from the frame border within 1e-2 px.  The remaining pixels sit in frame
    corners where the flow (8 px and more) points out of the image: the warp coordinates clamp, the data term is
    degenerate there, and float32 / float64 evaluations of the SAME formulas drift apart by up to ~1 px over 7 500
    iterations (measured: the witness evaluated in float32 differs from itself in float64 by 0.9 px at the same
    pixels) -- conditioning of the problem, not a property of either restatement."""
    e, _ = _witness_errors(oracle_tvl1, iters=300, warps=5)
    assert np.median(e) < 1e-4, np.median(e)
    assert (e < 1e-3).mean() > 0.96, (e < 1e-3).mean()
    assert e[:, 8:-8, 8:-8].max() < 1e-2, e[:, 8:-8, 8:-8].max()


ZOOM_STEPS = [(0.95, 1), (0.9, 1), (0.8, 2), (0.65, 3), (0.5, 4), (0.4, 5), (0.3, 6), (0.25, 7), (0.2, 9), (0.1, 18)]


@pytest.mark.parametrize("step,radius", ZOOM_STEPS)
def test_zoom_out_stage_against_float64_witness_per_step(oracle_tvl1, step, radius):
    """One zoom-out (S1: Gaussian of radius min((int)(3 sigma) + 1, 8), then bilinear sampling) of a 96 x 128 synthetic frame
    against the float64 restatement, for filter radii 1 ... 7 and the two clamped ones (9 -> 8 at step 0.2, 18 -> 8 at 0.1).
    Bound 1e-3 gray values (of 0..255).  Measured max |C - float64| per step, in the order of ZOOM_STEPS:
    4.3e-4, 2.9e-4, 2.9e-4, 2.3e-4, 3.6e-5, 1.8e-4, 9.5e-5, 4.1e-5, 7.8e-5, 2.8e-5 (float32 taps and fmaf accumulation against
    float64; the sampling coordinate x * (w / ow) rounded in float32 dominates where it falls next to a pixel centre).
    Constants and linear ramps survive the symmetric, normalised filter at every step, the clamped ones included."""
    from oracle import tvl1_ipol_f64 as W
    R, taps = oracle_tvl1.zoom_taps(step)
    sigma = np.float32(0.6) * np.sqrt(np.float32(1.0) / (np.float32(step) * np.float32(step)) - np.float32(1.0))
    assert int(np.float32(3.0) * sigma) + 1 == radius and R == min(radius, 8)
    g = taps.astype(np.float64)
    assert abs(g.sum() - 1.0) < 1e-6 and np.array_equal(g, g[::-1]) and np.all(g > 0.0)

    img = _synth_gray(1, 1, 96, 128, seed=3)[0, 0].astype(np.float32)
    out = oracle_tvl1.zoom_out(img, step)
    oh, ow = out.shape
    assert (ow, oh) == (int(np.float32(128) * np.float32(step) + np.float32(0.5)), int(np.float32(96) * np.float32(step) + np.float32(0.5)))
    wit = W.zoom_out(img.astype(np.float64), ow, oh, step)
    d = float(np.abs(out - wit).max())
    assert d < 1e-3, d

    const = np.full((96, 128), 37.0, dtype=np.float32)
    assert np.allclose(oracle_tvl1.zoom_out(const, step), 37.0, atol=1e-4)
    for ramp, axis in ((np.tile(np.arange(128, dtype=np.float32), (96, 1)), 1), (np.tile(np.arange(96, dtype=np.float32)[:, None], (1, 128)), 0)):
        z = oracle_tvl1.zoom_out(ramp, step)
        n_in, n_out = ramp.shape[axis], z.shape[axis]
        pos = np.arange(n_out) * (np.float32(n_in) / np.float32(n_out))  # sampling positions in the filtered ramp
        keep = (pos >= R) & (pos <= n_in - 1 - R)  # where the filter support does not touch the replicated border
        assert keep.sum() >= 2
        line = z[3, :] if axis == 1 else z[:, 3]
        assert np.allclose(line[keep], pos[keep], atol=1e-3), np.abs(line - pos)[keep].max()


WITNESS_SETS = [  # tau, lambda, theta, scale_step, nscales, levels at 128 x 96
    (0.25, 0.15, 0.3, 0.5, 5, 3), (0.25, 0.15, 0.3, 0.65, 5, 5), (0.25, 0.15, 0.3, 0.9, 5, 5), (0.25, 0.15, 0.3, 0.3, 5, 2),
    (0.25, 0.15, 0.3, 0.2, 5, 2), (0.25, 0.15, 0.3, 0.9, 12, 12), (0.125, 0.05, 0.5, 0.8, 5, 5), (0.125, 0.05, 0.5, 0.8, 12, 9),
    (0.25, 0.02, 1.0, 0.8, 5, 5), (0.25, 0.02, 1.0, 0.8, 12, 9)]


@pytest.mark.parametrize("tau,lam,theta,step,nscales,levels", WITNESS_SETS)
def test_float64_ipol_witness_at_non_default_parameters(oracle_tvl1, tau, lam, theta, step, nscales, levels):
    """The whole schedule (3 warps x 30 iterations per level) away from the defaults, 2 pairs of 96 x 128 synthetic frames,
    held to the bounds test_independent_float64_ipol_witness_short_schedules states: max 5e-3 px, median 1e-5 px.
    Measured max / median, px, in the order of WITNESS_SETS:
    4.8e-5 / 5.8e-7, 2.4e-4 / 6.1e-7, 3.7e-4 / 6.2e-7, 1.0e-4 / 5.6e-7, 4.2e-4 / 5.9e-7, 2.1e-3 / 6.5e-7 (12 levels),
    9.8e-5 / 6.4e-7, 9.2e-5 / 6.4e-7, 7.5e-6 / 5.8e-7, 7.1e-6 / 5.6e-7."""
    assert len(oracle_tvl1.pyramid_sizes(128, 96, nscales, step)) == levels
    gray = _synth_gray(2, 2, 96, 128, seed=7)
    e, ref = _witness_errors(oracle_tvl1, gray, tau, lam, theta, step, nscales, iters=30, warps=3)
    assert np.isfinite(ref).all() and float(np.abs(ref).max()) > 1.0
    assert e.max() < 5e-3 and np.median(e) < 1e-5, (e.max(), np.median(e))


@pytest.mark.parametrize("tau,lam,theta,med_bound,interior_bound", [(0.25, 0.6, 0.3, 1.4e-5, 0.29), (0.1, 0.3, 0.15, 4e-6, 3.4e-3)])
def test_float64_ipol_witness_at_large_lambda_theta(oracle_tvl1, tau, lam, theta, med_bound, interior_bound):
    """lambda * theta of 0.18 and 0.045 with a small theta: the data step is large against the smoothing, and the frame
    border, where the flow points out of the image and the warp coordinates clamp, is ill-conditioned in the way
    test_independent_float64_ipol_witness_full_schedule documents; float32 and float64 evaluations of the same formulas
    part there.  No bound on the maximum therefore (measured 9.3 px and 0.16 px, at border pixels): the median and every
    pixel further than 8 px from the border are held, each to 4 x the value measured (other libm, other thread splits):
    (0.25, 0.6, 0.3): median 3.4e-6 px, interior 0.071 px;  (0.1, 0.3, 0.15): median 9.9e-7 px, interior 8.3e-4 px.
    The sets are kept because that amplification makes the GPU bit comparison of tests/test_tvl1_params_gpu.py most
    sensitive."""
    gray = _synth_gray(2, 2, 96, 128, seed=7)
    e, ref = _witness_errors(oracle_tvl1, gray, tau, lam, theta, 0.8, 5, iters=30, warps=3)
    assert np.isfinite(ref).all()
    assert np.median(e) < med_bound, np.median(e)
    assert e[:, 8:-8, 8:-8].max() < interior_bound, e[:, 8:-8, 8:-8].max()


def test_thresholding_operator_forms_agree():
    """The C oracle writes TH as clamp(-rho / |g|^2, -l_t, l_t) with 1/|g|^2 := 0 below 1e-10; IPOL writes three cases
    and keeps the +-l_t g branches for tiny gradients.  Where |g|^2 >= 1e-10 the two are the same function; below, the
    step they disagree on is at most l_t * |g| < 0.045 * 1e-5 px."""
    rng = np.random.default_rng(0)
    l_t = 0.15 * 0.3
    g = rng.normal(size=(2, 4000)) * 10.0 ** rng.uniform(-8, 2, size=4000)
    rho = rng.normal(size=4000) * 10.0 ** rng.uniform(-6, 2, size=4000)
    grad = (g ** 2).sum(0)
    three = np.where(rho < -l_t * grad, l_t, np.where(rho > l_t * grad, -l_t, np.where(grad < 1e-10, 0.0, -rho / np.maximum(grad, 1e-300))))
    clamp = np.clip(-rho * np.where(grad < 1e-10, 0.0, 1.0 / np.maximum(grad, 1e-300)), -l_t, l_t)
    big = grad >= 1e-10
    assert np.allclose(three[big], clamp[big], rtol=1e-12, atol=0)
    assert np.abs((three - clamp) * np.sqrt(grad))[~big].max() < l_t * 1e-5
