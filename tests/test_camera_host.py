"""Host side of warped optical flow: the numpy float64 restatements of the homography fit and of the
camera compensation that tests/test_camera_gpu.py holds the kernels to, an independent float64 witness of the fit (every
entry of the normal equations from the explicit rows, summed by math.fsum, solved by numpy.linalg.solve), the recovery of a
planted homography under outlier boxes and noise, degenerate fields, and the refusal of bad options before anything reaches
the GPU."""
import math

import numpy as np
import pytest
import torch

F32 = np.float32
K, C0_SQ, CMIN_SQ = 16, 256.0, 1.0

PLANTED = np.array([[1.01, -0.008, 1.7],
                    [0.006, 0.988, -0.9],
                    [2e-5, -1.5e-5, 1.0]])


# ---- S21 restated ----

def _normalised(field):
    """field float32 [2,h,w] -> (u, v, du, dv, valid, s, cx, cy), flat float64 arrays in pixel order."""
    _, h, w = field.shape
    s = 2.0 / max(w, h)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    valid = (np.isfinite(field[0]) & np.isfinite(field[1])).ravel()
    u, v = ((x - cx) * s).ravel(), ((y - cy) * s).ravel()
    with np.errstate(invalid="ignore"):
        du = np.where(valid, field[0].astype(np.float64).ravel() * s, 0.0)
        dv = np.where(valid, field[1].astype(np.float64).ravel() * s, 0.0)
    return u, v, du, dv, valid, s, cx, cy


def _weights(g, u, v, up, vp, valid, s, c2):
    """Tukey's biweight of the transfer error of g in pixels; invalid pixels and non-finite errors weigh 0."""
    with np.errstate(all="ignore"):
        X = u + ((g[0] * u + g[1] * v) + g[2])
        Y = v + ((g[3] * u + g[4] * v) + g[5])
        D = 1.0 + (g[6] * u + g[7] * v)
        ex, ey = X / D - up, Y / D - vp
        e2 = (ex * ex + ey * ey) / (s * s)
        t = 1.0 - e2 / c2
        return np.where(valid & (t > 0.0), t * t, 0.0)


def _scale_sq(k, c0_sq, cmin_sq):
    """c_k^2, the squared scale of the weights that follow solve k."""
    return max(cmin_sq, math.ldexp(c0_sq, -k))


def _cholesky_solve(M, r):
    """S21's solve -> g, or None for a degenerate system (a pivot not finite or not above 2^-40 x the largest diagonal)."""
    n = M.shape[0]
    floor = max(M[i, i] for i in range(n)) * 2.0 ** -40
    Lo = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            d = M[j, j]
            for q in range(j):
                d -= Lo[j, q] * Lo[j, q]
            if not (np.isfinite(d) and d > floor):
                return None
            Lo[j, j] = math.sqrt(d)
            for i in range(j + 1, n):
                e = M[i, j]
                for q in range(j):
                    e -= Lo[i, q] * Lo[j, q]
                Lo[i, j] = e / Lo[j, j]
        y = np.zeros(n)
        for i in range(n):
            e = r[i]
            for q in range(i):
                e -= Lo[i, q] * y[q]
            y[i] = e / Lo[i, i]
        g = np.zeros(n)
        for i in range(n - 1, -1, -1):
            e = y[i]
            for q in range(i + 1, n):
                e -= Lo[q, i] * g[q]
            g[i] = e / Lo[i, i]
    return g


def _pixel_homography(g, s, cx, cy):
    """H = T^-1 (I + G) T divided by its [2][2] entry, T = (s 0 -cx s; 0 s -cy s; 0 0 1), written out."""
    a = np.array([[1.0 + g[0], g[1], g[2]], [g[3], 1.0 + g[4], g[5]], [g[6], g[7], 1.0]])
    b = np.empty((3, 3))
    for i in range(3):
        b[i, 0], b[i, 1], b[i, 2] = a[i, 0] * s, a[i, 1] * s, a[i, 2] - (a[i, 0] * cx + a[i, 1] * cy) * s
    Hm = np.empty((3, 3))
    Hm[0] = b[0] / s + cx * b[2]
    Hm[1] = b[1] / s + cy * b[2]
    Hm[2] = b[2]
    return Hm / b[2, 2]


def s21_fit(flow, iters=K, c0_sq=C0_SQ, cmin_sq=CMIN_SQ, order=None):
    """S21 restated in float64: flow float32 [N,2,h,w] -> (H [N,3,3], stats [N,2]).  The distinct sums of the normal
    equations are numpy sums over the pixels (in the order ``order`` when given: a permutation of the h*w pixels)."""
    flow = np.asarray(flow, dtype=np.float32)
    N, _, h, w = flow.shape
    Hs, stats = np.tile(np.eye(3), (N, 1, 1)), np.zeros((N, 2))
    for n in range(N):
        u, v, du, dv, valid, s, cx, cy = _normalised(flow[n])
        if order is not None:
            u, v, du, dv, valid = u[order], v[order], du[order], dv[order], valid[order]
        up, vp = u + du, v + dv
        om = valid.astype(np.float64)
        g = None
        for k in range(iters):
            if k > 0:
                om = _weights(g, u, v, up, vp, valid, s, _scale_sq(k - 1, c0_sq, cmin_sq))
            wu, wv = om * u, om * v
            tuu, tuv, tvv = wu * u, wu * v, wv * v
            q, z = up * up + vp * vp, up * du + vp * dv
            S = lambda a: float(np.sum(a))
            blk = np.array([[S(tuu), S(tuv), S(wu)], [S(tuv), S(tvv), S(wv)], [S(wu), S(wv), S(om)]])
            M = np.zeros((8, 8))
            M[0:3, 0:3] = M[3:6, 3:6] = blk
            for r0, p in ((0, up), (3, vp)):
                c = np.array([[S(tuu * p), S(tuv * p)], [S(tuv * p), S(tvv * p)], [S(wu * p), S(wv * p)]])
                M[r0:r0 + 3, 6:8] = -c
                M[6:8, r0:r0 + 3] = -c.T
            M[6, 6], M[6, 7], M[7, 6], M[7, 7] = S(tuu * q), S(tuv * q), S(tuv * q), S(tvv * q)
            r = np.array([S(wu * du), S(wv * du), S(om * du), S(wu * dv), S(wv * dv), S(om * dv), -S(wu * z), -S(wv * z)])
            stats[n, 0] = S(om) / (float(w) * float(h))
            g = _cholesky_solve(M, r)
            if g is None:
                stats[n, 1] = 1.0
                break
        if g is not None:
            Hs[n] = _pixel_homography(g, s, cx, cy)
    return Hs, stats


def s21_witness(flow, iters=K, c0_sq=C0_SQ, cmin_sq=CMIN_SQ):
    """An independent float64 witness of S21 for well-posed fields: the two rows a1, a2 of every pixel written out, every
    entry of M and r summed by math.fsum (exactly rounded), numpy.linalg.solve for g, and H by matrix products."""
    flow = np.asarray(flow, dtype=np.float32)
    N, _, h, w = flow.shape
    Hs, stats = np.empty((N, 3, 3)), np.zeros((N, 2))
    for n in range(N):
        u, v, du, dv, valid, s, cx, cy = _normalised(flow[n])
        up, vp = u + du, v + dv
        one, zero = np.ones_like(u), np.zeros_like(u)
        a1 = np.stack([u, v, one, zero, zero, zero, -up * u, -up * v])
        a2 = np.stack([zero, zero, zero, u, v, one, -vp * u, -vp * v])
        om = valid.astype(np.float64)
        for k in range(iters):
            if k > 0:
                om = _weights(g, u, v, up, vp, valid, s, _scale_sq(k - 1, c0_sq, cmin_sq))
            M, r = np.zeros((8, 8)), np.zeros(8)
            for i in range(8):
                for j in range(i, 8):
                    if (i < 3 and 3 <= j < 6):
                        continue  # a1 and a2 share no entry there
                    M[i, j] = M[j, i] = math.fsum((om * (a1[i] * a1[j] + a2[i] * a2[j])).tolist())
                r[i] = math.fsum((om * (a1[i] * du + a2[i] * dv)).tolist())
            g = np.linalg.solve(M, r)
        stats[n, 0] = math.fsum(om.tolist()) / (w * h)
        T = np.array([[s, 0.0, -cx * s], [0.0, s, -cy * s], [0.0, 0.0, 1.0]])
        A = np.array([[1.0 + g[0], g[1], g[2]], [g[3], 1.0 + g[4], g[5]], [g[6], g[7], 1.0]])
        Hm = np.linalg.inv(T) @ A @ T
        Hs[n] = Hm / Hm[2, 2]
    return Hs, stats


# ---- S22 restated ----

def camera_displacement(Hm, h, w):
    """The displacement field of one homography in float64, S22's arithmetic: -> (cx, cy) [h,w]."""
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        X = Hm[0, 0] * x + Hm[0, 1] * y + Hm[0, 2]
        Y = Hm[1, 0] * x + Hm[1, 1] * y + Hm[1, 2]
        D = Hm[2, 0] * x + Hm[2, 1] * y + Hm[2, 2]
        return X / D - x, Y / D - y


def s22_compensate(flow, Hs):
    """S22 restated: flow float32 [N,2,h,w], Hs float64 [N,3,3] -> float32 of the same shape."""
    flow = np.asarray(flow, dtype=np.float32)
    N, _, h, w = flow.shape
    out = np.empty_like(flow)
    with np.errstate(all="ignore"):
        for n in range(N):
            cx, cy = camera_displacement(Hs[n], h, w)
            out[n, 0] = flow[n, 0] - cx.astype(np.float32)
            out[n, 1] = flow[n, 1] - cy.astype(np.float32)
    return out


def same_bits(a, b):
    """Equal float32 arrays, a NaN matching a NaN."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=True))


def corner_gap(Ha, Hb, h, w):
    """The largest distance in pixels between the displacements two homographies give the four frame corners."""
    worst = 0.0
    for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
        p = np.array([x, y, 1.0])
        a, b = Ha @ p, Hb @ p
        worst = max(worst, float(np.hypot(a[0] / a[2] - b[0] / b[2], a[1] / a[2] - b[1] / b[2])))
    return worst


# ---- planted fields ----

BOXES = [("none", 0.0)] + [(where, share) for share in (0.10, 0.20) for where in ("corner", "centre", "edge")]


def planted_flow(h, w, where="none", share=0.0, sigma=0.0, seed=0, Hm=PLANTED):
    """The flow of the planted homography as float32 [1,2,h,w]; a box of ``share`` of the frame (the frame's aspect) at a
    corner, the centre or the middle of the left edge moves by another (+6, -4) px; Gaussian noise of ``sigma`` px."""
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    p = np.einsum("ij,jhw->ihw", Hm, np.stack([x, y, np.ones_like(x)]))
    d = np.stack([p[0] / p[2] - x, p[1] / p[2] - y])
    if share > 0.0:
        bh, bw = int(round(h * math.sqrt(share))), int(round(w * math.sqrt(share)))
        top, left = {"corner": (0, 0), "centre": ((h - bh) // 2, (w - bw) // 2), "edge": ((h - bh) // 2, 0)}[where]
        d[0, top:top + bh, left:left + bw] += 6.0
        d[1, top:top + bh, left:left + bw] -= 4.0
    if sigma > 0.0:
        d = d + np.random.RandomState(seed).standard_normal(d.shape) * sigma
    return d.astype(np.float32)[None]


def recovery_error(Hm, h, w, planted=PLANTED):
    """The largest distance over every pixel between the fitted and the planted camera displacement, in pixels."""
    ax, ay = camera_displacement(Hm, h, w)
    bx, by = camera_displacement(planted, h, w)
    return float(np.hypot(ax - bx, ay - by).max())


@pytest.mark.parametrize("h,w", [(240, 320), (241, 321), (29, 37)])
@pytest.mark.parametrize("where,share", BOXES)
def test_planted_homography_is_recovered_without_noise(h, w, where, share):
    Hs, stats = s21_fit(planted_flow(h, w, where, share))
    err = recovery_error(Hs[0], h, w)
    print("noise-free %dx%d %s %.2f: %.3g px, share %.4f" % (w, h, where, share, err, stats[0, 0]))
    assert stats[0, 1] == 0.0
    assert err <= 1e-6, err
    if (where, share) == ("corner", 0.20):
        assert abs(stats[0, 0] - 0.80) <= 0.02, stats[0, 0]


@pytest.mark.parametrize("h,w", [(240, 320), (241, 321)])
@pytest.mark.parametrize("where,share", BOXES)
def test_planted_homography_is_recovered_under_noise(h, w, where, share):
    Hs, stats = s21_fit(planted_flow(h, w, where, share, sigma=0.05, seed=h + int(100 * share)))
    err = recovery_error(Hs[0], h, w)
    print("sigma 0.05 %dx%d %s %.2f: %.3g px, share %.4f" % (w, h, where, share, err, stats[0, 0]))
    assert stats[0, 1] == 0.0
    assert err <= 1e-2, err


def test_restatement_agrees_with_the_witness():
    """The restatement's sums (numpy's pairwise order) and Cholesky against exactly rounded sums and LU."""
    for h, w, where, share in ((29, 37, "corner", 0.20), (48, 64, "centre", 0.10)):
        fl = planted_flow(h, w, where, share, sigma=0.05, seed=5)
        (Ha, sa), (Hb, sb) = s21_fit(fl), s21_witness(fl)
        assert corner_gap(Ha[0], Hb[0], h, w) <= 1e-10
        assert abs(sa[0, 0] - sb[0, 0]) <= 1e-10


def test_fit_is_insensitive_to_the_pixel_order():
    """The reference's own sensitivity to the summation order, which the device bound of 1e-9 px is set against."""
    h, w = 240, 320
    fl = planted_flow(h, w, "corner", 0.20, sigma=0.05, seed=11)
    Ha, _ = s21_fit(fl)
    worst = 0.0
    for seed in (0, 1):
        Hb, _ = s21_fit(fl, order=np.random.RandomState(seed).permutation(h * w))
        worst = max(worst, corner_gap(Ha[0], Hb[0], h, w))
    print("order sensitivity: %.3g px" % worst)
    assert worst <= 1e-10, worst


def test_a_nan_pixel_changes_nothing_but_its_own_weight():
    h, w = 48, 64
    fl = planted_flow(h, w, "centre", 0.10)
    Ha, sa = s21_fit(fl)
    hit = fl.copy()
    hit[0, 0, 3, 5] = np.nan
    hit[0, 1, 40, 60] = np.inf
    Hb, sb = s21_fit(hit)
    assert sb[0, 1] == 0.0 and corner_gap(Ha[0], Hb[0], h, w) <= 1e-6
    assert abs((sa[0, 0] - sb[0, 0]) * h * w - 2.0) <= 1e-3  # the two inliers' weights, each close to 1
    Hw, sw = s21_witness(hit)  # whose rows of the two pixels are finite and weighted 0
    assert corner_gap(Hb[0], Hw[0], h, w) <= 1e-10 and abs(sb[0, 0] - sw[0, 0]) <= 1e-10


def test_degenerate_fields_give_the_identity_and_status_1():
    for fl in (np.zeros((1, 2, 1, 1), F32), np.ones((2, 2, 1, 2), F32), np.full((1, 2, 24, 32), np.nan, F32),
               np.zeros((1, 2, 1, 9), F32)):
        Hs, stats = s21_fit(fl)
        assert np.array_equal(Hs, np.tile(np.eye(3), (fl.shape[0], 1, 1)))
        assert np.array_equal(stats[:, 1], np.ones(fl.shape[0]))
    assert s21_fit(np.full((1, 2, 24, 32), np.nan, F32))[1][0, 0] == 0.0
    mixed = np.concatenate([planted_flow(24, 32), np.full((1, 2, 24, 32), np.nan, F32)])
    Hs, stats = s21_fit(mixed)
    assert stats[:, 1].tolist() == [0.0, 1.0] and recovery_error(Hs[0], 24, 32) <= 1e-6


def test_s22_with_the_identity_returns_the_input_bits():
    rs = np.random.RandomState(2)
    fl = (rs.standard_normal((3, 2, 29, 37)) * 12).astype(np.float32)
    fl[0, 0, 0, 0], fl[1, 1, 5, 5], fl[2, 0, 3, 3] = np.nan, -0.0, np.inf
    out = s22_compensate(fl, np.tile(np.eye(3), (3, 1, 1)))
    assert np.array_equal(out.view(np.uint32)[~np.isnan(fl)], fl.view(np.uint32)[~np.isnan(fl)])
    assert np.array_equal(np.isnan(out), np.isnan(fl))


@pytest.mark.parametrize("h,w", [(240, 320), (29, 37)])
def test_s22_of_the_planted_flow_is_zero_within_two_ulp(h, w):
    fl = planted_flow(h, w)
    out = s22_compensate(fl, PLANTED[None])
    assert np.all(np.abs(out) <= 2 * np.spacing(np.abs(fl)))
    boxed = planted_flow(h, w, "centre", 0.10)
    res = s22_compensate(boxed, PLANTED[None])
    assert abs(float(res[0, 0, h // 2, w // 2]) - 6.0) < 1e-5 and abs(float(res[0, 1, h // 2, w // 2]) + 4.0) < 1e-5


# ---- option checks: before anything reaches the GPU ----

@pytest.fixture
def no_gpu_calls(monkeypatch):
    """Every path to the device raises AssertionError: a ValueError seen with it comes from a host check."""
    from video_analytics_amd import _ffi
    from video_analytics_amd import flow as vflow

    def boom(*a, **k):
        raise AssertionError("reached the GPU")
    for mod, name in ((_ffi, "ctx"), (_ffi, "lib"), (vflow, "tvl1_flow"), (vflow, "tvl1_flow_concurrent")):
        monkeypatch.setattr(mod, name, boom)


@pytest.mark.parametrize("camera", ["affine", "Homography", None, 1, ("homography",)])
def test_an_unknown_camera_is_refused_on_the_host(no_gpu_calls, camera):
    from video_analytics_amd import augment, pipeline
    from video_analytics_amd import flow as vflow
    from video_analytics_amd.temporalModel import flowVolumesFromFrames
    with pytest.raises(ValueError, match="camera"):
        vflow.check_motion("stack", False, 10, "x", camera=camera)
    gray = torch.zeros(2, 11, 240, 320, dtype=torch.uint8)
    for extra in (dict(), dict(views=augment.ten_crop_views(240, 320)), dict(motion="trajectory", mean_flow=True)):
        with pytest.raises(ValueError, match="camera"):
            flowVolumesFromFrames(gray, camera=camera, **extra)
    with pytest.raises(ValueError, match="camera"):
        pipeline.TwoStreamPipeline(device=0, camera=camera)


def test_the_camera_names_and_defaults(no_gpu_calls):
    import inspect
    from video_analytics_amd import pipeline
    from video_analytics_amd import flow as vflow
    from video_analytics_amd.temporalModel import flowVolumesFromFrames
    assert vflow.CAMERAS == ("none", "homography")
    for cam in vflow.CAMERAS:
        vflow.check_motion("stack", True, 10, "x", camera=cam)
    vflow.check_motion("stack", True, 10, "x")  # the existing four-argument call
    for f in (vflow.check_motion, vflow.apply_motion, flowVolumesFromFrames, pipeline.TwoStreamPipeline.__init__):
        params = list(inspect.signature(f).parameters.values())
        assert params[-1].name == "camera" and params[-1].default == "none", f
    flow = torch.zeros(2, 2, 8, 8)
    assert vflow.apply_motion(flow, 2) is flow and vflow.apply_motion(flow, 2, camera="none") is flow  # no kernel, no buffer


def test_camera_helpers_refuse_bad_arguments_on_the_host(no_gpu_calls):
    from video_analytics_amd import flow as vflow
    cpu = torch.zeros(4, 2, 8, 8)
    eye = torch.eye(3, dtype=torch.float64).repeat(4, 1, 1)
    for f in (lambda: vflow.fit_homography(cpu), lambda: vflow.fit_homography(torch.zeros(4, 3, 8, 8)),
              lambda: vflow.compensate_camera(cpu, eye), lambda: vflow.apply_motion(cpu, 2, camera="homography"),
              lambda: vflow.fit_homography(cpu, iters=0), lambda: vflow.fit_homography(cpu, c0=1.0, c_min=2.0),
              lambda: vflow.fit_homography(cpu, c_min=0.0), lambda: vflow.fit_homography(cpu, c0=float("nan"))):
        with pytest.raises(ValueError):
            f()


def test_precomputed_flow_volumes_refuse_a_camera_on_the_host(no_gpu_calls):
    """``flow_stack=`` is already quantised: a pipeline with a camera refuses it before anything is enqueued."""
    from video_analytics_amd import pipeline
    pipe = pipeline.TwoStreamPipeline.__new__(pipeline.TwoStreamPipeline)
    pipe.motion, pipe.mean_flow, pipe.camera, pipe._n = "stack", False, "homography", 0
    with pytest.raises(ValueError, match="camera"):
        pipe.submit(torch.zeros(2, 3, 224, 224, dtype=torch.uint8), None, flow_stack=torch.zeros(2, 20, 224, 224))
    assert pipe._n == 0
