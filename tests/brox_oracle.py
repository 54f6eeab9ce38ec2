"""The executable form of DESIGN.md S57-S62 (Brox optical flow) -- TEST INFRASTRUCTURE, never imported by the product.

numpy float32, elementwise operations only, every expression in the operation order the specification writes (no sum, mean
or dot on the result path: their order is numpy's; no fused multiply-add: numpy has none).  IEEE binary32 addition,
multiplication, division and square root are correctly rounded in numpy as they are on the device, so the library has to
reproduce these arrays bit for bit, whatever its tiling.

S1 (pyramid), S2 (centred gradient) and S8 (upsampling) are TV-L1's and come from the built C oracle of that method:
``tvl1_oracle.zoom_out``, ``ora_tvl1_centered_gradient`` and ``ora_tvl1_upsample_flow``, bound here.
"""
import ctypes

import numpy as np

from oracle import tvl1_oracle

f32 = np.float32

DEFAULTS = dict(alpha=0.197, gamma=50.0, scale_step=0.8, omega=1.9, epsilon=1e-3, nscales=16, warps=1, inner_iters=10,
                solver_iters=10)


def params(**over):
    p = dict(DEFAULTS)
    for k in over:
        if k not in p:
            raise ValueError("unknown Brox parameter %r" % k)
    p.update(over)
    return p


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _lib():
    L = tvl1_oracle.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    L.ora_tvl1_upsample_flow.argtypes = [fp, ctypes.c_int, ctypes.c_int, fp, ctypes.c_int, ctypes.c_int, ctypes.c_float]
    L.ora_tvl1_upsample_flow.restype = None
    return L


def gradient(img):
    """S2 -> (Ix, Iy)"""
    img = np.ascontiguousarray(img, dtype=f32)
    h, w = img.shape
    ix, iy = np.empty_like(img), np.empty_like(img)
    _lib().ora_tvl1_centered_gradient(_fp(img), w, h, _fp(ix), _fp(iy))
    return ix, iy


def upsample(uc, fw, fh, step):
    """S8"""
    uc = np.ascontiguousarray(uc, dtype=f32)
    ch, cw = uc.shape
    uf = np.empty((fh, fw), dtype=f32)
    _lib().ora_tvl1_upsample_flow(_fp(uc), cw, ch, _fp(uf), fw, fh, step)
    return uf


def bilinear(img, px, py):
    """S12's bilinear form: clamped position, plain float32 interpolation"""
    h, w = img.shape
    xc = np.minimum(np.maximum(px, f32(0)), f32(w - 1))
    yc = np.minimum(np.maximum(py, f32(0)), f32(h - 1))
    x0, y0 = np.floor(xc).astype(np.int64), np.floor(yc).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = xc - x0.astype(f32), yc - y0.astype(f32)
    a, b, c, d = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    top = a + ax * (b - a)
    bot = c + ax * (d - c)
    return top + ay * (bot - top)


def derivatives(img):
    """S57: (I, Ix, Iy, Ixx, Ixy, Iyy); Ixy is the x derivative of Iy"""
    ix, iy = gradient(img)
    ixx, _ = gradient(ix)
    ixy, iyy = gradient(iy)
    return img, ix, iy, ixx, ixy, iyy


def warp(d0, d1, u, v):
    """S58, S59 -> dict of the fields an inner step reads (and I1w)"""
    h, w = u.shape
    px = np.arange(w, dtype=f32)[None, :] + u
    py = np.arange(h, dtype=f32)[:, None] + v
    I1w, Ix, Iy, Ixx, Ixy, Iyy = (bilinear(f, px, py) for f in d1)
    return dict(I1w=I1w, Ix=Ix, Iy=Iy, Ixx=Ixx, Ixy=Ixy, Iyy=Iyy, Iz=I1w - d0[0], Ixz=Ix - d0[1], Iyz=Iy - d0[2])


def _nb(a):
    """the four neighbours with clamped indices: left, right, up, down"""
    p = np.pad(a, 1, mode="edge")
    return p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]


def coefficients(f, u, v, du, dv, p):
    """S60 -> dict(A12, D1, D2, b1, b2, wL, wR, wU, wD)"""
    alpha, gamma = f32(p["alpha"]), f32(p["gamma"])
    eps2 = f32(p["epsilon"]) * f32(p["epsilon"])
    h, w = u.shape
    half = f32(0.5)
    U, V = u + du, v + dv
    Ul, Ur, Ut, Ub = _nb(U)
    Vl, Vr, Vt, Vb = _nb(V)
    ux, uy = half * (Ur - Ul), half * (Ub - Ut)
    vx, vy = half * (Vr - Vl), half * (Vb - Vt)
    ps = alpha / np.sqrt(((ux * ux + uy * uy) + (vx * vx + vy * vy)) + eps2)
    pl, pr, pt, pb = _nb(ps)
    xs, ys = np.arange(w)[None, :], np.arange(h)[:, None]
    zero = np.zeros_like(ps)
    wL = np.where(xs > 0, half * (ps + pl), zero)
    wR = np.where(xs < w - 1, half * (ps + pr), zero)
    wU = np.where(ys > 0, half * (ps + pt), zero)
    wD = np.where(ys < h - 1, half * (ps + pb), zero)
    sw = (wL + wR) + (wU + wD)
    ul, ur, ut, ub = _nb(u)
    vl, vr, vt, vb = _nb(v)
    divu = (wL * (ul - u) + wR * (ur - u)) + (wU * (ut - u) + wD * (ub - u))
    divv = (wL * (vl - v) + wR * (vr - v)) + (wU * (vt - v) + wD * (vb - v))
    Ix, Iy, Ixx, Ixy, Iyy, Iz, Ixz, Iyz = (f[k] for k in ("Ix", "Iy", "Ixx", "Ixy", "Iyy", "Iz", "Ixz", "Iyz"))
    q = (Iz + Ix * du) + Iy * dv
    pD = f32(1) / np.sqrt(q * q + eps2)
    g1 = (Ixz + Ixx * du) + Ixy * dv
    g2 = (Iyz + Ixy * du) + Iyy * dv
    pG = gamma / np.sqrt((g1 * g1 + g2 * g2) + eps2)
    A11 = pD * (Ix * Ix) + pG * (Ixx * Ixx + Ixy * Ixy)
    A22 = pD * (Iy * Iy) + pG * (Ixy * Ixy + Iyy * Iyy)
    A12 = pD * (Ix * Iy) + pG * (Ixx * Ixy + Ixy * Iyy)
    b1 = divu - (pD * (Ix * Iz) + pG * (Ixx * Ixz + Ixy * Iyz))
    b2 = divv - (pD * (Iy * Iz) + pG * (Ixy * Ixz + Iyy * Iyz))
    return dict(A12=A12, D1=A11 + sw, D2=A22 + sw, b1=b1, b2=b2, wL=wL, wR=wR, wU=wU, wD=wD)


def sweep(c, du, dv, omega):
    """S61: one red-black SOR sweep, (x + y) even first -> (du, dv)"""
    omega = f32(omega)
    om1 = f32(1) - omega
    h, w = du.shape
    odd = ((np.arange(w)[None, :] + np.arange(h)[:, None]) & 1).astype(bool)
    for colour in (False, True):
        m = odd == colour
        l, r, t, b = _nb(du)
        su = (c["wL"] * l + c["wR"] * r) + (c["wU"] * t + c["wD"] * b)
        ndu = om1 * du + omega * (((c["b1"] + su) - c["A12"] * dv) / c["D1"])
        l, r, t, b = _nb(dv)
        sv = (c["wL"] * l + c["wR"] * r) + (c["wU"] * t + c["wD"] * b)
        ndv = om1 * dv + omega * (((c["b2"] + sv) - c["A12"] * ndu) / c["D2"])
        du, dv = np.where(m, ndu, du), np.where(m, ndv, dv)
    return du, dv


def inner_step(f, u, v, du, dv, p):
    """one lagged-nonlinearity step: S60's coefficients from (du, dv), then solver_iters sweeps"""
    with np.errstate(all="ignore"):
        c = coefficients(f, u, v, du, dv, p)
        for _ in range(p["solver_iters"]):
            du, dv = sweep(c, du, dv, p["omega"])
    return du, dv


def pyramid(img, p):
    """S57 + S1: the levels of one frame (gray values / 255), finest first"""
    img = np.asarray(img, dtype=f32) / f32(255)
    h, w = img.shape
    sizes = tvl1_oracle.pyramid_sizes(w, h, p["nscales"], p["scale_step"])
    levels = [np.ascontiguousarray(img)]
    for (lw, lh) in sizes[1:]:
        levels.append(tvl1_oracle.zoom_out(levels[-1], p["scale_step"]))
        assert levels[-1].shape == (lh, lw)
    return levels


def level(d0, d1, u, v, p):
    """S58-S61 on one level -> (u, v)"""
    for _ in range(p["warps"]):
        f = warp(d0, d1, u, v)
        du, dv = np.zeros_like(u), np.zeros_like(v)
        for _ in range(p["inner_iters"]):
            du, dv = inner_step(f, u, v, du, dv, p)
        u, v = u + du, v + dv
    return u, v


def flow_pair(i0, i1, p):
    """two gray frames [H,W] in [0,255] -> flow [2,H,W] float32"""
    p0, p1 = pyramid(i0, p), pyramid(i1, p)
    u = np.zeros_like(p0[-1])
    v = np.zeros_like(p0[-1])
    for s in range(len(p0) - 1, -1, -1):
        u, v = level(derivatives(p0[s]), derivatives(p1[s]), u, v, p)
        if s > 0:
            fh, fw = p0[s - 1].shape
            u, v = upsample(u, fw, fh, p["scale_step"]), upsample(v, fw, fh, p["scale_step"])
    return np.stack([u, v])


def brox_flow(frames, p=None):
    """frames uint8/float32 [S,F,H,W] (or [F,H,W]) -> flow float32 [S*(F-1),2,H,W], ``flow.brox_flow``'s layout"""
    p = p if p is not None else params()
    fr = np.asarray(frames)
    if fr.ndim == 3:
        fr = fr[None]
    S, F = fr.shape[:2]
    return np.stack([flow_pair(fr[s, k], fr[s, k + 1], p) for s in range(S) for k in range(F - 1)]).astype(f32)
