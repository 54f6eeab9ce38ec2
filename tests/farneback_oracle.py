"""The executable form of DESIGN.md S63-S67 (Farneback optical flow) -- TEST INFRASTRUCTURE, never imported by the product.

numpy float32, elementwise operations only, every expression in the operation order the specification writes (no sum, dot
or convolve on the result path: their order is numpy's; no fused multiply-add: numpy has none).  Tap loops are Python loops
over shifted, index-clamped arrays.  IEEE binary32 addition, multiplication and division are correctly rounded in numpy as
they are on the device, so the library has to reproduce these arrays bit for bit, whatever its tiling.

The constants (taps, inverse moments) are float64 scalars computed with ``math.exp`` in the written order and rounded to
float32 once, as the library's host code computes them.  S1 (pyramid) and S8 (upsampling) are TV-L1's and come from the built C
oracle of that method, as tests/brox_oracle.py binds them.
"""
import math

import numpy as np

import brox_oracle
from oracle import tvl1_oracle

f32 = np.float32

DEFAULTS = dict(pyr_scale=0.5, poly_sigma=1.2, levels=3, winsize=15, iterations=3, poly_n=5, gaussian=0)
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)
DET_REG = 1e-3


def params(**over):
    p = dict(DEFAULTS)
    for k in over:
        if k not in p:
            raise ValueError("unknown Farneback parameter %r" % k)
    p.update(over)
    return p


def poly_constants(p):
    """S64 -> (g, xg, xxg: float32 [n+1] for |k| = 0..n; ig11, ig03, ig33, ig55: float32)"""
    n = p["poly_n"]
    sigma = float(f32(p["poly_sigma"]))
    e = [math.exp(-float(k * k) / (2.0 * sigma * sigma)) for k in range(n + 1)]
    s = e[0]
    for k in range(1, n + 1):
        s = s + 2.0 * e[k]
    g, xg, xxg = [], [], []
    m2 = m4 = 0.0
    for k in range(n + 1):
        gk, k2 = e[k] / s, float(k * k)
        g.append(f32(gk))
        xg.append(f32(float(k) * gk))
        xxg.append(f32(k2 * gk))
        m2 = m2 + 2.0 * (k2 * gk)
        m4 = m4 + 2.0 * ((k2 * k2) * gk)
    d = m4 - m2 * m2
    return g, xg, xxg, f32(1.0 / m2), f32(-m2 / d), f32(1.0 / d), f32(1.0 / (m2 * m2))


def window_taps(p):
    """S66 -> float32 [m+1] for |i| = 0..m"""
    m = p["winsize"] // 2
    if not p["gaussian"]:
        return [f32(1.0 / float(p["winsize"]))] * (m + 1)
    sigma = 0.3 * float(m)
    e = [math.exp(-float(i * i) / (2.0 * sigma * sigma)) for i in range(m + 1)]
    s = e[0]
    for i in range(1, m + 1):
        s = s + 2.0 * e[i]
    return [f32(e[i] / s) for i in range(m + 1)]


def _shift(a, k, axis):
    """a at index + k along axis, the index clamped into the array"""
    n = a.shape[axis]
    idx = np.clip(np.arange(n) + k, 0, n - 1)
    return np.take(a, idx, axis=axis)


def _taps(a, coef, n, axis):
    """sum over k = -n..n of coef(k) * a(index + k), in that order"""
    acc = coef(-n) * _shift(a, -n, axis)
    for k in range(-n + 1, n + 1):
        acc = acc + coef(k) * _shift(a, k, axis)
    return acc


def polyexp(img, p):
    """S64: frame [H,W] float32 -> (b_x, b_y, a_xx, a_yy, a_xy) [5,H,W] float32"""
    img = np.ascontiguousarray(img, dtype=f32)
    n = p["poly_n"]
    g, xg, xxg, ig11, ig03, ig33, ig55 = poly_constants(p)
    cg = lambda k: g[abs(k)]
    cx = lambda k: -xg[-k] if k < 0 else xg[k]
    cxx = lambda k: xxg[abs(k)]
    m0, m1, m2 = _taps(img, cg, n, 0), _taps(img, cx, n, 0), _taps(img, cxx, n, 0)
    b1, b2, b4 = _taps(m0, cg, n, 1), _taps(m0, cx, n, 1), _taps(m0, cxx, n, 1)
    b3, b6 = _taps(m1, cg, n, 1), _taps(m1, cx, n, 1)
    b5 = _taps(m2, cg, n, 1)
    return np.stack([b2 * ig11, b3 * ig11, b1 * ig03 + b4 * ig33, b1 * ig03 + b5 * ig33, b6 * ig55]).astype(f32)


def _border(n):
    """S65's weight of every coordinate of an axis of n"""
    lo = np.ones(n, dtype=f32)
    hi = np.ones(n, dtype=f32)
    for i in range(5):
        lo[i] = f32(BORDER[i])
        hi[n - 1 - i] = f32(BORDER[i])
    return lo * hi


def matrices(r0, r1, u, v):
    """S65: coefficients [5,H,W] of both frames, flow -> (g11, g12, g22, h1, h2)"""
    h, w = u.shape
    one, half, quarter = f32(1), f32(0.5), f32(0.25)
    with np.errstate(all="ignore"):
        px = np.arange(w, dtype=f32)[None, :] + u
        py = np.arange(h, dtype=f32)[:, None] + v
        inside = (px >= f32(0)) & (px <= f32(w - 1)) & (py >= f32(0)) & (py <= f32(h - 1))
        x1f, y1f = np.minimum(np.floor(px), f32(w - 2)), np.minimum(np.floor(py), f32(h - 2))
        x1 = np.where(inside, x1f, f32(0)).astype(np.int64)
        y1 = np.where(inside, y1f, f32(0)).astype(np.int64)
        fx, fy = px - x1f, py - y1f
        a00, a01, a10, a11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
        c = [((a00 * r[y1, x1] + a01 * r[y1, x1 + 1]) + a10 * r[y1 + 1, x1]) + a11 * r[y1 + 1, x1 + 1] for r in r1]
        zero = np.zeros_like(u)
        bx1, by1 = np.where(inside, c[0], zero), np.where(inside, c[1], zero)
        axx = np.where(inside, (r0[2] + c[2]) * half, r0[2])
        ayy = np.where(inside, (r0[3] + c[3]) * half, r0[3])
        axy = np.where(inside, (r0[4] + c[4]) * quarter, r0[4] * half)
        dbx, dby = (r0[0] - bx1) * half, (r0[1] - by1) * half
        dbx = dbx + (axx * u + axy * v)
        dby = dby + (axy * u + ayy * v)
        s = _border(w)[None, :] * _border(h)[:, None]
        dbx, dby, axx, ayy, axy = dbx * s, dby * s, axx * s, ayy * s, axy * s
        return (axx * axx + axy * axy, (axx + ayy) * axy, ayy * ayy + axy * axy, axx * dbx + axy * dby, axy * dbx + ayy * dby)


def one_pass(r0, r1, u, v, p):
    """S65-S67: exactly one pass -> (u, v)"""
    m = p["winsize"] // 2
    kw = window_taps(p)
    ck = lambda i: kw[abs(i)]
    with np.errstate(all="ignore"):
        g11, g12, g22, h1, h2 = (_taps(_taps(e, ck, m, 0), ck, m, 1) for e in matrices(r0, r1, u, v))
        idet = f32(1) / ((g11 * g22 - g12 * g12) + f32(DET_REG))
        return (g22 * h1 - g12 * h2) * idet, (g11 * h2 - g12 * h1) * idet


def pyramid(img, p):
    """S63 + S1: the levels of one frame (gray values as they are), finest first"""
    img = np.ascontiguousarray(img, dtype=f32)
    h, w = img.shape
    sizes = tvl1_oracle.pyramid_sizes(w, h, p["levels"], p["pyr_scale"])
    levels = [img]
    for (lw, lh) in sizes[1:]:
        levels.append(tvl1_oracle.zoom_out(levels[-1], p["pyr_scale"]))
        assert levels[-1].shape == (lh, lw)
    return levels


def flow_pair(i0, i1, p):
    """two gray frames [H,W] in [0,255] -> flow [2,H,W] float32"""
    p0, p1 = pyramid(i0, p), pyramid(i1, p)
    u = np.zeros_like(p0[-1])
    v = np.zeros_like(p0[-1])
    for s in range(len(p0) - 1, -1, -1):
        r0, r1 = polyexp(p0[s], p), polyexp(p1[s], p)
        for _ in range(p["iterations"]):
            u, v = one_pass(r0, r1, u, v, p)
        if s > 0:
            fh, fw = p0[s - 1].shape
            u, v = brox_oracle.upsample(u, fw, fh, p["pyr_scale"]), brox_oracle.upsample(v, fw, fh, p["pyr_scale"])
    return np.stack([u, v])


def farneback_flow(frames, p=None):
    """frames uint8/float32 [S,F,H,W] (or [F,H,W]) -> flow float32 [S*(F-1),2,H,W], ``flow.farneback_flow``'s layout"""
    p = p if p is not None else params()
    fr = np.asarray(frames)
    if fr.ndim == 3:
        fr = fr[None]
    S, F = fr.shape[:2]
    return np.stack([flow_pair(fr[s, k], fr[s, k + 1], p) for s in range(S) for k in range(F - 1)]).astype(f32)
