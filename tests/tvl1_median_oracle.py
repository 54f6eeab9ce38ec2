"""ctypes binding of tests/tvl1_median_oracle.c and the float64 witness with the filter -- TEST INFRASTRUCTURE ONLY.

The C file restates the level and the driver of oracle/tvl1_oracle.c with the median filter of DESIGN.md S55; it is built
here with exactly the flags of oracle/Makefile (read from it: ``-ffp-contract=off`` is part of the arithmetic contract)
into a shared object next to this file.  The float64 witness restates ``level`` of oracle/tvl1_ipol_f64.py with a filter
written in numpy alone (edge padding, ``sliding_window_view``, ``np.median``) and imports everything else from there.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from oracle import tvl1_oracle
from oracle.tvl1_ipol_f64 import (GRAD_IS_ZERO, bilinear, centred_gradient, divergence, forward_gradient, pyramid_sizes,
                                  zoom_out)

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "tvl1_median_oracle.c")
_SO = os.path.join(_HERE, "libva_median_oracle.so")
_ORACLE_DIR = os.path.dirname(os.path.abspath(tvl1_oracle.__file__))


def _makefile_flags():
    text = open(os.path.join(_ORACLE_DIR, "Makefile")).read()
    return re.search(r"^CFLAGS\s*=\s*(.*)$", text, re.M).group(1).split()


def build(force=False):
    newest = max(os.path.getmtime(_SRC), os.path.getmtime(os.path.join(_ORACLE_DIR, "tvl1_oracle.c")))
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < newest:
        tmp = "%s.%d.tmp" % (_SO, os.getpid())
        subprocess.check_call([os.environ.get("CC", "gcc")] + _makefile_flags() + ["-o", tmp, _SRC, "-lm"])
        os.replace(tmp, _SO)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        fp, ci = ctypes.POINTER(ctypes.c_float), ctypes.c_int
        L.ora_flow_median.argtypes = [fp, ci, ci, ci, ci, fp]
        L.ora_flow_median.restype = ci
        L.ora_tvl1_median_flow.argtypes = [fp, ci, ci, ci, ci, ctypes.POINTER(tvl1_oracle.OraTvl1Params), ci, ci, fp,
                                           ctypes.POINTER(ctypes.c_long), ci]
        L.ora_tvl1_median_flow.restype = ci
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def flow_median(flow, ksize):
    """flow float32 [N,2,H,W] -> its ksize x ksize median, plane by plane (the C filter)."""
    fl = np.ascontiguousarray(flow, dtype=np.float32)
    n, two, H, W = fl.shape
    assert two == 2
    out = np.empty_like(fl)
    if lib().ora_flow_median(_fp(fl), n, W, H, ksize, _fp(out)) != 0:
        raise ValueError("ora_flow_median: bad arguments")
    return out


def tvl1_flow(frames, params=None, median=0, median_every=0, nthreads=0, return_iters=False):
    """``oracle.tvl1_oracle.tvl1_flow`` with the two options of S55."""
    fr = np.asarray(frames)
    if fr.ndim == 3:
        fr = fr[None]
    fr = np.ascontiguousarray(fr, dtype=np.float32)
    S, F, H, W = fr.shape
    P = params if params is not None else tvl1_oracle.default_params()
    flow = np.empty((S * (F - 1), 2, H, W), dtype=np.float32)
    iters = (ctypes.c_long * (S * (F - 1)))()
    rc = lib().ora_tvl1_median_flow(_fp(fr), S, F, W, H, ctypes.byref(P), median, median_every, _fp(flow), iters, nthreads)
    if rc != 0:
        raise ValueError("ora_tvl1_median_flow: bad arguments")
    if return_iters:
        return flow, np.array(list(iters), dtype=np.int64)
    return flow


# ---------------------------------------------------------------- numpy filter and float64 witness

def median_np(plane, ksize):
    """k x k median of a 2-D array in its own dtype: edge padding, every window, numpy's median (odd count: a sample)."""
    r = ksize // 2
    pad = np.pad(plane, r, mode="edge")
    return np.median(sliding_window_view(pad, (ksize, ksize)), axis=(-2, -1)).astype(plane.dtype)


def flow_median_np(flow, ksize):
    flow = np.asarray(flow)
    return np.stack([np.stack([median_np(f[0], ksize), median_np(f[1], ksize)]) for f in flow])


def level_f64(I0, I1, I1x, I1y, u1, u2, tau, lam, theta, warps, iters, median, median_every):
    """``level`` of oracle/tvl1_ipol_f64.py (IPOL Algorithm 1, three-case TH) with the filter at the head of iteration it,
    it % median_every == 0."""
    h, w = I0.shape
    l_t = lam * theta
    taut = tau / theta
    every = median_every if median_every > 0 else iters
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    p11 = np.zeros((h, w)); p12 = np.zeros((h, w)); p21 = np.zeros((h, w)); p22 = np.zeros((h, w))
    for _ in range(warps):
        I1w = bilinear(I1, xx + u1, yy + u2)
        I1wx = bilinear(I1x, xx + u1, yy + u2)
        I1wy = bilinear(I1y, xx + u1, yy + u2)
        grad = I1wx * I1wx + I1wy * I1wy
        rho_c = I1w - I1wx * u1 - I1wy * u2 - I0
        safe = np.where(grad < GRAD_IS_ZERO, 1.0, grad)
        for it in range(iters):
            if median and it % every == 0:
                u1 = median_np(u1, median)
                u2 = median_np(u2, median)
            rho = rho_c + (I1wx * u1 + I1wy * u2)
            lo = rho < -l_t * grad
            hi = rho > l_t * grad
            mid = np.where(grad < GRAD_IS_ZERO, 0.0, -rho / safe)
            fi = np.where(lo, l_t, np.where(hi, -l_t, mid))
            v1 = u1 + fi * I1wx
            v2 = u2 + fi * I1wy
            u1 = v1 + theta * divergence(p11, p12)
            u2 = v2 + theta * divergence(p21, p22)
            u1x, u1y = forward_gradient(u1)
            u2x, u2y = forward_gradient(u2)
            g1 = 1.0 + taut * np.hypot(u1x, u1y)
            g2 = 1.0 + taut * np.hypot(u2x, u2y)
            p11 = (p11 + taut * u1x) / g1
            p12 = (p12 + taut * u1y) / g1
            p21 = (p21 + taut * u2x) / g2
            p22 = (p22 + taut * u2y) / g2
    return u1, u2


def tvl1_flow_pair_f64(f0, f1, median, median_every, tau=0.25, lam=0.15, theta=0.3, nscales=5, warps=5, iters=300, step=0.8):
    """``tvl1_flow_pair`` of oracle/tvl1_ipol_f64.py over ``level_f64``."""
    f0 = np.asarray(f0, dtype=np.float64)
    f1 = np.asarray(f1, dtype=np.float64)
    h, w = f0.shape
    sizes = pyramid_sizes(w, h, nscales, step)
    P0, P1 = [f0], [f1]
    for (lw, lh) in sizes[1:]:
        P0.append(zoom_out(P0[-1], lw, lh, step))
        P1.append(zoom_out(P1[-1], lw, lh, step))
    cw, ch = sizes[-1]
    u1 = np.zeros((ch, cw))
    u2 = np.zeros((ch, cw))
    for s in range(len(sizes) - 1, -1, -1):
        I1x, I1y = centred_gradient(P1[s])
        u1, u2 = level_f64(P0[s], P1[s], I1x, I1y, u1, u2, tau, lam, theta, warps, iters, median, median_every)
        if s > 0:
            fw, fh = sizes[s - 1]
            lw, lh = sizes[s]
            yy, xx = np.mgrid[0:fh, 0:fw].astype(np.float64)
            u1 = bilinear(u1, xx * (lw / fw), yy * (lh / fh)) / step
            u2 = bilinear(u2, xx * (lw / fw), yy * (lh / fh)) / step
    return u1, u2
