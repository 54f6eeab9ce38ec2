"""An independent float64 restatement of Farneback optical flow -- TEST INFRASTRUCTURE.

Written from the publication (G. Farneback, SCIA 2003, sections 2-4), not from the float32 oracle: the polynomial expansion is
a weighted least-squares fit per pixel (``numpy.linalg.lstsq`` on the explicit basis 1, x, y, x^2, y^2, xy under the Gaussian
applicability) where the oracle and the kernel use the separable closed form; the matrices are 2x2 arrays per pixel
(``A^T A`` and ``A^T db`` by matrix products); the window sum is a dense 2-D sum; the 2x2 solve goes through
``numpy.linalg.solve``.  Nothing is rounded to float32: the taps are the continuous Gaussians.  Pyramid and upsampling are
the float64 forms of S1 and S8 in tests/brox_witness_f64.py.
"""
import numpy as np

import brox_witness_f64 as bw
from oracle import tvl1_oracle

BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)
DET_REG = 1e-3


def _basis(n, sigma):
    """-> (B [(2n+1)^2, 6] over the window in raster order, w [(2n+1)^2]: the applicability)"""
    dy, dx = np.mgrid[-n:n + 1, -n:n + 1].astype(np.float64)
    dx, dy = dx.ravel(), dy.ravel()
    w = np.exp(-(dx * dx + dy * dy) / (2.0 * sigma * sigma))
    return np.stack([np.ones_like(dx), dx, dy, dx * dx, dy * dy, dx * dy], axis=1), w


def polyexp(img, p):
    """frame [H,W] -> (b_x, b_y, a_xx, a_yy, a_xy) [5,H,W]: argmin over c of sum_w w (f - B c)^2 around every pixel, the
    frame continued by its border pixels"""
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape
    n = p["poly_n"]
    B, wt = _basis(n, float(np.float32(p["poly_sigma"])))
    pad = np.pad(img, n, mode="edge")
    patches = np.stack([pad[y:y + h, x:x + w].ravel() for y in range(2 * n + 1) for x in range(2 * n + 1)])  # [(2n+1)^2, H W]
    sw = np.sqrt(wt)[:, None]
    c = np.linalg.lstsq(sw * B, sw * patches, rcond=None)[0]  # [6, H W]
    return c[1:].reshape(5, h, w)


def _border(n):
    s = np.ones(n)
    for i, b in enumerate(BORDER):
        s[i] *= b
        s[n - 1 - i] *= b
    return s


def matrices(r0, r1, u, v):
    """-> G [H,W,2,2] = A^T A and hv [H,W,2] = A^T db of every pixel (section 4 of the publication, eq. 9-11 with the
    a-priori displacement (u, v)), with S65's rule outside the frame and its border weights"""
    h, w = u.shape
    px, py = np.arange(w)[None, :] + u, np.arange(h)[:, None] + v
    inside = (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)
    c = np.stack([bw.sample(r, np.where(inside, px, 0.0), np.where(inside, py, 0.0)) for r in r1])

    def quad(r):  # the symmetric matrix of the quadratic part
        return np.stack([np.stack([r[2], 0.5 * r[4]], -1), np.stack([0.5 * r[4], r[3]], -1)], -2)

    A0, A1 = quad(r0), quad(c)
    A = np.where(inside[..., None, None], 0.5 * (A0 + A1), A0)
    b0 = np.stack([r0[0], r0[1]], -1)
    b1 = np.where(inside[..., None], np.stack([c[0], c[1]], -1), 0.0)
    d = np.stack([u, v], -1)
    db = 0.5 * (b0 - b1) + np.einsum("...ij,...j->...i", A, d)
    s = _border(h)[:, None] * _border(w)[None, :]
    A, db = A * s[..., None, None], db * s[..., None]
    At = np.swapaxes(A, -1, -2)
    return At @ A, np.einsum("...ij,...j->...i", At, db)


def window(p):
    m = p["winsize"] // 2
    if not p["gaussian"]:
        k = np.full(2 * m + 1, 1.0 / p["winsize"])
    else:
        i = np.arange(-m, m + 1, dtype=np.float64)
        k = np.exp(-i * i / (2.0 * (0.3 * m) ** 2))
        k = k / k.sum()
    return np.outer(k, k)


def window_sum(a, K):
    """a [H,W,...]: dense 2-D sum under K, indices clamped"""
    m = K.shape[0] // 2
    h, w = a.shape[:2]
    pad = np.pad(a, [(m, m), (m, m)] + [(0, 0)] * (a.ndim - 2), mode="edge")
    out = np.zeros_like(a)
    for i in range(2 * m + 1):
        for j in range(2 * m + 1):
            out = out + K[i, j] * pad[i:i + h, j:j + w]
    return out


def one_pass(r0, r1, u, v, p):
    G, hv = matrices(r0, r1, u, v)
    K = window(p)
    G, hv = window_sum(G, K), window_sum(hv, K)
    det = np.linalg.det(G)
    # (G + reg)^-1 in S67's sense: the adjugate over det + reg, that is G^-1 h scaled by det / (det + reg)
    d = np.linalg.solve(G, hv[..., None])[..., 0] * (det / (det + DET_REG))[..., None]
    return d[..., 0], d[..., 1]


def flow_pair(i0, i1, p):
    """two gray frames [H,W] in [0,255] -> flow [2,H,W] float64"""
    h, w = np.asarray(i0).shape
    sizes = tvl1_oracle.pyramid_sizes(w, h, p["levels"], p["pyr_scale"])
    pyr = []
    for img in (i0, i1):
        lv = [np.asarray(img, dtype=np.float64)]
        for (lw, lh) in sizes[1:]:
            lv.append(bw.zoom_out(lv[-1], p["pyr_scale"], lw, lh))
        pyr.append(lv)
    u = np.zeros(pyr[0][-1].shape)
    v = np.zeros_like(u)
    for s in range(len(sizes) - 1, -1, -1):
        r0, r1 = polyexp(pyr[0][s], p), polyexp(pyr[1][s], p)
        for _ in range(p["iterations"]):
            u, v = one_pass(r0, r1, u, v, p)
        if s > 0:
            fw, fh = sizes[s - 1]
            u, v = bw.upsample(u, fw, fh, p["pyr_scale"]), bw.upsample(v, fw, fh, p["pyr_scale"])
    return np.stack([u, v])
