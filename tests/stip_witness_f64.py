"""An independent float64 statement of DESIGN.md S83-S90 -- TEST INFRASTRUCTURE, never imported by the product.

Built from library pieces the oracle does not use: ``scipy.ndimage.gaussian_filter(mode="reflect", truncate=4)``,
``np.gradient``, ``scipy.signal.argrelextrema``, a real ``arctan2`` and direct box sums without integral planes or fixed
point.  It shares no code with ``stip_oracle`` beyond the parameter dictionary.
"""
import numpy as np
from scipy import ndimage, signal


def harris(f, sigma, tau, p):
    """-> (L, the six smoothed products, H), float64 [T][h][w]"""
    f = np.asarray(f, dtype=np.float64)
    L = ndimage.gaussian_filter(f, (tau, sigma, sigma), mode="reflect", truncate=4.0)
    lt, ly, lx = (np.gradient(L, axis=a) if L.shape[a] > 1 else np.zeros_like(L) for a in (0, 1, 2))
    s = p["integration"]
    S = np.stack([ndimage.gaussian_filter(c, (s * tau, s * sigma, s * sigma), mode="reflect", truncate=4.0)
                  for c in (lx * lx, ly * ly, lt * lt, lx * ly, lx * lt, ly * lt)])
    xx, yy, tt, xy, xt, yt = S
    det = xx * (yy * tt - yt * yt) - xy * (xy * tt - yt * xt) + xt * (xy * yt - yy * xt)
    tr = xx + yy + tt
    return L, S, det - p["k"] * tr ** 3


def neighbour_margin(H, neighbours):
    """float64 [T][h][w]: H minus its largest compared neighbour; -inf on the faces"""
    T, h, w = H.shape
    out = np.full(H.shape, -np.inf)
    if T < 3 or h < 3 or w < 3:
        return out
    offs = [(dt, dy, dx) for dt in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dt, dy, dx) != (0, 0, 0) and (neighbours == 26 or abs(dt) + abs(dy) + abs(dx) == 1)]
    nb = np.stack([H[1 + dt:T - 1 + dt, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx] for dt, dy, dx in offs])
    out[1:-1, 1:-1, 1:-1] = H[1:-1, 1:-1, 1:-1] - nb.max(axis=0)
    return out


def maxima(H, min_response, neighbours):
    """-> int [n][3] (x, y, t) in t, y, x order.  6 neighbours: ``argrelextrema`` along each axis with its clipped
    comparison (a face compares with itself and fails); 26: the margin above must be positive as well."""
    ok = np.zeros(H.shape, dtype=bool)
    if min(H.shape) >= 1:
        ok[:] = H > min_response
        for axis in range(3):
            m = np.zeros(H.shape, dtype=bool)
            m[signal.argrelextrema(H, np.greater, axis=axis, mode="clip")] = True
            ok &= m
    if neighbours == 26:
        ok &= neighbour_margin(H, 26) > 0
    t, y, x = np.nonzero(ok)
    return np.stack([x, y, t], axis=1)


def votes(x, y, vmax, bins):
    """float64 [bins] + x.shape: the magnitude split linearly between the two nearest of `bins` circular bins, each share
    clamped to vmax; a non-finite magnitude votes 0"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        m = np.hypot(x, y)
        a = np.mod(np.arctan2(y, x), 2 * np.pi) * (bins / (2 * np.pi))
    ok = np.isfinite(m)
    m, a = np.where(ok, m, 0.0), np.where(ok, a, 0.0)
    b0 = np.floor(a)
    f = a - b0
    out = np.zeros((bins,) + x.shape)
    for b in range(bins):
        out[b] += np.where(b0.astype(int) % bins == b, np.minimum(m * (1 - f), vmax), 0.0)
        out[b] += np.where((b0.astype(int) + 1) % bins == b, np.minimum(m * f, vmax), 0.0)
    return out


def edges(c, delta, n, size):
    return [int(min(max(round(c - delta / 2 + j * delta / n), 0), size)) for j in range(n + 1)]


def describe(points, L_by_pair, flow, p, hog_vmax, flow_vmax):
    """points [n][5]; L_by_pair {(si, ti): L float64} -> float64 [n][2 nx ny nt bins]"""
    bins = p["bins"]
    flow = np.asarray(flow, dtype=np.float64)
    fl = np.concatenate([flow, flow[-1:]], axis=0)
    hof = votes(fl[:, 0], fl[:, 1], flow_vmax, bins)  # [bins][T][h][w]
    hog = {}
    out = []
    for x, y, t, si, ti in np.asarray(points).tolist():
        if (si, ti) not in hog:
            L = L_by_pair[(si, ti)]
            T, h, w = L.shape
            lx = np.gradient(L, axis=2) if w > 1 else np.zeros_like(L)
            ly = np.gradient(L, axis=1) if h > 1 else np.zeros_like(L)
            hog[(si, ti)] = votes(lx, ly, hog_vmax, bins)
        T, h, w = hof.shape[1:]
        dxy, dt = 2 * p["cuboid"] * p["sigmas"][si], 2 * p["cuboid"] * p["taus"][ti]
        ex, ey, et = edges(x, dxy, p["nx"], w), edges(y, dxy, p["ny"], h), edges(t, dt, p["nt"], T)
        d = []
        for v in (hog[(si, ti)], hof):
            for ct in range(p["nt"]):
                for cy in range(p["ny"]):
                    for cx in range(p["nx"]):
                        box = v[:, et[ct]:et[ct + 1], ey[cy]:ey[cy + 1], ex[cx]:ex[cx + 1]]
                        d.extend(box.reshape(bins, -1).sum(axis=1).tolist())
        d = np.array(d)
        n = np.sqrt((d * d).sum())
        out.append(d / n if n > 0 else np.zeros_like(d))
    return np.array(out).reshape(len(out), 2 * p["nx"] * p["ny"] * p["nt"] * bins)
