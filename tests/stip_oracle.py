"""The executable form of DESIGN.md S83-S90 (space-time interest points) -- TEST INFRASTRUCTURE, never imported by the product.

numpy float32 and integers, one function per stage, every expression in the operation order the specification writes:
elementwise operations and Python tap loops only (no ``sum``, ``dot`` or ``convolve`` on the result path, no fused
multiply-add: numpy has none; no library arctangent: S70's polynomial from ``dtraj_oracle``).  IEEE binary32 addition and
multiplication are correctly rounded in numpy as they are on the device, and everything behind the quantisation of S88 is
integer arithmetic, so the library has to reproduce these arrays bit for bit whatever its tile shapes.  S83's taps, S89's
cell edges and norms are float64 in the written order (Python floats).
"""
import math

import numpy as np

import dtraj_oracle as do

f32 = np.float32

DEFAULTS = dict(sigmas=tuple(float(f32(2.0 ** ((1 + i) / 2.0))) for i in range(1, 7)),
                taus=tuple(float(f32(2.0 ** (j / 2.0))) for j in (1, 2)),
                integration=2.0, k=0.005, min_response=0.0, cuboid=9.0, neighbours=6, nx=3, ny=3, nt=2, bins=4)
MAX_RADIUS = 512
HOG_VMAX, HOG_SHIFT = 512.0, 8
FLOW_VMAX, FLOW_SHIFT = 32.0, 12
MAX_SLICE = 32767  # pixels of a cell's slice of one frame: MAX_SLICE * VMAX * 2^SHIFT < 2^32 for both groups


def params(**over):
    p = dict(DEFAULTS)
    for k in over:
        if k not in p:
            raise ValueError("unknown space-time interest point parameter %r" % k)
    p.update(over)
    # the scales are float32 values, as the C structure holds them
    p["sigmas"] = tuple(float(f32(s)) for s in p["sigmas"])
    p["taus"] = tuple(float(f32(s)) for s in p["taus"])
    for name in ("integration", "k", "min_response", "cuboid"):
        p[name] = float(f32(p[name]))
    return p


def descriptor_length(p):
    return 2 * p["nx"] * p["ny"] * p["nt"] * p["bins"]


# ---------------------------------------------------------------- S83

def taps(sigma):
    """-> (r, g float32 [r+1]): r = int(4 sigma + 0.5); g[k] = exp(-k^2 / (2 sigma^2)) / S in float64, S added outwards"""
    sigma = float(sigma)
    r = int(4.0 * sigma + 0.5)
    d = 2.0 * sigma * sigma
    w = [math.exp(-(float(k) * float(k)) / d) for k in range(r + 1)]
    s = w[0]
    for k in range(1, r + 1):
        s = s + (w[k] + w[k])
    return r, np.array([f32(w[k] / s) for k in range(r + 1)], dtype=f32)


def fold(i, n):
    """scipy's ``reflect`` (d c b a | a b c d | d c b a) for any integer i (array or scalar): period 2n"""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


# ---------------------------------------------------------------- S84

def smooth_axis(a, g, axis):
    """acc = g0 c, then for k = 1..r: acc = acc + g[k] (a[-k] + a[+k]), float32"""
    a = np.asarray(a, dtype=f32)
    n = a.shape[axis]
    idx = np.arange(n)
    acc = g[0] * a
    for k in range(1, len(g)):
        acc = acc + g[k] * (np.take(a, fold(idx - k, n), axis=axis) + np.take(a, fold(idx + k, n), axis=axis))
    return acc


def smooth(f, sigma, tau):
    """f [T][h][w] (any dtype, converted to float32 exactly) -> L float32: along x, then y (sigma), then t (tau)"""
    a = np.asarray(f).astype(f32)
    _, gs = taps(sigma)
    _, gt = taps(tau)
    with np.errstate(all="ignore"):
        return smooth_axis(smooth_axis(smooth_axis(a, gs, 2), gs, 1), gt, 0)


# ---------------------------------------------------------------- S85

def gradient_axis(a, axis):
    """np.gradient's rule, float32: (a[i+1] - a[i-1]) 0.5 inside, one-sided at both ends, 0 on an axis of length 1"""
    a = np.asarray(a, dtype=f32)
    n = a.shape[axis]
    out = np.zeros_like(a)
    if n < 2:
        return out
    a = np.moveaxis(a, axis, 0)
    o = np.moveaxis(out, axis, 0)
    with np.errstate(all="ignore"):
        o[0] = a[1] - a[0]
        o[n - 1] = a[n - 1] - a[n - 2]
        if n > 2:
            o[1:n - 1] = (a[2:] - a[:n - 2]) * f32(0.5)
    return out


def gradient_products(L):
    """-> float32 [6][T][h][w]: LxLx, LyLy, LtLt, LxLy, LxLt, LyLt"""
    lx, ly, lt = gradient_axis(L, 2), gradient_axis(L, 1), gradient_axis(L, 0)
    with np.errstate(all="ignore"):
        return np.stack([lx * lx, ly * ly, lt * lt, lx * ly, lx * lt, ly * lt])


# ---------------------------------------------------------------- S86

def response(S, k):
    xx, yy, tt, xy, xt, yt = (np.asarray(s, dtype=f32) for s in S)
    k = f32(k)
    with np.errstate(all="ignore"):
        a = yy * tt - yt * yt
        b = xy * tt - yt * xt
        c = xy * yt - yy * xt
        det = (xx * a - xy * b) + xt * c
        tr = (xx + yy) + tt
        return det - k * ((tr * tr) * tr)


def harris(f, sigma, tau, p):
    """S84-S86 for one scale pair -> (L, the six smoothed products, H)"""
    L = smooth(f, sigma, tau)
    s = p["integration"]
    S = np.stack([smooth(c, s * sigma, s * tau) for c in gradient_products(L)])
    return L, S, response(S, p["k"])


# ---------------------------------------------------------------- S87

NEIGHBOURS = {6: [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)],
              26: [(dt, dy, dx) for dt in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dt, dy, dx) != (0, 0, 0)]}


def maxima(H, min_response, neighbours):
    """-> int32 [n][3] (x, y, t) in t, y, x order: finite, > min_response, strictly greater than every neighbour, off the faces"""
    H = np.asarray(H, dtype=f32)
    T, h, w = H.shape
    if T < 3 or h < 3 or w < 3:
        return np.zeros((0, 3), dtype=np.int32)
    c = H[1:-1, 1:-1, 1:-1]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(c) & (c > f32(min_response))
        for dt, dy, dx in NEIGHBOURS[neighbours]:
            ok &= c > H[1 + dt:T - 1 + dt, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    t, y, x = np.nonzero(ok)  # C order: t, then y, then x
    return np.stack([x + 1, y + 1, t + 1], axis=1).astype(np.int32)


# ---------------------------------------------------------------- S88

def group_votes(x, y, vmax, shift, bins):
    """S70-S71 with `bins` circular bins -> uint32 [bins] + x.shape"""
    m, a = do.orient(x, y)
    ok = np.isfinite(m)
    a, mm = np.where(ok, a, f32(0)), np.where(ok, m, f32(0))
    if bins != 8:
        a = a * f32(bins * 0.125)
    fl = np.floor(a)
    f = a - fl
    b0 = fl.astype(np.int64) % bins
    scale = f32(2.0 ** shift)
    q0 = np.rint(np.minimum(mm * (f32(1) - f), f32(vmax)) * scale).astype(np.uint32)
    q1 = np.rint(np.minimum(mm * f, f32(vmax)) * scale).astype(np.uint32)
    out = np.zeros((bins,) + b0.shape, dtype=np.uint32)
    np.put_along_axis(out, b0[None], q0[None], 0)
    np.put_along_axis(out, ((b0 + 1) % bins)[None], q1[None], 0)
    return out


def votes_hog(L, bins):
    """-> uint32 [T][bins][h][w] from (Lx, Ly)"""
    with np.errstate(all="ignore"):
        return np.moveaxis(group_votes(gradient_axis(L, 2), gradient_axis(L, 1), HOG_VMAX, HOG_SHIFT, bins), 0, 1)


def votes_hof(flow, bins):
    """flow [T-1][2][h][w] -> uint32 [T][bins][h][w]: the field of the last pair stands in for the last frame"""
    flow = np.asarray(flow, dtype=f32)
    fl = np.concatenate([flow, flow[-1:]], axis=0)
    with np.errstate(all="ignore"):
        return np.moveaxis(group_votes(fl[:, 0], fl[:, 1], FLOW_VMAX, FLOW_SHIFT, bins), 0, 1)


def integral(votes):
    """uint32 [T][bins][h][w] -> [T][bins][h+1][w+1] (S72)"""
    T, b, h, w = votes.shape
    return do.integral(votes.reshape(T * b, h, w)).reshape(T, b, h + 1, w + 1)


# ---------------------------------------------------------------- S89

def cell_edges(c, delta, n, size):
    """clamp(rint((c - delta/2) + (j delta)/n), 0, size), j = 0..n, float64 in this order"""
    out = []
    for j in range(n + 1):
        e = float(np.rint((float(c) - delta / 2.0) + (float(j) * delta) / float(n)))
        out.append(int(min(max(e, 0.0), float(size))))
    return out


def max_slice(p):
    """the largest cell slice the parameters admit: rounded edges lie at most delta / n + 1 apart"""
    side = 2.0 * p["cuboid"] * max(p["sigmas"])
    return (int(math.ceil(side / p["nx"])) + 1) * (int(math.ceil(side / p["ny"])) + 1)


def cuboid_sums(point, hogI, hofI, p):
    """-> Python ints [2 nx ny nt bins]: HOG then HOF, cells in (t, y, x) order"""
    x, y, t, si, ti = (int(v) for v in point)
    T, bins, h1, w1 = hogI.shape
    dxy, dt = (2.0 * p["cuboid"]) * p["sigmas"][si], (2.0 * p["cuboid"]) * p["taus"][ti]
    ex, ey, et = cell_edges(x, dxy, p["nx"], w1 - 1), cell_edges(y, dxy, p["ny"], h1 - 1), cell_edges(t, dt, p["nt"], T)
    out = []
    for I in (hogI, hofI):
        for ct in range(p["nt"]):
            for cy in range(p["ny"]):
                for cx in range(p["nx"]):
                    acc = [0] * bins
                    for f in range(et[ct], et[ct + 1]):
                        s = do.cell_sum(I[f], ex[cx], ex[cx + 1], ey[cy], ey[cy + 1])
                        for b in range(bins):
                            acc[b] += int(s[b])
                    out.extend(acc)
    return out


def descriptor(sums, p):
    """the integers -> float32 [dim]: value unit, divided by the float64 L2 norm added in index order; zero norm -> zeros"""
    half = len(sums) // 2
    v = [float(s) * (2.0 ** -HOG_SHIFT if i < half else 2.0 ** -FLOW_SHIFT) for i, s in enumerate(sums)]
    ss = 0.0
    for x in v:
        ss = ss + x * x
    norm = math.sqrt(ss)
    return np.array([f32(x / norm) if norm > 0.0 else f32(0) for x in v], dtype=f32)


def describe(points, hogI, hofI, p):
    if len(points) == 0:
        return np.zeros((0, descriptor_length(p)), dtype=f32)
    return np.stack([descriptor(cuboid_sums(q, hogI, hofI, p), p) for q in points])


# ---------------------------------------------------------------- the whole call

def extract(gray, flow, p, keep=None):
    """-> points int32 [n][5], response float32 [n], desc float32 [n][dim]; keep (a dict) receives L, S, H per scale pair"""
    gray = np.asarray(gray)
    bins = p["bins"]
    hofI = integral(votes_hof(flow, bins))
    pts, resp, desc = [], [], []
    for si, sigma in enumerate(p["sigmas"]):
        for ti, tau in enumerate(p["taus"]):
            L, S, H = harris(gray, sigma, tau, p)
            if keep is not None:
                keep[(si, ti)] = (L, S, H)
            m = maxima(H, p["min_response"], p["neighbours"])
            q = np.concatenate([m, np.full((len(m), 1), si, np.int32), np.full((len(m), 1), ti, np.int32)], axis=1).astype(np.int32)
            pts.append(q)
            resp.append(H[m[:, 2], m[:, 1], m[:, 0]].astype(f32))
            desc.append(describe(q, integral(votes_hog(L, bins)), hofI, p))
    return np.concatenate(pts), np.concatenate(resp), np.concatenate(desc)
