"""The executable form of DESIGN.md S69-S76 (dense trajectories) -- TEST INFRASTRUCTURE, never imported by the product.

numpy float32 and integers, one function per stage, every expression in the operation order the specification writes (no
fused multiply-add: numpy has none; no library arctangent: S70's polynomial, with the literals of DESIGN.md).  IEEE binary32
addition, multiplication, division and square root are correctly rounded in numpy as they are on the device, and everything
behind the quantisation of S71 is integer arithmetic, so the library has to reproduce these arrays bit for bit whatever its
tile shape, chunk length or reduction order.  S76's tests and norms are float64 in the written order (Python floats).
"""
import math

import numpy as np

f32 = np.float32

DEFAULTS = dict(step=5, length=15, patch=32, nxy=2, nt=3, quality=0.001, min_flow=0.4, min_std=1.7320508, max_std=30.0, max_dis=20.0,
                max_dis_share=0.7)
PLANES = 33
GROUPS = (("hog", 0, 8), ("hof", 8, 9), ("mbhx", 17, 8), ("mbhy", 25, 8))  # name, first plane, bins
HOG_VMAX, HOG_SHIFT = 2048.0, 8
FLOW_VMAX, FLOW_SHIFT = 32.0, 14
# S70: p(s) ~ atan(s) 4 / pi on [0,1]
ATAN = tuple(f32(c) for c in (1.2732345, -0.4242086, 0.25219768, -0.16850284, 0.10143076, -0.042850755, 0.0086996285))
REJECTED = ("left_frame", "static", "erratic", "jump", "unfinished")
ALIVE, LEFT, DONE = 0, 1, 2


def params(**over):
    p = dict(DEFAULTS)
    for k in over:
        if k not in p:
            raise ValueError("unknown dense-trajectory parameter %r" % k)
    p.update(over)
    return p


def descriptor_length(p):
    return 2 * p["length"] + PLANES * p["nt"] * p["nxy"] * p["nxy"]


def sobel(field):
    """S69 -> (gx, gy), float32 [h][w], replicated border"""
    a = np.pad(np.asarray(field, dtype=f32), 1, mode="edge")
    tl, tc, tr = a[:-2, :-2], a[:-2, 1:-1], a[:-2, 2:]
    l, r = a[1:-1, :-2], a[1:-1, 2:]
    bl, bc, br = a[2:, :-2], a[2:, 1:-1], a[2:, 2:]
    gx = ((tr - tl) + f32(2) * (r - l)) + (br - bl)
    gy = ((bl - tl) + f32(2) * (bc - tc)) + (br - tr)
    return gx, gy


def orient(x, y):
    """S70 -> (m, a): magnitude and bin coordinate in [0,8], float32"""
    x, y = np.asarray(x, dtype=f32), np.asarray(y, dtype=f32)
    with np.errstate(all="ignore"):
        m = np.sqrt(x * x + y * y)
        ax, ay = np.abs(x), np.abs(y)
        lo, hi = np.fmin(ax, ay), np.fmax(ax, ay)
        s = lo / np.where(hi > 0, hi, f32(1))
        s2 = s * s
        p = np.full_like(s, ATAN[6])
        for c in ATAN[5::-1]:
            p = p * s2 + c
        p = p * s
        p = np.where(ay > ax, f32(2) - p, p)
        p = np.where(x < 0, f32(4) - p, p)
        p = np.where(y < 0, f32(8) - p, p)
    return m, p.astype(f32)


def group_votes(x, y, vmax, shift):
    """S70-S71 -> (m, b0, q0, q1): the magnitude, the first bin and the two quantised votes (0 where m is not finite)"""
    m, a = orient(x, y)
    ok = np.isfinite(m)
    a, mm = np.where(ok, a, f32(0)), np.where(ok, m, f32(0))
    fl = np.floor(a)
    f = a - fl
    b0 = fl.astype(np.int64) & 7
    scale = f32(2.0 ** shift)
    q0 = np.rint(np.minimum(mm * (f32(1) - f), f32(vmax)) * scale).astype(np.uint32)
    q1 = np.rint(np.minimum(mm * f, f32(vmax)) * scale).astype(np.uint32)
    return m, b0, q0, q1


def _planes(b0, q0, q1):
    out = np.zeros((8,) + b0.shape, dtype=np.uint32)
    np.put_along_axis(out, b0[None], q0[None], 0)
    np.put_along_axis(out, ((b0 + 1) & 7)[None], q1[None], 0)
    return out


def votes(gray, u, v, p):
    """S69-S71: gray, u, v [h][w] -> uint32 [33][h][w]"""
    gray, u, v = (np.asarray(a).astype(f32) for a in (gray, u, v))
    out = np.zeros((PLANES,) + gray.shape, dtype=np.uint32)
    _, b0, q0, q1 = group_votes(*sobel(gray), HOG_VMAX, HOG_SHIFT)
    out[0:8] = _planes(b0, q0, q1)
    m, b0, q0, q1 = group_votes(u, v, FLOW_VMAX, FLOW_SHIFT)
    with np.errstate(invalid="ignore"):
        still = m <= f32(p["min_flow"])
    out[8:16] = _planes(b0, np.where(still, 0, q0).astype(np.uint32), np.where(still, 0, q1).astype(np.uint32))
    out[16] = np.where(still, 1 << FLOW_SHIFT, 0).astype(np.uint32)
    with np.errstate(all="ignore"):
        _, b0, q0, q1 = group_votes(*sobel(u), FLOW_VMAX, FLOW_SHIFT)
        out[17:25] = _planes(b0, q0, q1)
        _, b0, q0, q1 = group_votes(*sobel(v), FLOW_VMAX, FLOW_SHIFT)
        out[25:33] = _planes(b0, q0, q1)
    return out


def integral(q):
    """S72: uint32 [planes][h][w] -> uint32 [planes][h+1][w+1], sums mod 2^32"""
    q = np.asarray(q, dtype=np.uint32)
    out = np.zeros((q.shape[0], q.shape[1] + 1, q.shape[2] + 1), dtype=np.uint64)
    out[:, 1:, 1:] = np.cumsum(np.cumsum(q.astype(np.uint64), axis=1), axis=2)
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def cell_sum(I, xa, xb, ya, yb):
    """S72: the four-corner sums of all planes over [xa,xb) x [ya,yb), mod 2^32 (uint32 [planes]); 0 for an empty cell"""
    if xb <= xa or yb <= ya:
        return np.zeros(I.shape[0], dtype=np.uint32)
    with np.errstate(over="ignore"):
        return ((I[:, yb, xb] - I[:, ya, xb]) - I[:, yb, xa]) + I[:, ya, xa]


def direct_cell_sum(q, xa, xb, ya, yb):
    """the same sums straight from the votes, as Python integers"""
    return [int(q[c, ya:yb, xa:xb].astype(np.uint64).sum()) if xb > xa and yb > ya else 0 for c in range(q.shape[0])]


def corner(gray):
    """S73 -> (response float32 [h][w], the bit pattern of its maximum)"""
    gx, gy = sobel(gray)
    prods = [np.pad(a, 1, mode="edge") for a in (gx * gx, gx * gy, gy * gy)]
    h, w = gx.shape
    sums = []
    for a in prods:
        s = a[0:h, 0:w]
        for k in range(1, 9):
            s = s + a[k // 3:k // 3 + h, k % 3:k % 3 + w]
        sums.append(s)
    sa, sb, sc = sums
    d = sa - sc
    r = np.sqrt(d * d + f32(4) * (sb * sb))
    lam = ((sa + sc) - r) * f32(0.5)
    lam = np.where(lam > 0, lam, f32(0)).astype(f32)
    return lam, int(lam.max().view(np.uint32))


def nearest(v, n):
    """S74: nearest pixel of a float32 coordinate, inside [0, n-1]"""
    return min(max(int(math.floor(float(f32(v) + f32(0.5)))), 0), n - 1)


def new_track(start, x, y, p):
    return dict(start=start, pts=[(f32(x), f32(y))], acc=np.zeros((p["nt"], p["nxy"] * p["nxy"], PLANES), dtype=np.uint64))


def sample(tracks, resp, maxbits, frame, p):
    """S74: appends the tracks that start at `frame` behind the live ones, in raster order of the cells"""
    h, w = resp.shape
    step = p["step"]
    ncx, ncy = w // step, h // step
    occ = np.zeros((ncy, ncx), dtype=bool)
    for t in tracks:
        x, y = t["pts"][-1]
        cx, cy = nearest(x, w) // step, nearest(y, h) // step
        if cx < ncx and cy < ncy:
            occ[cy, cx] = True
    tq = f32(p["quality"]) * np.array([maxbits], dtype=np.uint32).view(f32)[0]
    for cy in range(ncy):
        for cx in range(ncx):
            px, py = cx * step + step // 2, cy * step + step // 2
            if not occ[cy, cx] and resp[py, px] > tq:
                tracks.append(new_track(frame, px, py, p))
    return tracks


def step(tracks, I, med, frame, p):
    """S75: every live track adds its slice and moves -> the list of statuses"""
    h, w = med.shape[1:]
    L, nxy, cs = p["length"], p["nxy"], p["patch"] // p["nxy"]
    tlen = L // p["nt"]
    stat = []
    for t in tracks:
        k = frame - t["start"]
        px, py = t["pts"][k]
        rx, ry = nearest(px, w), nearest(py, h)
        x0, y0 = rx - p["patch"] // 2, ry - p["patch"] // 2
        for cy in range(nxy):
            for cx in range(nxy):
                xa, xb = min(max(x0 + cx * cs, 0), w), min(max(x0 + (cx + 1) * cs, 0), w)
                ya, yb = min(max(y0 + cy * cs, 0), h), min(max(y0 + (cy + 1) * cs, 0), h)
                t["acc"][k // tlen, cy * nxy + cx] += cell_sum(I, xa, xb, ya, yb).astype(np.uint64)
        with np.errstate(all="ignore"):
            nx, ny = f32(px) + f32(med[0, ry, rx]), f32(py) + f32(med[1, ry, rx])
        inside = bool(nx >= f32(0) and nx <= f32(w - 1) and ny >= f32(0) and ny <= f32(h - 1))
        if inside:
            t["pts"].append((nx, ny))
            stat.append(DONE if k + 1 == L else ALIVE)
        else:
            stat.append(LEFT)
    return stat


def classify(pts, p):
    """S76's tests, float64 in the written order -> (0 valid / 1 static / 2 erratic / 3 jump, the total length)"""
    n = len(pts)
    sx = sy = 0.0
    for x, y in pts:
        sx, sy = sx + float(x), sy + float(y)
    mx, my = sx / float(n), sy / float(n)
    vx = vy = 0.0
    for x, y in pts:
        dx, dy = float(x) - mx, float(y) - my
        vx, vy = vx + dx * dx, vy + dy * dy
    sdx, sdy = math.sqrt(vx / float(n)), math.sqrt(vy / float(n))
    total = longest = 0.0
    for k in range(n - 1):
        dx, dy = float(pts[k + 1][0]) - float(pts[k][0]), float(pts[k + 1][1]) - float(pts[k][1])
        seg = math.sqrt(dx * dx + dy * dy)
        total = total + seg
        longest = seg if seg > longest else longest
    lim = {k: float(f32(p[k])) for k in ("min_std", "max_std", "max_dis", "max_dis_share")}
    if sdx < lim["min_std"] and sdy < lim["min_std"]:
        return 1, total
    if sdx > lim["max_std"] or sdy > lim["max_std"]:
        return 2, total
    if longest > lim["max_dis"]:
        return 3, total
    if longest > lim["max_dis_share"] * total:
        return 3, total
    return 0, total


def descriptor(t, total, p):
    """S76: shape | HOG | HOF | MBHx | MBHy, float32"""
    pts = t["pts"]
    out = []
    for k in range(len(pts) - 1):
        for c in (0, 1):
            out.append(f32((float(pts[k + 1][c]) - float(pts[k][c])) / total))
    acc = t["acc"].reshape(-1, PLANES)
    for _, p0, nb in GROUPS:
        unit = 2.0 ** -(HOG_SHIFT if p0 == 0 else FLOW_SHIFT)
        vals = [float(int(a)) * unit for a in acc[:, p0:p0 + nb].reshape(-1)]
        ss = 0.0
        for v in vals:
            ss = ss + v * v
        norm = math.sqrt(ss)
        out.extend(f32(v / norm) if norm > 0.0 else f32(0) for v in vals)
    return np.array(out, dtype=f32)


def finish(tracks, stat, p, found, rejected, dropped=None):
    """S76: -> the surviving tracks; valid finished ones are appended to `found` (desc, points, start), the others counted
    (and appended to `dropped` as (track, index into REJECTED) when a list is given)"""
    alive = []
    for t, s in zip(tracks, stat):
        if s == ALIVE:
            alive.append(t)
        elif s == LEFT:
            rejected[0] += 1
            if dropped is not None:
                dropped.append((t, 0))
        else:
            code, total = classify(t["pts"], p)
            if code:
                rejected[code] += 1
                if dropped is not None:
                    dropped.append((t, code))
            else:
                found.append((descriptor(t, total, p), np.array(t["pts"], dtype=f32), t["start"]))
    return alive


def median3(flow):
    """S55 with k = 3 on [n][2][h][w]: edge replication, the fifth smallest of the nine samples"""
    flow = np.asarray(flow, dtype=f32)
    h, w = flow.shape[-2:]
    a = np.pad(flow, [(0, 0)] * (flow.ndim - 2) + [(1, 1), (1, 1)], mode="edge")
    win = np.stack([a[..., dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    return np.sort(win, axis=0)[4]


def extract(gray, flow, med, p, dropped=None):
    """S69-S76 end to end: gray [T][h][w], flow and median-filtered flow [T-1][2][h][w] -> dict like dense_trajectories', and the frames
    at which tracks started"""
    T = gray.shape[0]
    L = p["length"]
    tracks, found, rejected, started = [], [], [0, 0, 0, 0, 0], set()
    for t in range(T - 1):
        if t <= T - 1 - L:
            n0 = len(tracks)
            resp, mb = corner(gray[t])
            sample(tracks, resp, mb, t, p)
            if len(tracks) > n0:
                started.add(t)
        I = integral(votes(gray[t], flow[t, 0], flow[t, 1], p))
        stat = step(tracks, I, med[t], t, p)
        tracks = finish(tracks, stat, p, found, rejected, dropped)
    rejected[4] = len(tracks)
    dim = descriptor_length(p)
    return dict(desc=np.stack([f[0] for f in found]) if found else np.zeros((0, dim), dtype=f32),
                points=np.stack([f[1] for f in found]) if found else np.zeros((0, L + 1, 2), dtype=f32),
                start=np.array([f[2] for f in found], dtype=np.int32), rejected=dict(zip(REJECTED, rejected)), count=len(found),
                started_frames=sorted(started))
