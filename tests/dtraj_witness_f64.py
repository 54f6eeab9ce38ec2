"""An independent float64 restatement of DESIGN.md S69-S76 (dense trajectories) -- TEST INFRASTRUCTURE.

It shares no code with tests/dtraj_oracle.py and takes none of its shortcuts: the angle is ``np.arctan2``, votes stay float64
(no fixed point), a cell's histogram is summed straight from the votes of its pixels (no integral planes), and tracking is a
plain loop over Python lists.  What the two must agree on, and how closely, is worked out in tests/test_dtraj_host.py.
"""
import math

import numpy as np

HOG_VMAX, FLOW_VMAX = 2048.0, 32.0
OFFSETS = (0, 8, 17, 25)  # first plane of HOG, HOF, MBHx, MBHy
BINS = (8, 9, 8, 8)


def gradients(a):
    a = np.pad(np.asarray(a, dtype=np.float64), 1, mode="edge")
    h, w = a.shape[0] - 2, a.shape[1] - 2
    gx, gy = np.zeros((h, w)), np.zeros((h, w))
    kx = ((-1.0, 0.0, 1.0), (-2.0, 0.0, 2.0), (-1.0, 0.0, 1.0))
    for dy in range(3):
        for dx in range(3):
            gx += kx[dy][dx] * a[dy:dy + h, dx:dx + w]
            gy += kx[dx][dy] * a[dy:dy + h, dx:dx + w]
    return gx, gy


def soft_bins(x, y, vmax):
    """float64 [8][h][w]: magnitude shared between the two bins around the angle, 45 degrees a bin"""
    m = np.hypot(x, y)
    a = np.mod(np.arctan2(y, x), 2.0 * math.pi) / (math.pi / 4.0)
    b0 = np.floor(a)
    f = a - b0
    out = np.zeros((8,) + m.shape)
    for b in range(8):
        out[b] += np.where(b0.astype(int) % 8 == b, np.minimum(m * (1.0 - f), vmax), 0.0)
        out[b] += np.where((b0.astype(int) + 1) % 8 == b, np.minimum(m * f, vmax), 0.0)
    return m, out


def votes(gray, u, v, min_flow):
    """float64 [33][h][w], unquantised"""
    gray, u, v = (np.asarray(a, dtype=np.float64) for a in (gray, u, v))
    out = np.zeros((33,) + gray.shape)
    out[0:8] = soft_bins(*gradients(gray), HOG_VMAX)[1]
    m, hof = soft_bins(u, v, FLOW_VMAX)
    still = m <= min_flow
    out[8:16] = np.where(still, 0.0, hof)
    out[16] = still
    out[17:25] = soft_bins(*gradients(u), FLOW_VMAX)[1]
    out[25:33] = soft_bins(*gradients(v), FLOW_VMAX)[1]
    return out


def flow_magnitude(u, v):
    return np.hypot(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64))


def tube_slice(vt, x, y, patch, nxy):
    """[nxy*nxy][33]: the histograms of the cells of the patch around pixel (x, y), each clipped to the frame"""
    h, w = vt.shape[1:]
    cs = patch // nxy
    out = []
    for cy in range(nxy):
        for cx in range(nxy):
            xa, ya = x - patch // 2 + cx * cs, y - patch // 2 + cy * cs
            xs = [i for i in range(xa, xa + cs) if 0 <= i < w]
            ys = [j for j in range(ya, ya + cs) if 0 <= j < h]
            out.append([sum(vt[c, j, i] for j in ys for i in xs) for c in range(33)])
    return np.array(out)


def min_eigen(gray):
    gx, gy = gradients(gray)
    h, w = gx.shape
    t = [np.pad(a, 1, mode="edge") for a in (gx * gx, gx * gy, gy * gy)]
    a, b, c = (sum(q[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) for q in t)
    return np.maximum(0.5 * ((a + c) - np.sqrt((a - c) ** 2 + 4.0 * b * b)), 0.0)


def round_px(v, n):
    return min(max(int(math.floor(v + 0.5)), 0), n - 1)


def extract(gray, flow, med, p):
    """-> list of (descriptor float64 [dim], points [(x, y)], start) and the five reject counts"""
    T, h, w = gray.shape
    L, step, patch, nxy, nt = p["length"], p["step"], p["patch"], p["nxy"], p["nt"]
    live, found, rej = [], [], [0, 0, 0, 0, 0]
    for t in range(T - 1):
        if t <= T - 1 - L:
            resp = min_eigen(gray[t])
            tq = p["quality"] * resp.max()
            taken = set()
            for tr in live:
                x, y = tr["pts"][-1]
                taken.add((round_px(x, w) // step, round_px(y, h) // step))
            for cy in range(h // step):
                for cx in range(w // step):
                    px, py = cx * step + step // 2, cy * step + step // 2
                    if (cx, cy) not in taken and resp[py, px] > tq:
                        live.append(dict(start=t, pts=[(float(px), float(py))], hist=np.zeros((nt, nxy * nxy, 33))))
        vt = votes(gray[t], flow[t, 0], flow[t, 1], p["min_flow"])
        keep = []
        for tr in live:
            k = t - tr["start"]
            x, y = tr["pts"][-1]
            rx, ry = round_px(x, w), round_px(y, h)
            tr["hist"][k // (L // nt)] += tube_slice(vt, rx, ry, patch, nxy)
            nx, ny = x + float(med[t, 0, ry, rx]), y + float(med[t, 1, ry, rx])
            if not (0.0 <= nx <= w - 1 and 0.0 <= ny <= h - 1):
                rej[0] += 1
                continue
            tr["pts"].append((nx, ny))
            if k + 1 < L:
                keep.append(tr)
                continue
            pts = np.array(tr["pts"])
            sd = pts.std(axis=0)
            seg = np.hypot(*np.diff(pts, axis=0).T)
            if sd[0] < p["min_std"] and sd[1] < p["min_std"]:
                rej[1] += 1
            elif sd[0] > p["max_std"] or sd[1] > p["max_std"]:
                rej[2] += 1
            elif seg.max() > p["max_dis"] or seg.max() > p["max_dis_share"] * seg.sum():
                rej[3] += 1
            else:
                d = [np.diff(pts, axis=0).reshape(-1) / seg.sum()]
                for o, nb in zip(OFFSETS, BINS):
                    blk = tr["hist"][:, :, o:o + nb].reshape(-1)
                    n = np.linalg.norm(blk)
                    d.append(blk / n if n > 0 else blk)
                found.append((np.concatenate(d), tr["pts"], tr["start"]))
        live = keep
    rej[4] = len(live)
    return found, rej
