"""Scenes the space-time interest point tests share -- TEST INFRASTRUCTURE.  numpy and scipy only."""
import numpy as np
from scipy import ndimage


def _texture(rs, h, w, sigma):
    t = ndimage.gaussian_filter(rs.rand(h, w), sigma, mode="wrap")
    return (t - t.min()) / (t.max() - t.min())


def events(T=12, w=48, h=40, seed=3, grid=(5, 4), radius=1.8):
    """A smooth background drifting one pixel per frame, and one small blob in every cell of a grid that reverses, stops or
    appears at a frame of its own.  The blob of the middle cell is the planted event, brighter than any other: it
    moves right and turns back at frame T // 2; ``event`` is its (x, y, t) there.
    -> gray uint8 [T][h][w], flow float32 [T-1][2][h][w] (the planted motion), event"""
    rs = np.random.RandomState(seed)
    back = _texture(rs, h, w + T, 6.0)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    gx, gy = grid
    mid = (gy // 2) * gx + gx // 2
    kinds = ["reverse", "stop", "appear"]
    specs = []
    for b in range(gx * gy):
        cx = (b % gx + 0.5) * w / gx + (0.0 if b == mid else rs.uniform(-1.5, 1.5))
        cy = (b // gx + 0.5) * h / gy + (0.0 if b == mid else rs.uniform(-1.5, 1.5))
        if b == mid:
            specs.append(("reverse", cx, cy, 1.0, 1.0, T // 2))
        else:
            specs.append((kinds[b % 3], cx, cy, rs.uniform(0.6, 1.2) * rs.choice([-1, 1]), rs.uniform(0.5, 0.7) * rs.choice([-1, 1]),
                          int(rs.randint(3, T - 3))))
    gray = np.zeros((T, h, w))
    flow = np.zeros((T - 1, 2, h, w), dtype=np.float32)
    for t in range(T):
        f = 100.0 + 40.0 * back[:, t:t + w]
        if t < T - 1:
            flow[t, 0] = -1.0  # the background drifts left
        for kind, cx, cy, v, amp, tc in specs:
            if kind == "appear" and t < tc:
                continue
            x = cx - v * abs(t - tc) if kind == "reverse" else (cx + v * min(t - tc, 0) if kind == "stop" else cx)
            vel = (v if t < tc else -v) if kind == "reverse" else (v if t < tc and kind == "stop" else 0.0)
            g = np.exp(-((xs - x) ** 2 + (ys - cy) ** 2) / (2 * radius * radius))
            f = f + 110.0 * amp * g
            if t < T - 1:
                flow[t, 0][g > 0.1] = vel
        gray[t] = f
    gray = np.rint(np.clip(gray, 0, 255)).astype(np.uint8)
    return gray, flow, (int(round(specs[mid][1])), int(round(specs[mid][2])), T // 2)
