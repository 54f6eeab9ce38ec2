"""Scenes the dense-trajectory tests share -- TEST INFRASTRUCTURE."""
import numpy as np


def texture(n, w, h, seed):
    """n smooth random fields in [0,255], float32, not whole numbers (the recipe of tests/test_farneback_gpu.py's _texture)"""
    import torch
    from video_analytics_amd import synth
    t = torch.from_numpy(np.random.RandomState(seed).rand(n, 1, h, w).astype(np.float32))
    t = synth._blur(t, 1.0)[:, 0]
    t = (t - t.amin()) / (t.amax() - t.amin()) * 255.0
    return t.numpy().astype(np.float32)


BOX = dict(x=2, y=2, w=52, h=30, dx=2, dy=1)


def planted(T=12, w=80, h=64, seed=5, box=BOX):
    """A textured box moving (dx, dy) px per frame over a still textured background, and its exact flow.
    -> gray uint8 [T][h][w], flow float32 [T-1][2][h][w], the box's rectangles [(x0, y0, x1, y1)] per frame"""
    back, front = texture(2, w, h, seed)
    gray = np.zeros((T, h, w), dtype=np.uint8)
    flow = np.zeros((T - 1, 2, h, w), dtype=np.float32)
    rects = []
    for t in range(T):
        x0, y0 = box["x"] + box["dx"] * t, box["y"] + box["dy"] * t
        x1, y1 = x0 + box["w"], y0 + box["h"]
        assert 0 <= x0 and x1 <= w and 0 <= y0 and y1 <= h
        f = np.rint(back).astype(np.uint8)
        f[y0:y1, x0:x1] = np.rint(front[:box["h"], :box["w"]]).astype(np.uint8)
        gray[t] = f
        rects.append((x0, y0, x1, y1))
        if t < T - 1:
            flow[t, 0, y0:y1, x0:x1] = box["dx"]
            flow[t, 1, y0:y1, x0:x1] = box["dy"]
    return gray, flow, rects
