"""What a Brox or Farneback call reaches inside the library -- TEST INFRASTRUCTURE, never imported by the product.

The arithmetic of ``pick_shape``, ``launch_inner`` and ``run_inner_step`` (csrc/brox.hip) and of ``pass_tile`` and
``poly_tile`` (csrc/farneback.hip), restated in Python with the constants written out.  The limit cases of
tests/test_brox_params_gpu.py and tests/test_farneback_params_gpu.py assert through it that they reach the kernel form they
are named for, so that a changed constant in the library turns them red, not hollow; tests/test_brox_host.py and
tests/test_farneback_host.py pin it to the library where the library's decision shows without a GPU
(``va_*_workspace_bytes`` is 0 for a refused tuning).  The tables of limit cases live here, so that the host tests can
confirm every one of them legal before the GPU tests launch it.
"""

import numpy as np

MAX_LDS = 160 * 1024  # kVaMaxLds: what one workgroup holds

# ---------------------------------------------------------------- Brox (csrc/brox.hip)

BROX_MAX_PAIRS = 3072  # kMaxPairs
BROX_MAX_K = 17        # kMaxK
BROX_DEFAULT_K = 5     # kDefaultK
BROX_MAX_SIDE = 78     # kMaxSide


def _cdiv(a, b):
    return (a + b - 1) // b


def _pairs(rw, rh):
    return ((rw + 1) // 2) * rh


def brox_form(pairs):
    """``launch_inner``: (NT, PPT) of the instantiation that runs a largest region of ``pairs`` pixel pairs"""
    if pairs <= 256:
        return (256, 1)
    if pairs <= 1024:
        return (256, 4)
    if pairs <= 2048:
        return (1024, 2)
    return (1024, 3)


def brox_shape(w, h, solver_iters, whole_field=-1, tile_w=0, tile_h=0, sweeps_per_launch=0):
    """``pick_shape`` and what follows from it for one inner step on a field of w x h -> dict(whole, TW, TH, ntx, nty, K, H,
    rw, rh: the largest region, pairs, lds: bytes, form: (NT, PPT), launches: sweeps of every launch of a step), or None
    where the library refuses the tuning"""
    if whole_field == -1 and _pairs(w, h) <= BROX_MAX_PAIRS:
        s = dict(whole=True, TW=w, TH=h, ntx=1, nty=1, K=solver_iters, H=0, rw=w, rh=h)
        s["launches"] = [solver_iters]
    else:
        K = min(sweeps_per_launch if sweeps_per_launch > 0 else BROX_DEFAULT_K, solver_iters)
        H = 2 * K + 2
        T = (BROX_MAX_SIDE - 2 * H) & ~1
        TW = min(tile_w if tile_w > 0 else _cdiv(w, _cdiv(w, T)), w)
        TH = min(tile_h if tile_h > 0 else _cdiv(h, _cdiv(h, T)), h)
        s = dict(whole=False, TW=TW, TH=TH, ntx=_cdiv(w, TW), nty=_cdiv(h, TH), K=K, H=H, rw=min(TW + 2 * H, w), rh=min(TH + 2 * H, h))
        nl = _cdiv(solver_iters, K)
        base, extra = solver_iters // nl, solver_iters % nl
        s["launches"] = [base + (1 if i < extra else 0) for i in range(nl)]
    s["pairs"] = _pairs(s["rw"], s["rh"])
    s["lds"] = (s["rw"] + 2) * (s["rh"] + 2) * 12
    s["form"] = brox_form(s["pairs"])
    if s["pairs"] > BROX_MAX_PAIRS:
        return None
    assert s["lds"] <= MAX_LDS and sum(s["launches"]) == solver_iters
    return s


def brox_regions(shape, w, h):
    """``k_brox_inner``'s own arithmetic -> (RW, RH) of every tile's region: the tile and its halo, cut by the field's border
    (``shape['pairs']`` is what the launch is sized for; a tile at the border runs less)"""
    out = []
    for ty in range(shape["nty"]):
        for tx in range(shape["ntx"]):
            cx0, cy0 = tx * shape["TW"], ty * shape["TH"]
            cx1, cy1 = min(cx0 + shape["TW"], w), min(cy0 + shape["TH"], h)
            out.append((min(cx1 + shape["H"], w) - max(cx0 - shape["H"], 0), min(cy1 + shape["H"], h) - max(cy0 - shape["H"], 0)))
    return out


def brox_rotation(shape, inner_iters):
    """``run_inner_step``, step after step from buffer 0 -> the buffer that holds (du, dv) after every inner step"""
    cur, ends = 0, []
    for _ in range(inner_iters):
        if not shape["whole"]:
            other = ((cur + 1) % 3, (cur + 2) % 3)
            for i in range(len(shape["launches"])):
                cur = other[i & 1]
        ends.append(cur)
    return ends


# va_brox_inner_step on whole fields, at both sides of every number launch_inner and pick_shape compare with:
# (w, h, solver_iters, pixel pairs, (NT, PPT)); the last is the first field the library tiles on its own
BROX_WHOLE_CASES = [
    (32, 16, 3, 256, (256, 1)),
    (33, 16, 3, 272, (256, 4)),
    (32, 64, 3, 1024, (256, 4)),
    (49, 41, 3, 1025, (1024, 2)),
    (64, 64, 3, 2048, (1024, 2)),
    (65, 63, 3, 2079, (1024, 3)),
    (96, 64, 3, 3072, (1024, 3)),   # the last whole field
    (384, 16, 3, 3072, (1024, 3)),  # LDS rows of 386 cells
    (16, 384, 3, 3072, (1024, 3)),  # 386 LDS rows
]
# 97 x 64 = 3136 pairs: the first field the library tiles on its own.  solver_iters 5 lets K be kDefaultK: H 12, tiles of
# 49 x 32; the launch is sized for regions of 73 x 56 = 2072 pairs (above 2048: three pairs per lane), though with two tiles
# a side every region is cut by the field's border to 61 x 44 at the most.
# 150 x 63 in three tiles of 50 x 63 with K 3: the middle tile's region is 66 x 63 = 2079 pairs and as high as the field, so
# that the pairs past the first 2048 are pixels of the result (in a region with a halo below, they would be halo)
BROX_TILED_CASES = [
    dict(w=97, h=64, solver_iters=5, tuning=dict(), K=5, H=12, TW=49, TH=32, rw=73, rh=56, pairs=2072, form=(1024, 3), runs=31 * 44),
    dict(w=150, h=63, solver_iters=3, tuning=dict(whole_field=0, tile_w=50, tile_h=63, sweeps_per_launch=3), K=3, H=8, TW=50, TH=63,
         rw=66, rh=63, pairs=2079, form=(1024, 3), runs=2079),
]

# the sweep split of a tiled step (whole_field = 0, the library's own tiles), on 97 x 64 and on 150 x 131:
# (solver_iters, sweeps_per_launch, K, sweeps of every launch)
BROX_SPLIT_CASES = [
    (7, 3, 3, [3, 2, 2]),         # an odd number of launches
    (8, 3, 3, [3, 3, 2]),
    (4, 9, 4, [4]),               # K clamped to solver_iters
    (17, 17, 17, [17]),           # kMaxK: halo 36, tiles of 6 x 6, regions of 78 x 78
    (40, 17, 17, [14, 13, 13]),
]
BROX_SPLIT_FIELDS = [(97, 64), (150, 131)]

# ---------------------------------------------------------------- Farneback (csrc/farneback.hip)

FB_DEF_TILE = (32, 16)  # kDefTileW, kDefTileH


def pass_lds(winsize, tw, th):
    """dynamic LDS of ``k_farneback_pass`` with a tile of tw x th, bytes"""
    m = winsize // 2
    rw, rh = tw + 2 * m, th + 2 * m
    return 5 * (rw * rh + rw * th) * 4


def pass_tile(winsize, tile_w=0, tile_h=0):
    """``pass_tile`` -> (TW, TH, LDS bytes), or None where the library refuses the caller's tile"""
    own = bool(tile_w or tile_h)
    tw, th = tile_w or FB_DEF_TILE[0], tile_h or FB_DEF_TILE[1]
    while True:
        lds = pass_lds(winsize, tw, th)
        if lds <= MAX_LDS:
            return tw, th, lds
        if own or tw * th <= 64:
            return None
        if tw > th:
            tw //= 2
        else:
            th //= 2


def poly_lds(poly_n, tw, th):
    """dynamic LDS of ``k_farneback_polyexp`` with a tile of tw x th, bytes"""
    rw, rh = tw + 2 * poly_n, th + 2 * poly_n
    return (rw * rh + 3 * rw * th) * 4


def poly_tile(poly_n, tile_w=0, tile_h=0):
    """``poly_tile`` -> (TW, TH, LDS bytes), or None where the library refuses the tile"""
    tw, th = tile_w or FB_DEF_TILE[0], tile_h or FB_DEF_TILE[1]
    lds = poly_lds(poly_n, tw, th)
    return (tw, th, lds) if lds <= MAX_LDS else None


# va_farneback_pass at the limits of the window: (winsize, caller's tile or (0, 0), the tile that runs, LDS bytes, fields)
FB_PASS_FIELDS = [(83, 67), (20, 16)]
FB_PASS_CASES = [
    (3, (0, 0), (32, 16), 23120, FB_PASS_FIELDS),    # narrower than the five-pixel border weights
    (5, (0, 0), (32, 16), 25920, FB_PASS_FIELDS),
    (59, (0, 0), (32, 16), 162000, FB_PASS_FIELDS),  # 1,840 B below the limit
    (61, (0, 0), (16, 16), 139840, FB_PASS_FIELDS),  # the library's tile halved
    (63, (0, 0), (16, 16), 146640, FB_PASS_FIELDS),
    (63, (16, 16), (16, 16), 146640, FB_PASS_FIELDS),
    (31, (64, 16), (64, 16), 116560, FB_PASS_FIELDS),
    (15, (1, 1), (1, 1), 4800, [(20, 16)]),
]

# va_farneback_polyexp: (poly_n, poly_sigma, caller's tile or (0, 0), LDS bytes, (w, h))
FB_POLY_CASES = [
    (5, 0.6, (0, 0), 12432, (83, 67)), (7, 0.6, (0, 0), 14352, (83, 67)),
    (5, 3.0, (0, 0), 12432, (83, 67)), (7, 3.0, (0, 0), 14352, (83, 67)),
    (5, 1.2, (128, 64), 146832, (150, 131)), (7, 1.5, (128, 64), 153360, (150, 131)),  # more than 64 KB of LDS
    (5, 1.2, (256, 8), 44688, (150, 131)),
    (5, 1.2, (1, 1), 616, (16, 16)), (7, 1.5, (1, 1), 1080, (16, 16)),
]

# ---------------------------------------------------------------- frame content the synthetic clips do not produce

CONTENTS = ("constant", "checker", "leaving")


def _smooth_texture(H, W, seed):
    """a random texture in [0,255] smoothed by five passes of a 3 x 3 box, float64"""
    t = np.random.RandomState(seed).rand(H, W)
    for _ in range(5):
        p = np.pad(t, 1, mode="edge")
        t = sum(p[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    return (t - t.min()) / (t.max() - t.min()) * 255.0


def _sample(img, px, py):
    h, w = img.shape
    x, y = np.clip(px, 0.0, w - 1.0), np.clip(py, 0.0, h - 1.0)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = x - x0, y - y0
    return (1 - ay) * ((1 - ax) * img[y0, x0] + ax * img[y0, x1]) + ay * ((1 - ax) * img[y1, x0] + ax * img[y1, x1])


def content_pairs(name, H, W):
    """three pairs of one content class -> uint8 [3,2,H,W]
    constant: two identical constant frames (0, 128 and 255): no gradient anywhere, the flow is exactly 0
    checker:  a 0/255 checkerboard (cells of 1, 2 and 3 pixels) and the same board moved by one pixel (in x, in y, in both)
    leaving:  a texture and the same texture magnified about the frame's centre (by 1.1, 1.15 and 1.2): the flow points
              outwards everywhere and leaves the frame on all four sides"""
    yy, xx = np.mgrid[0:H, 0:W]
    if name == "constant":
        return np.stack([np.full((2, H, W), c, dtype=np.uint8) for c in (0, 128, 255)])
    if name == "checker":
        board = lambda n, x, y: ((((x // n) + (y // n)) & 1) * 255).astype(np.uint8)
        return np.stack([np.stack([board(n, xx, yy), board(n, xx + dx, yy + dy)]) for n, dx, dy in ((1, 1, 0), (2, 0, 1), (3, 1, 1))])
    if name == "leaving":
        out = []
        for k, s in enumerate((1.1, 1.15, 1.2)):
            t = _smooth_texture(H, W, 1000 * H + W + k)
            cx, cy = 0.5 * (W - 1), 0.5 * (H - 1)
            out.append(np.stack([t, _sample(t, cx + (xx - cx) / s, cy + (yy - cy) / s)]))
        return np.rint(np.stack(out)).astype(np.uint8)
    raise KeyError(name)


def leaves_on_all_sides(flow):
    """flow [n,2,H,W]: in every pair x + u or y + v lies outside the frame past each of its four sides"""
    n, _, H, W = flow.shape
    px, py = flow[:, 0] + np.arange(W, dtype=np.float32), flow[:, 1] + np.arange(H, dtype=np.float32)[:, None]
    sides = [(px < 0).reshape(n, -1).any(1), (px > W - 1).reshape(n, -1).any(1), (py < 0).reshape(n, -1).any(1), (py > H - 1).reshape(n, -1).any(1)]
    return bool(np.all(sides))
