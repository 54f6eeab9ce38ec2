"""What the TV-L1 host logic plans, over a grid of frame sizes and tuning values: tvl1_plans.npz.

    python tests/golden/make_tvl1_plan_golden.py        # rewrites tests/golden/tvl1_plans.npz from the built library

The file records `flow.tile_plan(w, h, p)` (every level, all six fields) and `va_tvl1_workspace_bytes(w, h, n_seq, 2, p)`.
It is written ONCE from the library of the commit before a refactor of the host side and then holds the refactored
library to the same decisions (tests/test_abi.py); regenerate it only together with a change that means to move a plan.
No GPU is needed: both entry points are host logic.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "tvl1_plans.npz")

WIDTHS = (16, 17, 64, 100, 114, 128, 129, 131, 143, 179, 190, 224, 225, 256, 257, 300, 400, 700, 1280, 1920)
HEIGHTS = (16, 33, 57, 91, 224, 720, 1080)
N_SEQ = (1, 3, 320)
PARAMS = (dict(), dict(stream_waves=1), dict(stream_waves=2), dict(stream_waves=7), dict(stream_waves=8), dict(stream_waves=9),
          dict(tile_mask=1 << 8), dict(tile_mask=(1 << 8) | (1 << 10)), dict(iters=10), dict(iters=23), dict(iters=300))
MAX_LEVELS = 16
KEYS = ("tile_w", "tile_h", "waves", "block_iters", "tiles_x", "tiles_y")


def compute():
    """-> dict(levels [W, H, P] int32, plans [W, H, P, 16, 6] int32 (-1 beyond the last level),
    workspace [W, H, N, P] int64) from the library that is built in this tree."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from video_analytics_amd import _ffi, flow
    lib = _ffi.lib()
    lib.va_tvl1_workspace_bytes.restype = ctypes.c_size_t
    nw, nh, nn, npar = len(WIDTHS), len(HEIGHTS), len(N_SEQ), len(PARAMS)
    levels = np.zeros((nw, nh, npar), np.int32)
    plans = np.full((nw, nh, npar, MAX_LEVELS, len(KEYS)), -1, np.int32)
    workspace = np.zeros((nw, nh, nn, npar), np.int64)
    for k, kw in enumerate(PARAMS):
        p = _ffi.default_tvl1_params(epsilon=0.0, **kw)
        for i, w in enumerate(WIDTHS):
            for j, h in enumerate(HEIGHTS):
                plan = flow.tile_plan(w, h, p)
                levels[i, j, k] = len(plan)
                for s, d in enumerate(plan):
                    plans[i, j, k, s] = [d[key] for key in KEYS]
                for m, n in enumerate(N_SEQ):
                    workspace[i, j, m, k] = lib.va_tvl1_workspace_bytes(w, h, n, 2, ctypes.byref(p))
    return dict(levels=levels, plans=plans, workspace=workspace)


if __name__ == "__main__":
    got = compute()
    np.savez_compressed(OUT, **got)
    print("%s: %d bytes, %d plans, %d workspace sizes" % (OUT, os.path.getsize(OUT), got["levels"].size, got["workspace"].size))
