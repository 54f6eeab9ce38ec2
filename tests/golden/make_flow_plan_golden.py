"""What the Brox and Farneback host logic plans, over a grid of frame sizes and parameters: flow_plans.npz.

    python tests/golden/make_flow_plan_golden.py        # rewrites tests/golden/flow_plans.npz from the built library

The file records `va_brox_workspace_bytes` and `va_farneback_workspace_bytes` and, through a `BroxParams` and a
`FarnebackParams`, `flow.pyramid_sizes`.  Like tvl1_plans.npz (make_tvl1_plan_golden.py) it is written ONCE from the library
of the commit before a refactor of the host side and then holds the refactored library to the same sizes
(tests/test_abi.py); regenerate it only together with a change that means to move a workspace or a level size.
No GPU is needed: every entry point here is host logic.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "flow_plans.npz")

SIZES = ((16, 16), (17, 300), (64, 48), (83, 67), (224, 224), (320, 240), (1280, 720))
N_SEQ = (1, 3)
FRAMES = (2, 11)
STEPS = (0.5, 0.8, 0.95)
LEVELS = (1, 3, 16)
BROX = tuple(dict(whole_field=wf, sweeps_per_launch=k) for wf in (-1, 0) for k in (0, 3))
FARNEBACK = tuple(dict(winsize=ws, poly_n=n) for ws in (3, 15, 63) for n in (5, 7))
MAX_LEVELS = 16


def compute():
    """-> dict(brox_levels, farneback_levels [size, step, levels] int32, brox_sizes, farneback_sizes [size, step, levels, 16, 2]
    int32 (-1 beyond the last level), brox_workspace [size, n_seq, frames, step, levels, BROX] int64, farneback_workspace
    [..., FARNEBACK] int64) from the library that is built in this tree."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from video_analytics_amd import _ffi, flow
    lib = _ffi.lib()
    grid = (len(SIZES), len(STEPS), len(LEVELS))
    methods = (("brox", _ffi.default_brox_params, "scale_step", "nscales", BROX, lib.va_brox_workspace_bytes),
               ("farneback", _ffi.default_farneback_params, "pyr_scale", "levels", FARNEBACK, lib.va_farneback_workspace_bytes))
    got = {}
    for name, defaults, step_name, levels_name, variants, workspace_bytes in methods:
        levels = np.zeros(grid, np.int32)
        sizes = np.full(grid + (MAX_LEVELS, 2), -1, np.int32)
        workspace = np.zeros((len(SIZES), len(N_SEQ), len(FRAMES)) + grid[1:] + (len(variants),), np.int64)
        for i, (w, h) in enumerate(SIZES):
            for j, step in enumerate(STEPS):
                for k, nlev in enumerate(LEVELS):
                    for v, kw in enumerate(variants):
                        p = defaults(**dict(kw, **{step_name: step, levels_name: nlev}))
                        if v == 0:
                            pyr = flow.pyramid_sizes(w, h, p)
                            levels[i, j, k] = len(pyr)
                            sizes[i, j, k, :len(pyr)] = pyr
                        for a, n_seq in enumerate(N_SEQ):
                            for b, fps in enumerate(FRAMES):
                                workspace[i, a, b, j, k, v] = workspace_bytes(w, h, n_seq, fps, ctypes.byref(p))
        got[name + "_levels"], got[name + "_sizes"], got[name + "_workspace"] = levels, sizes, workspace
    return got


if __name__ == "__main__":
    got = compute()
    np.savez_compressed(OUT, **got)
    print("%s: %d bytes, %d pyramids, %d workspace sizes" % (OUT, os.path.getsize(OUT),
                                                               got["brox_levels"].size + got["farneback_levels"].size,
                                                               got["brox_workspace"].size + got["farneback_workspace"].size))
