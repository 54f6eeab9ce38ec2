"""Builds tests/golden/tvl1_median.npz: flows of the median oracle (tests/tvl1_median_oracle.c).

    python tests/golden/make_tvl1_median_golden.py

The 64x48 frames are the ``gray`` of tvl1_64x48.npz (two sequences of three frames: four pairs) and are not stored again.
Schedule of the fixed-mode flows: 5 levels x 3 warps x 30 iterations, the golden schedule of tvl1_64x48.npz.

  flow_m5_e10   [4,2,48,64]  median 5 every 10 iterations (a segment shorter than a four-wave pass of the row pipeline)
  flow_m3_e7    [2,2,48,64]  median 3 every 7 (divides neither 30 nor any block depth); first sequence
  flow_m5_e0    [2,2,48,64]  median 5 once per warp; first sequence
  flow_eps_m5_e30, iters_eps_m5_e30   [2,...]  epsilon 0.01, up to 300 iterations, median 5 every 30; first sequence
  wide_gray     [1,2,40,200] u8: one pair 200 wide x 40 high (two strips of the row pipeline on level 0, a row pitch that
                differs from the width on the two coarsest levels, a coarsest level of 82x17)
  wide_flow_m5_e10  [1,2,40,200]  its flow, median 5 every 10 (the tests derive further sequences from the pair and hold
                those to the oracle itself)

Float fields barely compress; the sequences left out keep the file under 300 KB.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "tvl1_median.npz")
SHORT = dict(epsilon=0.0, iters=30, warps=3)


def wide_gray():
    from video_analytics_amd import synth
    return synth.synth_clips(1, seed=11, H=40, W=200, n_gray=2)[1].numpy()


def arrays():
    import tvl1_median_oracle as mo
    from oracle import tvl1_oracle
    gray = np.load(os.path.join(HERE, "tvl1_64x48.npz"))["gray"]
    short = tvl1_oracle.default_params(**SHORT)
    out = {
        "flow_m5_e10": mo.tvl1_flow(gray, short, 5, 10),
        "flow_m3_e7": mo.tvl1_flow(gray[:1], short, 3, 7),
        "flow_m5_e0": mo.tvl1_flow(gray[:1], short, 5, 0),
    }
    eps, iters = mo.tvl1_flow(gray[:1], tvl1_oracle.default_params(epsilon=0.01, iters=300), 5, 30, return_iters=True)
    out["flow_eps_m5_e30"] = eps
    out["iters_eps_m5_e30"] = iters
    wide = wide_gray()
    out["wide_gray"] = wide
    out["wide_flow_m5_e10"] = mo.tvl1_flow(wide, short, 5, 10)
    return out


if __name__ == "__main__":
    a = arrays()
    np.savez_compressed(OUT, **a)
    print("tvl1_median:", {k: v.shape for k, v in a.items()}, "eps-mode iterations", a["iters_eps_m5_e30"],
          os.path.getsize(OUT), "bytes")
