"""The bodies of the TV-L1 row pipeline (k_iter_stream), one small frame per path, bit-exact against the C oracle.

A strip that ends before the image's last column runs a copy of the pipeline without the right-border multiplier
(DESIGN.md section 7); the last strip of a row, the shared last strips of two pairs and single-strip levels run the
generic copy.  Each frame below is a few rows high; three pairs give the shared-strip form a couple of pairs and an odd
last one.  tile_mask bit 8 forces the row pipeline on every level.

What each frame runs is asserted from the launch report (``CLAIMS`` names the case of tests/test_tvl1_launches_gpu.py with
the same frame and parameters, whose ``must`` holds the path).  The report showed that four of the six iteration counts fall
back to the two-wave and one-wave forms (a four-wave pass needs more than three quarters of its depth): the paths first
claimed here -- 4 x 4, 4 x 5 with passes of unequal K, shared last strips at 143 columns -- run in the ``rows_*`` cases of that
file, on the same frames at other iteration counts.
"""
import numpy as np
import pytest
import torch

from test_tvl1_launches_gpu import CASES, assert_claims

pytestmark = pytest.mark.gpu

# (W, H, iters, stream_waves) -> the case of tests/test_tvl1_launches_gpu.py that states what this call launches
CLAIMS = {
    (224, 40, 37, 0): "rows_224x40_37_fallback",  # two strips, inner + last: 2 x 8, 2 x 8, then 5 iterations in one wave
    (179, 33, 41, 0): "rows_179x33_41_fallback",  # two strips, 20-column halo: 2 x 8 three times (16 + 16 + 9)
    (143, 30, 41, 0): "rows_143x30_41_fallback",  # inner strip + last strip, 2 x 8: no shared last strips in this form
    (130, 24, 16, 0): "rows_130x24_last_strip_two_columns",  # 4 x 5, one pass; shared last strips, half = 1 and 2
    (114, 30, 33, 0): "rows_114x30_33_fallback",  # single strip, the generic body: 2 x 8, 2 x 8, 1 x 10
    (300, 20, 25, 0): "rows_300x20_25_one_wave",  # three strips: an inner strip with halos on both sides, 1 x 10
    (224, 40, 37, 1): "rows_224x40_one_wave",
    (224, 40, 37, 2): "rows_224x40_two_waves",
}


def _check(oracle_tvl1, W, H, iters, **tuning):
    from video_analytics_amd import flow as vflow
    from video_analytics_amd import synth
    _, gray, _ = synth.synth_clips(3, seed=7 * W + H, H=H, W=W, n_gray=2)  # 3 sequences x 2 frames: 3 pairs
    kw = dict(epsilon=0.0, iters=iters, warps=2, nscales=1)
    cid = CLAIMS[(W, H, iters, tuning.get("stream_waves", 0))]
    case = CASES[cid]
    assert (case["W"], case["H"], case["S"], case["F"]) == (W, H, 3, 2) and case["kw"] == dict(kw, tile_mask=1 << 8, **tuning), cid
    assert_claims(cid)
    ref = oracle_tvl1.tvl1_flow(gray.numpy(), oracle_tvl1.default_params(**kw), nthreads=8)
    out = vflow.tvl1_flow(gray.cuda(), tile_mask=1 << 8, **kw, **tuning)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.shape == ref.shape == (3, 2, H, W)
    assert np.array_equal(out, ref), "max abs diff %g" % np.abs(out - ref).max()


@pytest.mark.parametrize("W,H,iters", [
    (224, 40, 37),
    (179, 33, 41),
    (143, 30, 41),
    (130, 24, 16),
    (114, 30, 33),
    (300, 20, 25),
])
def test_row_pipeline_paths_bit_exact(oracle_tvl1, W, H, iters):
    _check(oracle_tvl1, W, H, iters)


@pytest.mark.parametrize("waves", [1, 2])
def test_row_pipeline_fallback_forms_bit_exact(oracle_tvl1, waves):
    # the one-wave and two-wave forms share stream_job (and its LDS arrays) with the four-wave forms
    _check(oracle_tvl1, 224, 40, 37, stream_waves=waves)
