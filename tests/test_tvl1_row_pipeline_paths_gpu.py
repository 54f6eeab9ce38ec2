"""The bodies of the TV-L1 row pipeline (k_iter_stream), one small frame per path, bit-exact against the C oracle.

A strip that ends before the image's last column runs a copy of the pipeline without the right-border multiplier
(DESIGN.md section 7); the last strip of a row, the shared last strips of two pairs and single-strip levels run the
generic copy.  Each frame below is the smallest that takes one of these paths, a few rows high; three pairs give the
shared-strip form a couple of pairs and an odd last one.  tile_mask bit 8 forces the row pipeline on every level.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _check(oracle_tvl1, W, H, iters, **tuning):
    from video_analytics_amd import flow as vflow
    from video_analytics_amd import synth
    _, gray, _ = synth.synth_clips(3, seed=7 * W + H, H=H, W=W, n_gray=2)  # 3 sequences x 2 frames: 3 pairs
    kw = dict(epsilon=0.0, iters=iters, warps=2, nscales=1)
    ref = oracle_tvl1.tvl1_flow(gray.numpy(), oracle_tvl1.default_params(**kw), nthreads=8)
    out = vflow.tvl1_flow(gray.cuda(), tile_mask=1 << 8, **kw, **tuning)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.shape == ref.shape == (3, 2, H, W)
    assert np.array_equal(out, ref), "max abs diff %g" % np.abs(out - ref).max()


@pytest.mark.parametrize("W,H,iters", [
    (224, 40, 37),  # two strips, inner + last, 4 x 4
    (179, 33, 41),  # two strips, 4 x 5; passes of unequal K
    (143, 30, 41),  # inner strip + shared last strips, half = 1 and 2
    (130, 24, 16),  # last strip two columns wide
    (114, 30, 33),  # single strip, the generic body
    (300, 20, 25),  # three strips: an inner strip with halos on both sides
])
def test_row_pipeline_paths_bit_exact(oracle_tvl1, W, H, iters):
    _check(oracle_tvl1, W, H, iters)


@pytest.mark.parametrize("waves", [1, 2])
def test_row_pipeline_fallback_forms_bit_exact(oracle_tvl1, waves):
    # the one-wave and two-wave forms share stream_job (and its LDS arrays) with the four-wave forms
    _check(oracle_tvl1, 224, 40, 37, stream_waves=waves)
