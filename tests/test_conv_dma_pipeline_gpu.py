"""The software pipeline of k_conv3x3_dma_f32's K loop, at the shapes where a pipeline goes wrong.

The kernel reads the fragments of K sub-step ks + 1 before the MFMAs of ks (two register sets), forms the next K step's
DMA offsets beside the last sub-step's MFMAs (one-buffer form: one step ahead of their use) and issues the ring's refill
right behind the first fragment reads (ring form); out-of-image taps are out-of-range buffer offsets.  What such a
pipeline gets wrong is its first and last sub-step and its first and last K step, so every instantiation runs here with
  * cin = 32: ONE channel chunk per tap (nine K steps: every tap's first step is also its last),
  * cin = 96: an odd number of chunks per tap (27 K steps),
  * hw = 28 and hw = 12: frames that leave partial bricks, and
  * batches that are no multiple of the brick's batch depth (hw = 12 bricks span several images).

Per case: the output of the LDS-DMA kernel (``kernel_opt`` 1) equals the register-staged kernel's (``kernel_opt`` 0, the
witness: the same products in the same order, another staging path, no pipeline) bit for bit; two launches agree bit
for bit; the canaries around ``out`` and the guards around ``in`` hold (``_run``); and the float64 rule of
tests/test_conv_layers_gpu.py holds (reference and error rule are imported from there, not restated).
"""
import pytest
import torch

from test_conv_layers_gpu import F_, T, _c, _check_against_reference, _dma, _make_inputs, _run, reference_layer

# id -> (case, instantiation the LDS-DMA path must reach).  Grids: 128-pixel bricks x 64 channels; the ring below 1024 of
# them, else 128-channel tiles where cout % 128 == 0, else 64-channel tiles.  28 x 28 frames in 32 x 4 bricks: 7 per image;
# 12 x 12 frames: at least 144 / 128 bricks per image whatever the brick, so 65 images x 14 or 15 channel tiles pass 1024.
CASES = {
    # ---- ring form (NBUF = 3)
    "ring_hw12_cin32_b5": (_c("f32", 12, 32, 64, False, 5, None), _dma(1, F_, 3)),
    "ring_hw12_cin96_pool_b5": (_c("f32", 12, 96, 128, True, 5, None), _dma(1, T, 3)),
    "ring_hw28_cin32_pool_b3": (_c("f32", 28, 32, 64, True, 3, None), _dma(1, T, 3)),
    "ring_hw28_cin96_b3": (_c("f32", 28, 96, 128, False, 3, None), _dma(1, F_, 3)),
    # ---- one buffer, 128-channel tiles
    "wide_hw28_cin32_pool_b33": (_c("f32", 28, 32, 384, True, 33, None), _dma(2, T, 1)),
    "wide_hw28_cin96_b33": (_c("f32", 28, 96, 384, False, 33, None), _dma(2, F_, 1)),
    "wide_hw12_cin32_b65": (_c("f32", 12, 32, 896, False, 65, None), _dma(2, F_, 1)),
    "wide_hw12_cin96_pool_b65": (_c("f32", 12, 96, 896, True, 65, None), _dma(2, T, 1)),
    # ---- one buffer, 64-channel tiles
    "single_hw28_cin32_b33": (_c("f32", 28, 32, 320, False, 33, None), _dma(1, F_, 1)),
    "single_hw28_cin96_pool_b33": (_c("f32", 28, 96, 320, True, 33, None), _dma(1, T, 1)),
    "single_hw12_cin32_pool_b65": (_c("f32", 12, 32, 960, True, 65, None), _dma(1, T, 1)),
    "single_hw12_cin96_b65": (_c("f32", 12, 96, 960, False, 65, None), _dma(1, F_, 1)),
}


def test_cases_reach_every_instantiation_with_both_chunk_counts_and_both_frame_sizes():
    """CPU: the table itself -- six instantiations, each with cin 32 and cin 96, each with hw 12 and hw 28."""
    seen = {}
    for case, name in CASES.values():
        seen.setdefault(name, []).append(case)
    assert sorted(seen) == sorted(_dma(nt, p, nb) for nt, nb in ((1, 3), (2, 1), (1, 1)) for p in (T, F_))
    for name, cases in seen.items():
        assert {c["cin"] for c in cases} == {32, 96}, name
        assert {c["hw"] for c in cases} == {12, 28}, name


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(CASES))
def test_dma_pipeline_matches_the_register_staged_kernel_bit_for_bit(cid):
    case, want = CASES[cid]
    inp = _make_inputs(case, seed=sum(map(ord, cid)))
    zeros = torch.zeros(64, dtype=torch.float32, device="cuda")
    name, out1 = _run(case, inp, 1, zeros)
    assert name == want, (cid, name, want)
    _, out2 = _run(case, inp, 1, zeros)
    assert torch.equal(out1.view(torch.uint8), out2.view(torch.uint8)), (cid, name, "not deterministic")
    wname, wit = _run(case, inp, 0, zeros)
    assert wname.startswith("k_conv3x3_mfma<"), (cid, wname)
    diff = out1.view(torch.int32) != wit.view(torch.int32)
    assert not bool(diff.any()), (cid, name, "differs from", wname, int(diff.sum()), "values; first at",
                                  [int(v) for v in diff.nonzero()[0]])
    ref, pre, s = reference_layer(inp["x"], inp["w"], inp["b"], case["pool"])
    r = _check_against_reference(case, out1, ref, pre, s, (cid, name))
    print("%s: %s, worst normalised fp32 error %.3g" % (cid, name, r))
