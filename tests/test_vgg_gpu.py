"""GPU parity of the VGG-16 stream (HIP conv/FC kernels through the C ABI) against the torch-CPU
oracle (oracle/vgg_oracle.py).  Tolerance: the north star's 1e-3 absolute on fp32 class scores
(activations are O(1) by construction of the synthetic weights); observed error is ~1e-5.
PARITY UNPINNED against the reference itself (no tests/goldens/checkpoints ship with it)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-3


@pytest.fixture(scope="module")
def weights3():
    from video_analytics_amd import synth
    return synth.synth_vgg16_weights(c_in=3, seed=1)


def _inputs(B, C, seed):
    from video_analytics_amd import synth
    u = synth.hash_uniform(seed, 77, B * C * 224 * 224).reshape(B, C, 224, 224)
    return torch.from_numpy(u * 4.0 - 2.0)  # roughly the range of normalised images


def test_copy_first_layer_matches_reference_rule(weights3):
    from oracle import vgg_oracle
    from video_analytics_amd import vgg
    ref = vgg_oracle.copy_first_layer(weights3["conv_w"][0], 20)
    out = vgg.copy_first_layer(weights3["conv_w"][0].cuda(), 20).cpu()
    assert out.shape == (64, 20, 3, 3)
    assert torch.equal(out, ref)


def test_copy_first_layer_equals_the_reference_run():
    """``va_copy_first_layer`` against the output of the reference's own ``TemporalNetwork.__copyFirstLayer__``
    (Sheet03/temporalModel.py:149-162, executed in the build container by tests/golden/make_reference_fixtures.py on a
    seeded ``Conv2d(3, 64, 3, padding=1)``): bit-equal."""
    import os
    from video_analytics_amd import vgg
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_model_kats.npz"))
    w_in, w_out = torch.from_numpy(z["copyFirstLayer_w_in"]), torch.from_numpy(z["copyFirstLayer_w_out"])
    out = vgg.copy_first_layer(w_in.cuda(), 20).cpu()
    assert out.shape == (64, 20, 3, 3) and torch.equal(out, w_out)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_result_does_not_depend_on_what_the_workspace_held(weights3, dtype):
    # the caller owns the workspace: NaN bit patterns everywhere must not leak into the result
    from video_analytics_amd import vgg
    w = weights3
    x = _inputs(3, 3, seed=8).cuda()
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, dtype=dtype)
    a = [t.clone() for t in m.forward(x, want_feat=True)]
    for t in vgg._ws_cache.values():
        t.fill_(0xFF)
    b = m.forward(x, want_feat=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    m.close()


@pytest.mark.parametrize("B", [1, 3])
def test_spatial_stream_matches_oracle(weights3, B):
    from oracle import vgg_oracle
    from video_analytics_amd import vgg
    w = weights3
    x = _inputs(B, 3, seed=5)
    feat_r, desc_r, log_r = vgg_oracle.forward(x, w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"])
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    feat, desc, logits = m.forward(x.cuda(), want_feat=True)
    torch.cuda.synchronize()
    assert float(log_r.abs().max()) > 0.05  # the comparison is not vacuous
    assert float((feat.cpu() - feat_r).abs().max()) < TOL
    assert float((desc.cpu() - desc_r).abs().max()) < TOL
    assert float((logits.cpu() - log_r).abs().max()) < TOL
    assert torch.equal(logits.cpu().argmax(1), log_r.argmax(1))
    m.close()


def test_temporal_stream_matches_oracle(weights3):
    from oracle import vgg_oracle
    from video_analytics_amd import synth, vgg
    w = synth.synth_vgg16_weights(c_in=20, seed=2)
    w0 = vgg_oracle.copy_first_layer(w["conv_w"][0], 20)
    conv_w = [w0] + w["conv_w"][1:]
    x = _inputs(2, 20, seed=6)
    feat_r, desc_r, log_r = vgg_oracle.forward(x, conv_w, w["conv_b"], w["fc_w"], w["fc_b"])
    m = vgg.Vgg16Stream(conv_w, w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    feat, desc, logits = m.forward(x.cuda(), want_feat=True)
    assert float((feat.cpu() - feat_r).abs().max()) < TOL
    assert float((desc.cpu() - desc_r).abs().max()) < TOL
    assert float((logits.cpu() - log_r).abs().max()) < TOL
    m.close()


def test_u8_input_normalisation_matches_oracle(weights3):
    from oracle import vgg_oracle
    from video_analytics_amd import synth, vgg
    from video_analytics_amd.parameters import NORM_MEANS_TF, NORM_STDS_TF
    w = weights3
    rgb, _, _ = synth.synth_clips(2, seed=3)
    xr = vgg_oracle.normalize_u8(rgb, NORM_MEANS_TF, NORM_STDS_TF)
    _, desc_r, log_r = vgg_oracle.forward(xr, w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"])
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, NORM_MEANS_TF, NORM_STDS_TF)
    _, desc, logits = m.forward(rgb.cuda())
    assert float((logits.cpu() - log_r).abs().max()) < TOL
    assert float((desc.cpu() - desc_r).abs().max()) < TOL
    m.close()


@pytest.mark.parametrize("c_in", [1, 2, 5, 8, 21])
def test_bf16_fused_first_layer_other_channel_counts(weights3, c_in):
    # the fused first layer pads the channels of its LDS patch to a multiple of 4 and a kernel row to 16-element blocks:
    # 1 -> 4 / 16, 5 -> 8 / 32, 21 -> 24 / 80 (the largest it accepts); against the staged path (input conversion + three K
    # steps), which is bit-equal when no channel is padded (8) and within bf16 noise otherwise
    from video_analytics_amd import _ffi, vgg
    w = {k: [t.clone() for t in v] for k, v in weights3.items()}
    g = torch.Generator().manual_seed(100 + c_in)  # (distinct weights per channel and tap: a permuted K order would show)
    w["conv_w"][0] = torch.randn(64, c_in, 3, 3, generator=g) * float(w["conv_w"][0].std()) * (3.0 / c_in) ** 0.5
    x = _inputs(2, c_in, seed=40 + c_in).cuda()
    outs = []
    for first in (1, 0):
        m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, dtype="bf16")
        m.set_option(_ffi.VA_OPT_BF16_FIRST_LAYER, first)
        feat, _, logits = m.forward(x, want_feat=True)
        outs.append((feat.cpu(), logits.cpu()))
        m.close()
    ls = float(outs[1][1].abs().max())
    assert float((outs[0][1] - outs[1][1]).abs().max()) / ls < 1e-2
    if c_in % 4 == 0:
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_bf16_batch_beyond_32bit_buffer_offsets_is_rejected(weights3):
    # the bf16 staging addresses a layer's activations with 32-bit byte offsets: 336 images x 224 x 224 x 64 bf16 channels
    # are 2.16 GB -- refused with a message (the fp32 path has no such limit); 330 images (2.12 GB < 2^31) still run
    from video_analytics_amd import vgg
    w = weights3
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, dtype="bf16")
    x = torch.zeros(336, 3, 224, 224, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="split the batch"):
        m.forward(x)
    _, _, logits = m.forward(x[:330])
    assert bool(torch.isfinite(logits).all()) and torch.equal(logits[0], logits[329])
    m.close()


def test_bf16_u8_input_goes_through_the_fused_first_layer(weights3):
    # the bf16 first layer converts u8 frames itself (ToTensor + Normalize in the kernel): same scores as the bf16 model fed
    # the normalised floats, up to bf16 roundings of inputs that differ in their last float bit
    from oracle import vgg_oracle
    from video_analytics_amd import synth, vgg
    from video_analytics_amd.parameters import NORM_MEANS_TF, NORM_STDS_TF
    w = weights3
    rgb, _, _ = synth.synth_clips(3, seed=5)
    xr = vgg_oracle.normalize_u8(rgb, NORM_MEANS_TF, NORM_STDS_TF)
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, NORM_MEANS_TF, NORM_STDS_TF, dtype="bf16")
    _, _, log_u8 = m.forward(rgb.cuda())
    _, _, log_f = m.forward(xr.cuda())
    ls = float(log_f.abs().max())
    assert float((log_u8 - log_f).abs().max()) / ls < 1e-2
    m.close()


def test_batch_40_crosses_fc_row_tile(weights3):
    # 40 > 32: two FC row tiles and a partial conv batch brick; compare rows 0..2 and 37..39 with the oracle
    from oracle import vgg_oracle
    from video_analytics_amd import vgg
    w = weights3
    x = _inputs(40, 3, seed=8)
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    _, desc, logits = m.forward(x.cuda())
    idx = [0, 1, 2, 37, 38, 39]
    _, desc_r, log_r = vgg_oracle.forward(x[idx], w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"])
    assert float((logits.cpu()[idx] - log_r).abs().max()) < TOL
    assert float((desc.cpu()[idx] - desc_r).abs().max()) < TOL
    m.close()


@pytest.mark.parametrize("c_in", [3, 20])
def test_benchmark_batch_32_matches_oracle_on_every_row(weights3, c_in):
    """BASELINE configs[1]'s batch (32 clips per GPU): every row of both streams against the torch-CPU oracle
    (the tile/brick choice of the conv kernels and the FC row tiling depend on the batch)."""
    from oracle import vgg_oracle
    from video_analytics_amd import vgg
    torch.set_num_threads(8)
    w = {k: [t.clone() for t in v] for k, v in weights3.items()}
    if c_in != 3:
        w["conv_w"][0] = vgg_oracle.copy_first_layer(w["conv_w"][0], c_in)
    x = _inputs(32, c_in, seed=40 + c_in)
    feat_r, desc_r, log_r = vgg_oracle.forward(x, w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"])
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    feat, desc, logits = m.forward(x.cuda(), want_feat=True)
    assert float((feat.cpu() - feat_r).abs().max()) < TOL
    assert float((desc.cpu() - desc_r).abs().max()) < TOL
    assert float((logits.cpu() - log_r).abs().max()) < TOL
    assert torch.equal(logits.cpu().argmax(1), log_r.argmax(1))
    m.close()


def test_reference_classifier_traversal_runs_verbatim(weights3):
    """The body of the reference's validate() forward (Sheet03/spatialModel.py:212-218), verbatim, over the mirror's
    ``features`` / ``classifierList`` / ``classifierLen``: equal to forward() bit for bit."""
    from video_analytics_amd.spatialModel import SpatialNetwork
    w = {k: [t.clone() for t in v] for k, v in weights3.items()}
    self = SpatialNetwork(101, 1, 0.1, 0.9, 256, None, None, [10, 20], None, gpu=True, weights=w)
    ip = _inputs(3, 3, seed=19).cuda()
    op = self.features(ip)
    op = op.view(op.size(0), -1)
    for cl in self.classifierList[:(self.classifierLen - 1)]:  # evaluate till second last layer
        op = cl(op)
    featureVectors = op  # keep the second last layer's output as the feature vector
    for cl in self.classifierList[(self.classifierLen - 1):]:  # continue till last layer
        op = cl(op)
    _, desc, logits = self.model.forward(ip)
    assert torch.equal(featureVectors, desc) and torch.equal(op, logits)
    assert self.classifierLen == 10
    with pytest.raises(ValueError):
        self.classifierList[9](desc)  # not the tensor stage 8 handed out
    with pytest.raises(ValueError):
        self.classifierList[3](ip)
    self.model.close()


def test_bf16_stream_tracks_the_fp32_stream(weights3):
    """BASELINE config 5 (bf16 conv stack, fp32 accumulate/classifier): not a parity configuration -- the
    test states its deviation from the fp32 oracle: relative error of the class scores below 3e-2 of their
    range, identical arg-max on these inputs, and batch-composition independence."""
    from oracle import vgg_oracle
    from video_analytics_amd import vgg
    w = weights3
    x = _inputs(5, 3, seed=5)
    _, desc_r, log_r = vgg_oracle.forward(x, w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"])
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, dtype="bf16")
    feat, desc, logits = m.forward(x.cuda(), want_feat=True)
    scale = float(log_r.abs().max())
    err = float((logits.cpu() - log_r).abs().max())
    assert err / scale < 3e-2, (err, scale)
    assert err > 1e-4  # it really is the bf16 path
    assert torch.equal(logits.cpu().argmax(1), log_r.argmax(1))
    _, _, one = m.forward(x[3:4].cuda())
    assert torch.equal(one[0], logits[3])
    m.close()


@pytest.mark.parametrize("c_in,B", [(3, 5), (20, 3), (3, 33)])
def test_bf16_stream_against_its_own_restatement_and_across_staging_schemes(weights3, c_in, B):
    """(1) The bf16 path against its restatement (bf16-rounded operands, fp32 accumulation,
    oracle.vgg_oracle.forward_bf16): two valid bf16 evaluations that differ only in the fp32 accumulation
    order decorrelate their bf16 rounding decisions layer by layer, so they agree to the bf16 noise level
    (stated: 1e-2 of the range), not better.  (2) What IS exact: the three tile/staging schemes of the kernel
    (automatic; 64-channel tiles + single LDS buffer; 3-deep DMA ring on every layer) run the same MFMA
    sequence per output element and must agree bit for bit, run to run -- a staging race shows up here.
    B = 33 crosses a batch brick; c_in = 20 is the temporal first layer."""
    from oracle import vgg_oracle
    from video_analytics_amd import vgg
    w = {k: [t.clone() for t in v] for k, v in weights3.items()}
    if c_in != 3:
        w["conv_w"][0] = vgg_oracle.copy_first_layer(w["conv_w"][0], c_in)
    x = _inputs(B, c_in, seed=11 + c_in)
    feat_r, desc_r, log_r = vgg_oracle.forward_bf16(x, w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"])
    outs = []
    from video_analytics_amd import _ffi
    # Two groups of schemes, each adding the same products in the same order per accumulator, so bit-equal inside a group:
    # (0, 5, 7) -- the automatic choice, the two-group kernel, the weights-resident kernel -- run the 14 x 14 layers on the
    # one-image-per-workgroup kernel (round 3: chunk-major K order there); (1, 2) keep the tap-major kernel on every layer.
    # Between the groups: the bf16 noise level, like any two valid bf16 evaluations.
    variants = (0, 5, 7, 1, 2)
    for variant in variants:
        m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, dtype="bf16")
        m.set_option(_ffi.VA_OPT_BF16_VARIANT, variant)
        feat, desc, logits = m.forward(x.cuda(), want_feat=True)
        feat2, _, logits2 = m.forward(x.cuda(), want_feat=True)
        assert torch.equal(feat, feat2) and torch.equal(logits, logits2)
        outs.append((feat.cpu(), logits.cpu()))
        m.close()
    for k in (1, 2):
        assert torch.equal(outs[k][0], outs[0][0]) and torch.equal(outs[k][1], outs[0][1]), variants[k]
    assert torch.equal(outs[4][0], outs[3][0]) and torch.equal(outs[4][1], outs[3][1])
    fs, ls = float(feat_r.abs().max()), float(log_r.abs().max())
    for k in (0, 3):
        ef, el = float((outs[k][0] - feat_r).abs().max()), float((outs[k][1] - log_r).abs().max())
        assert ef / fs < 1e-2 and el / ls < 1e-2, (variants[k], ef, fs, el, ls)
    assert float((outs[3][1] - outs[0][1]).abs().max()) / ls < 1e-2
    # variant 6 (the two-group kernel on halo bricks, retired) is refused
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, dtype="bf16")
    with pytest.raises(ValueError):
        m.set_option(_ffi.VA_OPT_BF16_VARIANT, 6)
    m.close()
    # the first layer: by default it reads the NCHW input itself (k_conv1_fused_bf16); VA_OPT_BF16_FIRST_LAYER = 0 is the
    # staged path (input conversion + three K steps) -- for 3 channels another grouping of the sum, the same bf16 noise level
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, dtype="bf16")
    m.set_option(_ffi.VA_OPT_BF16_FIRST_LAYER, 0)
    feat, desc, logits = m.forward(x.cuda(), want_feat=True)
    ef, el = float((feat.cpu() - feat_r).abs().max()), float((logits.cpu() - log_r).abs().max())
    assert ef / fs < 1e-2 and el / ls < 1e-2, ("staged first layer", ef, fs, el, ls)
    assert float((logits.cpu() - outs[0][1]).abs().max()) / ls < 1e-2
    if c_in % 4 == 0:  # (no channel padding in the patch: the same products in the same order, so even bit-equal)
        assert torch.equal(feat.cpu(), outs[0][0])
    m.close()


def test_validate_batch_matches_oracle():
    from oracle import vgg_oracle
    from video_analytics_amd import vgg
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(37, 101, generator=g) * 3
    labels = torch.randint(1, 26, (37,), generator=g)
    logits[5, 7] = logits[5, 9] = logits[5].max() + 1  # tie: first max wins
    loss_r, corr_r = vgg_oracle.validate_batch(logits, labels)
    out = vgg.validate_batch(logits.cuda(), labels.cuda()).cpu()
    assert abs(float(out[0]) - float(loss_r)) < 1e-4
    assert int(out[1]) == corr_r


def test_bad_shapes_raise_value_error(weights3):
    from video_analytics_amd import vgg
    w = weights3
    with pytest.raises(ValueError):
        vgg.Vgg16Stream(w["conv_w"][:12], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    with pytest.raises(ValueError):
        m.forward(torch.zeros(1, 3, 200, 200, device="cuda"))
    with pytest.raises(ValueError):
        m.forward(torch.zeros(1, 3, 224, 224))
    with pytest.raises(ValueError):
        m.forward(torch.zeros(1, 3, 224, 224, dtype=torch.uint8, device="cuda"))  # no mean/std given
    m.close()


@pytest.mark.parametrize("c_in,seed,f32_conv", [pytest.param(3, 1, 1, id="3-1"), pytest.param(20, 2, 1, id="20-2"),
                                                pytest.param(3, 1, 0, id="3-1-f32conv0"),
                                                pytest.param(20, 2, 0, id="20-2-f32conv0")])
def test_fp32_stream_against_an_independent_gpu_implementation(c_in, seed, f32_conv):
    """A second, independent fp32 evaluation of the same network ON THE GPU -- torch's own ``conv2d`` / ``max_pool2d`` /
    ``linear`` (MIOpen / rocBLAS kernels: nothing of this library) -- as a witness beside the torch-CPU oracle: the HIP
    stream, the CPU oracle and the vendor kernels agree within the 1e-3 of the north star on every class score of a
    9-clip batch (checker only: SURVEY.md section 7 allows MIOpen as an optional cross-check in tests, never on the
    measured path).  f32_conv = 0: VA_OPT_F32_CONV_KERNEL = 0, the register-staged kernel on every layer."""
    import torch.nn.functional as F
    from oracle import vgg_oracle
    from video_analytics_amd import _ffi, synth, vgg
    w = synth.synth_vgg16_weights(c_in=c_in, seed=seed)
    if c_in != 3:
        w["conv_w"][0] = vgg_oracle.copy_first_layer(w["conv_w"][0], c_in)
    x = _inputs(9, c_in, seed=40 + c_in)
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    m.set_option(_ffi.VA_OPT_F32_CONV_KERNEL, f32_conv)
    feat, desc, logits = m.forward(x.cuda(), want_feat=True)
    with torch.no_grad():
        op, i = x.cuda(), 0
        for v in vgg_oracle.VGG16_CFG:
            if v == "M":
                op = F.max_pool2d(op, 2, 2)
            else:
                op = F.relu(F.conv2d(op, w["conv_w"][i].cuda(), w["conv_b"][i].cuda(), padding=1))
                i += 1
        feat_g = op
        op = op.reshape(op.size(0), -1)
        for k in range(3):
            op = F.relu(F.linear(op, w["fc_w"][k].cuda(), w["fc_b"][k].cuda()))
        desc_g, logits_g = op, F.linear(op, w["fc_w"][3].cuda(), w["fc_b"][3].cuda())
    _, desc_r, log_r = vgg_oracle.forward(x, w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"])
    assert float((logits - logits_g).abs().max()) < TOL and float((desc - desc_g).abs().max()) < TOL
    assert float((feat - feat_g).abs().max()) < TOL * max(1.0, float(feat_g.abs().max()))
    assert float((logits_g.cpu() - log_r).abs().max()) < TOL  # (and the two witnesses agree with each other)
    assert float(log_r.abs().max()) > 1.0
    m.close()


@pytest.mark.parametrize("n_classes,desc_dim", [(1, 16), (129, 16), (4096, 16), (1, 4096), (129, 4096), (4096, 4096)])
def test_classifier_at_other_shapes_against_float64(n_classes, desc_dim):
    """``va_vgg16_classify`` on random features at batches 1, 31, 33, 65 (the 32-row M tiles of k_fc_splitk and their ragged
    ends) and at class / descriptor counts that leave a ragged 128-column N tile (1, 129) or fill it (16 -> one tile,
    4096), against the float64 linear chain.  Error bound: the fp32 rule of tests/test_conv_layers_gpu.py,
    |got - ref| < C_F32 2^-24 S: for the descriptor with the magnitude sums of the chain S_k = |W_k| S_(k-1) + |b_k|,
    S_0 = |feat| (an error of an earlier layer reaches the later ones through |W_k|; ReLU does not enlarge it); for the
    class scores layer by layer, against the last Linear applied in float64 to the descriptor the kernels returned
    (measured: r <= 2e-4 on the descriptor, <= 1e-5 on the scores)."""
    from test_conv_layers_gpu import C_F32, U
    from video_analytics_amd import synth, vgg
    w = synth.synth_vgg16_weights(c_in=3, n_classes=n_classes, desc_dim=desc_dim, seed=9, device="cuda")
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], n_classes, desc_dim)
    g = torch.Generator(device="cuda").manual_seed(n_classes + desc_dim)
    W = [t.double() for t in w["fc_w"]]
    Bs = [t.double() for t in w["fc_b"]]
    for B in (1, 31, 33, 65):
        feat = torch.randn(B, 512, 7, 7, device="cuda", generator=g)
        desc, logits = m.classify(feat)
        h, s = feat.double().reshape(B, -1), feat.double().abs().reshape(B, -1)  # CHW-major flatten order
        for k in range(4):
            h = torch.nn.functional.linear(h, W[k], Bs[k])
            s = torch.nn.functional.linear(s, W[k].abs(), Bs[k].abs())
            if k < 3:
                h = h.clamp_min(0.0)
            if k == 2:
                desc_r, s_desc = h, s
        d = desc.double()
        log_r = torch.nn.functional.linear(d, W[3], Bs[3])
        s_log = torch.nn.functional.linear(d.abs(), W[3].abs(), Bs[3].abs())
        for got, ref, sk, what in ((desc, desc_r, s_desc, "desc"), (logits, h, s, "logits (chain)"),
                                   (logits, log_r, s_log, "logits")):
            r = float(((got.double() - ref).abs() / (U * sk)).max())
            print("classifier %d classes, desc %d, batch %d: %s normalised error %.3g" % (n_classes, desc_dim, B, what, r))
            assert r < C_F32, (what, B, r)
        assert float(h.abs().max()) > 0.0
    m.close()
