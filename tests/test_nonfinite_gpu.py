"""NaN and infinity through the CNN body: every conv instantiation, the training max-pool, the classifier, whole streams
and the training step.

The rule (numerics of the CNN): NaN and +-inf pass through conv, ReLU, 2x2 max-pool and FC as under IEEE
arithmetic and as in torch (``relu``, ``clamp_min``, ``amax`` and ``max_pool2d`` keep a NaN); positions a ReLU mask zeroes
are 0 whatever the value (``torch.where``).  ReLU and the 2x2 max used to be ``fmaxf``, which answers its OTHER operand for
a NaN: a NaN activation became 0 one layer later, a diverged checkpoint gave finite class scores and a NaN batch a finite
training loss.  They are IEEE ``maximum`` now (``relu_keep_nan`` / ``max_keep_nan`` in csrc/vgg.hip, k_maxpool in
csrc/train.hip); every test below that plants a NaN fails with ``fmaxf`` in the epilogue it reaches.

Per conv case (``test_conv_layer_keeps_nan_and_infinity``): one clean launch, then three planted launches on the same
inputs -- NaN pixels, +-inf pixels, a NaN bias and a NaN weight.  A = the outputs whose float64 reference
(``reference_layer`` of test_conv_layers_gpu.py) changed or is not finite.  Outside A the output is bit-identical to the
clean launch; inside A every element is in the reference's class {finite, -inf, +inf, NaN}, and where that is finite the
fp32 / bf16 error rule of test_conv_layers_gpu.py holds with the clean run's magnitude sum (ReLU of -inf is exactly 0).
No kernel reached through ``va_conv3x3_layer`` has a wider NaN reach than the reference: their K dimension is never padded
with neighbouring data (the fused first layer's is: tests/test_first_layer_gpu.py pins that reach).
"""
import math

import pytest
import torch

from test_conv_layers_gpu import CASES, INSTANTIATIONS, _check_against_reference, _make_inputs, _run, reference_layer

NAN, INF = float("nan"), float("inf")


def classes(t):
    """0 finite, 1 -inf, 2 +inf, 3 NaN, per element."""
    c = torch.zeros(t.shape, dtype=torch.int8, device=t.device)
    c[t == -INF] = 1
    c[t == INF] = 2
    c[t.isnan()] = 3
    return c


def _bits(t):
    return t.contiguous().view(torch.uint8)


# ------------------------------------------------------------------------------------------- the reference (CPU) ----

PLANTS = ("nan_pixel", "+inf_pixel", "-inf_pixel", "nan_weight", "nan_bias")


def test_reference_layer_has_torchs_nonfinite_classes():
    """CPU: ``reference_layer`` puts every output into the class float64 F.conv2d -> F.relu -> F.max_pool2d puts it, for a
    NaN / +inf / -inf pixel, one NaN weight (one tap, one input channel) and one NaN bias, with and without pool and
    ``linear``.  With a mask, masked positions are 0 even where the value is NaN (``torch.where``: the kernels' rule; a
    product with the 0 / 1 mask would keep the NaN); the unmasked positions keep torch's class."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(11)
    B, hw, cin, cout = 2, 8, 5, 6
    x0 = torch.randn(B, hw, hw, cin, generator=g, dtype=torch.float64)
    w0 = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    b0 = torch.randn(cout, generator=g, dtype=torch.float64)
    m = torch.randn(B, hw, hw, cout, generator=g, dtype=torch.float64)
    combos = 0
    for plant in PLANTS:
        x, w, b = x0.clone(), w0.clone(), b0.clone()
        if plant.endswith("pixel"):
            x[1, 3, 4, 2] = {"nan": NAN, "+inf": INF, "-inf": -INF}[plant.split("_")[0]]
        elif plant == "nan_weight":
            w[4, 1, 0, 2] = NAN  # (a border tap: it meets the zero padding, and 0 x NaN is NaN in conv2d and in the helper)
        else:
            b[2] = NAN
        wp = w.permute(0, 2, 3, 1).reshape(cout, 9, cin)
        conv = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1)
        for pool in (False, True):
            for linear in (False, True):
                want = conv if linear else F.relu(conv)
                if pool:
                    want = F.max_pool2d(want, 2)
                got, _, _ = reference_layer(x, wp, b, pool, linear)
                cw = classes(want.permute(0, 2, 3, 1))
                assert torch.equal(classes(got), cw), (plant, pool, linear)
                assert int((cw != 0).sum()) > 0, (plant, pool, linear)  # (ReLU turns -inf into 0: the -inf pixel still leaves +inf)
                combos += 1
        for linear in (False, True):
            want = (conv if linear else F.relu(conv)).permute(0, 2, 3, 1)
            got, _, _ = reference_layer(x, wp, b, False, linear, m)
            assert bool((got[m <= 0] == 0).all()) and bool((classes(want)[m <= 0] != 0).any()), (plant, linear)
            assert not plant.startswith("nan") or bool(want[m <= 0].isnan().any()), (plant, linear)
            assert torch.equal(classes(got)[m > 0], classes(want)[m > 0]), (plant, linear)
    assert combos == 20


# --------------------------------------------------------------------------------------- every conv instantiation ----

def _smallest_case(name):
    """(case id, kernel_opt) of the case with the fewest multiply-adds whose ``runs`` reach the instantiation."""
    best = None
    for cid, c in sorted(CASES.items()):
        for opt, reached in c["runs"]:
            if reached == name:
                cost = c["B"] * c["hw"] ** 2 * c["cin"] * c["cout"]
                if best is None or cost < best[0]:
                    best = (cost, cid, opt)
    assert best is not None, name
    return best[1], best[2]


def test_every_instantiation_has_a_smallest_case():
    """CPU: the choice below reaches all 29 instantiations, and its pixel plants stay apart (see ``_sites``)."""
    picked = {name: _smallest_case(name) for name in INSTANTIATIONS}
    assert len(picked) == 29
    for name, (cid, _) in picked.items():
        _sites(CASES[cid])


def _sites(case):
    """Pixel sites (image, y, x, channel): three NaNs -- pixel (0, 0) of image 0, the last pixel of the last image (ragged
    brick, ragged batch), an interior pixel of a middle image -- and two infinities at interior pixels, +inf and -inf.
    Sites that share an image are at least 3 pixels apart: their 3 x 3 neighbourhoods do not touch."""
    B, hw, cin = case["B"], case["hw"], case["cin"]
    q = max(1, hw // 4)
    nans = [(0, 0, 0, 0), (B - 1, hw - 1, hw - 1, cin - 1), (B // 2, hw // 2, hw // 2, cin // 2)]
    infs = [(0, q, q, 1, INF), (B - 1, hw - 1 - q, hw - 1 - q, cin - 2, -INF)]
    for group in (nans, infs):
        for i, s in enumerate(group):
            for t in group[:i]:
                assert s[0] != t[0] or max(abs(s[1] - t[1]), abs(s[2] - t[2])) >= 3, (case, s, t)
    for s in infs + nans[2:]:
        assert 1 <= s[1] <= hw - 2 and 1 <= s[2] <= hw - 2, (case, s)  # interior
    return nans, infs


def _planted(inp, x=None, w=None, b=None):
    """A copy of the inputs with x (inside a copy of its guarded buffer), w or b replaced."""
    out = dict(inp)
    if x is not None:
        gi, n = inp["gi"], x.numel()
        out["in_buf"] = inp["in_buf"].clone()
        out["xin"] = out["in_buf"][gi:gi + n].view(x.shape)
        out["xin"].copy_(x)
        out["x"] = x
    if w is not None:
        out["w"] = w
    if b is not None:
        out["b"] = b
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", INSTANTIATIONS)
def test_conv_layer_keeps_nan_and_infinity(name):
    cid, opt = _smallest_case(name)
    case = CASES[cid]
    inp = _make_inputs(case, seed=sum(map(ord, cid)) + 1)
    zeros = torch.zeros(64, dtype=torch.float32, device="cuda")
    nans, infs = _sites(case)
    ref_c, _, s_c = reference_layer(inp["x"], inp["w"], inp["b"], case["pool"], case["linear"], inp["mask"])
    launched, clean = _run(case, inp, opt, zeros)
    assert launched == name, (cid, opt, launched)

    xn, xi = inp["x"].clone(), inp["x"].clone()
    for (i, y, x, c) in nans:
        xn[i, y, x, c] = NAN
    for (i, y, x, c, v) in infs:
        xi[i, y, x, c] = v
    wn, bn = inp["w"].clone(), inp["b"].clone()
    bn[0] = NAN
    wn[case["cout"] - 1, 0, case["cin"] // 2] = NAN  # (tap 0: at the top and left borders it meets the zero padding)
    plants = (("nan pixels", _planted(inp, x=xn), True), ("inf pixels", _planted(inp, x=xi), True),
              ("nan bias and weight", _planted(inp, w=wn, b=bn), False))
    for what, pin, is_pixel in plants:
        label = (cid, name, what)
        ref, pre, _ = reference_layer(pin["x"], pin["w"], pin["b"], case["pool"], case["linear"], pin["mask"])
        launched, got = _run(case, pin, opt, zeros, finite=False)
        assert launched == name, label
        A = (ref != ref_c) | ~torch.isfinite(ref)
        frac = float(A.double().mean())
        print("%s / %s: A covers %.1f %% of the outputs" % (cid, what, 100.0 * frac))
        assert frac > 0.0, label
        if is_pixel:  # a condition on the test, not on the kernel: the "outside" half never shrinks to nothing
            assert frac <= 0.25, (label, frac)
        else:         # channel 0 (bias) and the last channel (weight), wherever no mask zeroes them
            expect = torch.zeros_like(A)
            expect[..., 0] = expect[..., -1] = True
            if pin["mask"] is not None:
                expect &= pin["mask"] > 0
            assert torch.equal(A, expect) and bool(ref[A].isnan().all()), label
        same = (_bits(got) == _bits(clean)).view(*got.shape, -1).all(dim=-1)
        assert bool(same[~A].all()), (label, "changed outside the reference's reach", torch.nonzero(~same & ~A)[:8].tolist())
        cg, cr = classes(got), classes(ref)
        bad = A & (cg != cr)
        assert not bool(bad.any()), (label, "class differs from the float64 reference's", int(bad.sum()),
                                     [(idx, int(cg[tuple(idx)]), int(cr[tuple(idx)])) for idx in torch.nonzero(bad)[:8].tolist()])
        fin = A & (cr == 0)
        if bool(fin.any()):  # e.g. ReLU of -inf and the pooling windows around it: the usual bound, clean magnitudes
            _check_against_reference(case, got[fin], ref[fin], pre[fin], s_c[fin], label)
        if what == "nan pixels":
            assert bool(got.isnan().any()), label
        if what == "inf pixels":
            assert bool(got.isinf().any()), label
            assert not case["linear"] or bool((got == -INF).any()), label


# --------------------------------------------------------------------------------------------- training max-pool ----

@pytest.mark.gpu
@pytest.mark.parametrize("H", [2, 14])
def test_train_pool_layer_keeps_a_nan(H):
    """``va_train_pool_layer``: a NaN in one element of a window (each of the four positions in turn) gives a NaN p for that
    window and channel; every other p is bit-equal to the clean run.  (dy is not looked at: the loss is NaN by then.)"""
    from test_train_kernels_gpu import _Box, _Inputs
    from video_analytics_amd import vgg
    g = torch.Generator().manual_seed(3 + H)
    B, C = 3, 68
    y = torch.randn(B, H, H, C, generator=g).clamp_min(0.0)
    dp = torch.randn(B, H // 2, H // 2, C, generator=g)

    def run(yy, what):
        In = _Inputs(y=yy, dp=dp)
        p, dy = _Box((B, H // 2, H // 2, C)), _Box((B, H, H, C))
        vgg.train_pool_layer(In.y, p.t, In.dp, dy.t)
        torch.cuda.synchronize()
        In.check(what)
        p.check(what + ("p",), finite=False)
        dy.check(what + ("dy",), finite=False)
        p2 = _Box((B, H // 2, H // 2, C))
        vgg.train_pool_layer(In.y, p2.t)  # the forward alone
        torch.cuda.synchronize()
        p2.check(what + ("p alone",), finite=False)
        assert torch.equal(_bits(p.t), _bits(p2.t)), what
        return p.t.clone()

    clean = run(y, ("pool", H, "clean"))
    assert bool(torch.isfinite(clean).all())
    wy, wx = H // 2 - 1, (H // 2) // 2  # a window in the last row of windows
    for k, (dy_, dx_) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        b, c = k % B, (17 * k + 5) % C
        yn = y.clone()
        yn[b, 2 * wy + dy_, 2 * wx + dx_, c] = NAN
        got = run(yn, ("pool", H, k))
        assert bool(got[b, wy, wx, c].isnan()), (H, k, "the NaN was dropped")
        same = _bits(got).view(-1, 4) == _bits(clean).view(-1, 4)
        hit = torch.zeros_like(clean, dtype=torch.bool)
        hit[b, wy, wx, c] = True
        assert bool(same.all(dim=1)[~hit.view(-1)].all()), (H, k)


# ------------------------------------------------------------------------------------------------ the classifier ----

def _float64_chain(w, feat):
    """The float64 linear chain of test_classifier_at_other_shapes_against_float64: (descriptor, logits)."""
    h = feat.double().reshape(feat.shape[0], -1)
    for k in range(4):
        h = torch.nn.functional.linear(h, w["fc_w"][k].double(), w["fc_b"][k].double())
        if k < 3:
            h = h.clamp_min(0.0)
        if k == 2:
            desc = h
    return desc, h


@pytest.mark.gpu
def test_classifier_keeps_nan_rows_and_a_nan_bias():
    """``va_vgg16_classify`` at batches 3 and 33 (33 crosses the 32-row tile of k_fc_splitk), 129 classes, descriptor 16.
    A NaN in one feature of row 1 (and of row 32) makes that row's descriptor and logits NaN, every other row is bit-equal
    to the clean call.  A NaN in one fc7 bias (the second Linear) or in one bias of the descriptor layer (the third): NaN in
    the descriptor and the logits exactly where the float64 chain has it -- the whole descriptor, or one column of it --
    and in every logit."""
    from video_analytics_amd import synth, vgg
    n_classes, desc_dim = 129, 16
    w = synth.synth_vgg16_weights(c_in=3, n_classes=n_classes, desc_dim=desc_dim, seed=9, device="cuda")
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], n_classes, desc_dim)
    g = torch.Generator(device="cuda").manual_seed(21)
    feats = {}
    for B in (3, 33):
        feat = feats[B] = torch.randn(B, 512, 7, 7, device="cuda", generator=g)
        desc, logits = m.classify(feat)
        desc, logits = desc.clone(), logits.clone()
        assert bool(torch.isfinite(desc).all()) and bool(torch.isfinite(logits).all()) and float(desc.abs().max()) > 0
        rows = [1] + ([32] if B == 33 else [])
        fn = feat.clone()
        for r in rows:
            fn[r, 100 + r, 3, 4] = NAN
        dn, ln = m.classify(fn)
        keep = torch.ones(B, dtype=torch.bool, device="cuda")
        keep[rows] = False
        assert bool(dn[rows].isnan().all()) and bool(ln[rows].isnan().all()), (B, "a NaN feature left finite outputs in its row")
        assert torch.equal(_bits(dn[keep]), _bits(desc[keep])) and torch.equal(_bits(ln[keep]), _bits(logits[keep])), B
    m.close()
    for layer, idx in ((1, 7), (2, 3)):
        wb = dict(w)
        wb["fc_b"] = [t.clone() for t in w["fc_b"]]
        wb["fc_b"][layer][idx] = NAN
        m = vgg.Vgg16Stream(wb["conv_w"], wb["conv_b"], wb["fc_w"], wb["fc_b"], n_classes, desc_dim)
        for B in (3, 33):
            desc, logits = m.classify(feats[B])
            desc_r, log_r = _float64_chain(wb, feats[B])
            assert torch.equal(classes(desc), classes(desc_r)) and torch.equal(classes(logits), classes(log_r)), (layer, B)
            assert bool(log_r.isnan().all()), (layer, B)
            if layer == 2:  # one column of the descriptor
                col = torch.zeros(desc_dim, dtype=torch.bool, device="cuda")
                col[idx] = True
                assert torch.equal(desc_r.isnan(), col[None, :].expand(B, -1)), B
            else:
                assert bool(desc_r.isnan().all()), B
        m.close()


# ------------------------------------------------------------------------------------------------- whole streams ----

def _offset_copy(x, shift):
    """x on the device, ``shift`` elements past a 16-byte boundary."""
    buf = torch.empty(x.numel() + 16, dtype=x.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == (shift * x.element_size()) % 16 and v.is_contiguous()
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("c_in", [3, 20])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stream_forward_keeps_a_nan_pixel_and_a_nan_weight(dtype, c_in):
    """``Vgg16Stream.forward`` at batch 3, float32 input.  One NaN pixel in image 1: row 1 of the descriptor and of the
    logits is all NaN, rows 0 and 2 are bit-equal to the clean call -- with the input 16-byte aligned and 4 bytes past
    alignment (bf16: the fused first layer and the staged path; they used to disagree, NaN against zeros).  One NaN weight
    in conv3_1: every row is NaN."""
    from oracle import vgg_oracle
    from video_analytics_amd import synth, vgg
    w = synth.synth_vgg16_weights(c_in=3, seed=6, device="cuda")
    if c_in != 3:
        w["conv_w"][0] = vgg_oracle.copy_first_layer(w["conv_w"][0].cpu(), c_in).cuda()
    x = torch.from_numpy(synth.hash_uniform(90 + c_in, 1, 3 * c_in * 224 * 224).reshape(3, c_in, 224, 224)) * 4.0 - 2.0
    xn = x.clone()
    xn[1, c_in - 1, 117, 59] = NAN
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, dtype=dtype)
    for shift in (0, 1):
        _, desc, logits = m.forward(_offset_copy(x, shift))
        desc, logits = desc.clone(), logits.clone()
        assert bool(torch.isfinite(desc).all()) and bool(torch.isfinite(logits).all()) and float(desc.abs().max()) > 0
        _, dn, ln = m.forward(_offset_copy(xn, shift))
        assert bool(dn[1].isnan().all()) and bool(ln[1].isnan().all()), (dtype, c_in, shift, "the NaN pixel was lost on the way")
        for r in (0, 2):
            assert torch.equal(_bits(dn[r]), _bits(desc[r])) and torch.equal(_bits(ln[r]), _bits(logits[r])), (dtype, c_in, shift, r)
    m.close()
    cw = [t.clone() for t in w["conv_w"]]
    cw[4][200, 77, 1, 2] = NAN  # conv3_1: 128 -> 256 channels
    m = vgg.Vgg16Stream(cw, w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, dtype=dtype)
    _, dn, ln = m.forward(x.cuda())
    assert bool(dn.isnan().all()) and bool(ln.isnan().all()), (dtype, c_in, "a NaN weight left finite outputs")
    m.close()


# ------------------------------------------------------------------------------------------------------ training ----

@pytest.fixture(scope="module")
def nan_batch():
    """Weights, a batch of two images with one NaN pixel, labels, and the autograd oracle's loss for it (computed once)."""
    from oracle import train_oracle
    from video_analytics_amd import synth
    torch.set_num_threads(8)
    w = synth.synth_vgg16_weights(c_in=3, seed=4)
    x = torch.from_numpy(synth.hash_uniform(75, 3, 2 * 3 * 224 * 224).reshape(2, 3, 224, 224)) * 4.0 - 2.0
    x[1, 2, 30, 200] = NAN
    labels = torch.tensor([8, 8], dtype=torch.int64)
    loss_r, _, _, _ = train_oracle.TrainOracle(w, 1e-4, 0.9).step(x, labels, seed=1000)
    return w, x, labels, loss_r


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["train_step", "train_step_consensus"])
def test_training_step_reports_a_nan_loss(form, nan_batch):
    """One NaN pixel in the batch: ``train_step`` and ``train_step_consensus`` (one video of two snippets) report a NaN
    loss, as torch.optim.SGD's user sees with the reference model (oracle/train_oracle.py: autograd on the same batch).
    Nothing is asserted about the parameters afterwards."""
    from video_analytics_amd import vgg
    w, x, labels, loss_r = nan_batch
    assert math.isnan(loss_r)
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    if form == "train_step":
        stats, _ = m.train_step(x.cuda(), labels.cuda(), 1e-4, 0.9, 1000)
    else:
        stats, _ = m.train_step_consensus(x.cuda(), labels[:1].cuda(), 2, 1e-4, 0.9, 1000)
    assert math.isnan(float(stats.cpu()[0])), (form, float(stats.cpu()[0]))
    m.close()
