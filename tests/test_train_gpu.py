"""Training step against torch autograd + torch.optim.SGD on the CPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# Update of a tensor vs the oracle's, relative to the largest update in that tensor.  Not tighter because backward
# passes through DECISIONS of the forward pass: the max-pool gradient goes to the arg-max of each window and the ReLU
# gradient to the positive elements, and a few elements per 100 000 sit closer to such a decision than the fp32
# difference between the two forward passes (measured here: 2 of 100 352 windows of conv4_3 pick another position in
# the first case, 1 of 154 420 elements of conv5_2 flips its ReLU mask in the second; everywhere else the
# gradients agree to 2e-5): every layer below such a flip inherits a ~2e-3..7e-3 relative difference.
TOL_UPDATE = 1e-2


def _relerr(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


# A flipped decision perturbs EVERY gradient below it by about the same relative amount (measured: max and RMS error
# both 2e-3..4e-3 on conv layers 0..9, 2e-5 on layers 10..12 above the first flip), so TOL_UPDATE cannot tell a flip
# from a genuine gradient bug of that size.  test_conv_updates_under_the_products_own_decisions removes the
# ambiguity: the oracle back-propagates through the decisions the HIP forward pass actually took, and every update
# must then agree to TOL_UPDATE_DECIDED.
TOL_UPDATE_DECIDED = 5e-4


def _rmserr(a, b):
    return float((a - b).double().pow(2).mean().sqrt()) / max(float(b.double().pow(2).mean().sqrt()), 1e-30)


@pytest.mark.parametrize("c_in,B", [(3, 2), (20, 3)])
def test_two_sgd_steps_match_autograd(c_in, B):
    """Two steps (the second one, restarted from the oracle's state, exercises the momentum buffers): loss, hits,
    train-mode descriptors, every parameter and every momentum buffer against the oracle.  The update of a
    tensor is compared relative to the largest update in that tensor."""
    from oracle import train_oracle, vgg_oracle
    from video_analytics_amd import synth, vgg
    torch.set_num_threads(8)
    w = synth.synth_vgg16_weights(c_in=3, seed=4)
    if c_in != 3:
        w["conv_w"][0] = vgg_oracle.copy_first_layer(w["conv_w"][0], c_in)
    lr, mu = 1e-4, 0.9  # small enough that the random-init network does not blow up in the second step
    ora = train_oracle.TrainOracle(w, lr, mu)
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    w0 = {k: [t.clone() for t in v] for k, v in w.items()}
    for step in range(2):
        if step == 1:
            # second step from the SAME state (parameters and momentum buffers of the oracle after step 0), so that it
            # checks the momentum arithmetic and import_state rather than the divergence of two chaotic trajectories
            m.import_state(ora.weights())
            m.import_state(ora.momentum(), momentum=True)
            w0 = ora.weights()
        u = synth.hash_uniform(70 + step, c_in, B * c_in * 224 * 224).reshape(B, c_in, 224, 224)
        x = torch.from_numpy(u * 4.0 - 2.0)
        labels = torch.tensor([(7 * i + 3 * step + 1) % 101 for i in range(B)], dtype=torch.int64)
        loss_r, corr_r, desc_r, _ = ora.step(x, labels, seed=1000 + step)
        stats, desc = m.train_step(x.cuda(), labels.cuda(), lr, mu, 1000 + step)
        stats = stats.cpu()
        assert abs(float(stats[0]) - loss_r) < 2e-4 * max(1.0, abs(loss_r)), (float(stats[0]), loss_r)
        assert int(stats[1]) == corr_r
        assert _relerr(desc.cpu(), desc_r) < 1e-3
        got, ref = m.export_state(), ora.weights()
        gotm, refm = m.export_state(momentum=True), ora.momentum()
        worst, rms = [], []
        for k in ("conv_w", "conv_b", "fc_w", "fc_b"):
            for i, (g, r, o, gm, rm) in enumerate(zip(got[k], ref[k], w0[k], gotm[k], refm[k])):
                e_upd = _relerr(g.cpu() - o, r - o)
                e_mom = _relerr(gm.cpu(), rm)
                e_rms = _rmserr(g.cpu() - o, r - o)
                worst.append((max(e_upd, e_mom), step, k, i))
                rms.append((e_rms, step, k, i))
                print("step %d %-6s %2d: update err %.2e (rms %.2e)  momentum err %.2e" % (step, k, i, e_upd, e_rms, e_mom))
        assert max(worst)[0] < TOL_UPDATE, max(worst)
        assert max(rms)[0] < TOL_UPDATE, max(rms)
        tight = [e for e, _, k, i in worst if k.startswith("fc")]  # no pooling / ReLU decision below the classifier's own
        assert max(tight) < 5e-4, max(tight)
    m.close()


@pytest.mark.parametrize("c_in,B,f32_conv", [pytest.param(3, 2, 1, id="3-2"), pytest.param(20, 3, 1, id="20-3"),
                                             pytest.param(3, 2, 0, id="3-2-f32conv0")])
def test_conv_updates_under_the_products_own_decisions(c_in, B, f32_conv):
    """One SGD step where the autograd oracle uses the ReLU masks and pooling arg-maxima of the HIP forward pass
    (read from the training workspace: all 13 conv outputs stay there; va_vgg16_train_plan gives the offsets).  With
    the decisions shared, nothing but fp32 summation order separates the two backward passes: every parameter update,
    conv layers 0..9 included, must agree to TOL_UPDATE_DECIDED (max AND rms), and the decisions themselves must
    differ from the oracle's own in at most a few elements per million.  f32_conv = 0: VA_OPT_F32_CONV_KERNEL = 0 (the
    register-staged kernel in the forward pass and in every dgrad convolution)."""
    import ctypes
    from oracle import train_oracle, vgg_oracle
    from video_analytics_amd import _ffi, synth, vgg
    torch.set_num_threads(8)
    w = synth.synth_vgg16_weights(c_in=3, seed=4)
    if c_in != 3:
        w["conv_w"][0] = vgg_oracle.copy_first_layer(w["conv_w"][0], c_in)
    lr, mu = 1e-4, 0.9
    u = synth.hash_uniform(70, c_in, B * c_in * 224 * 224).reshape(B, c_in, 224, 224)
    x = torch.from_numpy(u * 4.0 - 2.0)
    labels = torch.tensor([(7 * i + 1) % 101 for i in range(B)], dtype=torch.int64)
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    m.set_option(_ffi.VA_OPT_F32_CONV_KERNEL, f32_conv)
    stats, _ = m.train_step(x.cuda(), labels.cuda(), lr, mu, 1000)
    torch.cuda.synchronize()
    off = (ctypes.c_ulonglong * 30)()
    _ffi.check(_ffi.lib().va_vgg16_train_plan(m._h, B, off))
    ws = [t for k, t in vgg._ws_cache.items() if "train" in str(k)][0]
    ys, hw = [], 224
    for i, v in enumerate([c for c in vgg_oracle.VGG16_CFG if c != "M"]):
        n = B * hw * hw * v
        y = ws[off[i]:off[i] + 4 * n].view(torch.float32).view(B, hw, hw, v).permute(0, 3, 1, 2).contiguous().cpu()
        ys.append(y)
        if off[13 + i]:
            hw //= 2
    dec = train_oracle.decisions_from_activations(ys)
    # the product's decisions against the oracle's own: a handful of near-ties, not a different function
    own = train_oracle.decisions_from_activations(
        _conv_outputs(x, w["conv_w"], w["conv_b"]))
    n_dec = sum(d["mask"].numel() for d in dec)
    n_flip = sum(int((a["mask"] != b["mask"]).sum()) for a, b in zip(dec, own))
    n_flip += sum(int((a["pool_idx"] != b["pool_idx"]).sum()) for a, b in zip(dec, own) if a["pool_idx"] is not None)
    print("decisions that differ between the HIP and the torch-CPU forward pass: %d of %d" % (n_flip, n_dec))
    assert n_flip <= max(8, n_dec // 100000), (n_flip, n_dec)
    ora = train_oracle.TrainOracle(w, lr, mu)
    loss_r, corr_r, _, _ = ora.step(x, labels, seed=1000, decisions=dec)
    assert abs(float(stats.cpu()[0]) - loss_r) < 2e-4 * max(1.0, abs(loss_r))
    got, ref = m.export_state(), ora.weights()
    worst = []
    for k in ("conv_w", "conv_b", "fc_w", "fc_b"):
        for i, (g, r, o) in enumerate(zip(got[k], ref[k], w[k])):
            e_max, e_rms = _relerr(g.cpu() - o, r - o), _rmserr(g.cpu() - o, r - o)
            worst.append((max(e_max, e_rms), k, i))
            print("%-6s %2d: update err %.2e (rms %.2e)" % (k, i, e_max, e_rms))
    m.close()
    assert max(worst)[0] < TOL_UPDATE_DECIDED, max(worst)


def _conv_outputs(x, conv_w, conv_b):
    import torch.nn.functional as F
    from oracle import vgg_oracle
    ys, h, i = [], x, 0
    with torch.no_grad():
        for v in vgg_oracle.VGG16_CFG:
            if v == "M":
                h = F.max_pool2d(h, 2, 2)
            else:
                h = F.relu(F.conv2d(h, conv_w[i], conv_b[i], padding=1))
                ys.append(h)
                i += 1
    return ys


def test_export_import_round_trip():
    from video_analytics_amd import synth, vgg
    w = synth.synth_vgg16_weights(c_in=3, seed=5)
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    got = m.export_state()
    for k in w:
        for a, b in zip(got[k], w[k]):
            assert torch.equal(a.cpu(), b)
    w2 = synth.synth_vgg16_weights(c_in=3, seed=6)
    m.import_state(w2)
    got = m.export_state()
    for k in w2:
        for a, b in zip(got[k], w2[k]):
            assert torch.equal(a.cpu(), b)
    m.train_init()
    m.import_state(w, momentum=True)
    gotm = m.export_state(momentum=True)
    for k in w:
        for a, b in zip(gotm[k], w[k]):
            assert torch.equal(a.cpu(), b)
    x = torch.zeros(1, 20, 224, 224, device="cuda")
    with pytest.raises(ValueError):
        m.train_step(x, torch.zeros(1, dtype=torch.int64), 0.1, 0.9, 0)  # 20 channels into a 3-channel model
    with pytest.raises(ValueError):
        m.train_step(x[:, :3], torch.zeros(2, dtype=torch.int64), 0.1, 0.9, 0)  # labels do not match the batch
    with pytest.raises(ValueError):
        m.import_state(dict(w, conv_w=w["conv_w"][:12]))
    m.close()


def test_out_of_range_labels_fail_loudly():
    """nn.CrossEntropyLoss refuses a target outside [0, C) (Sheet03/spatialModel.py:114,219); the mirror's datasets
    return the list files' raw 1-based labels, so label 101 with nActionClasses = 101 is one full UCF-101 list away.
    Host labels: ValueError before anything is launched.  Device labels: no out-of-bounds read, NaN loss."""
    from video_analytics_amd import synth, vgg
    logits = torch.from_numpy(synth.hash_uniform(3, 1, 4 * 101).reshape(4, 101)).cuda()
    good = torch.tensor([0, 100, 5, 7], dtype=torch.int64)
    ok = vgg.validate_batch(logits, good).cpu()
    assert torch.isfinite(ok).all()
    for bad in ([0, 101, 5, 7], [0, -1, 5, 7]):
        with pytest.raises(ValueError, match="out of bounds"):
            vgg.validate_batch(logits, torch.tensor(bad, dtype=torch.int64))
        out = vgg.validate_batch(logits, torch.tensor(bad, dtype=torch.int64).cuda()).cpu()
        assert torch.isnan(out[0]) and 0 <= float(out[1]) <= 3
    w = synth.synth_vgg16_weights(c_in=3, seed=4)
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    x = torch.zeros(2, 3, 224, 224, device="cuda")
    with pytest.raises(ValueError, match="out of bounds"):
        m.train_step(x, torch.tensor([1, 101], dtype=torch.int64), 1e-4, 0.9, 0)
    stats, _ = m.train_step(x, torch.tensor([1, 101], dtype=torch.int64).cuda(), 1e-4, 0.9, 0)
    assert torch.isnan(stats.cpu()[0])
    m.close()


class _MemDataset(torch.utils.data.Dataset):
    def __init__(self, x, labels, prefix):
        self.x, self.labels, self.prefix = x, labels, prefix

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], int(self.labels[i]), "v_%s_g01_c%02d" % (self.prefix, i + 1)


def test_execute_trains_validates_checkpoints_and_resumes(tmp_path, monkeypatch):
    """SpatialNetwork.execute() with a train loader (Sheet03/spatialModel.py:265-283): per epoch train + validate,
    checkpoint with the reference's keys, performance CSV, descriptor CSVs, best-model copy, the
    scheduler.step(loss) quirk, and resume() from the checkpoint into a fresh object."""
    import csv
    import os
    from torch.utils.data import DataLoader
    from video_analytics_amd import synth, spatialModel
    from video_analytics_amd.spatialModel import SpatialNetwork
    monkeypatch.chdir(tmp_path)
    for name in ("TRAIN_CSV", "TEST_CSV", "PERFORMANCE_CSV"):
        monkeypatch.setattr(SpatialNetwork, name, str(tmp_path / (name.lower() + ".csv")))
    w = synth.synth_vgg16_weights(c_in=3, seed=9)
    xs = torch.from_numpy(synth.hash_uniform(90, 1, 5 * 3 * 224 * 224).reshape(5, 3, 224, 224) * 4.0 - 2.0)
    train = DataLoader(_MemDataset(xs[:4], [1, 2, 3, 4], "Train"), batch_size=2, shuffle=False, num_workers=0)
    test = DataLoader(_MemDataset(xs[2:], [3, 4, 5], "Test"), batch_size=2, shuffle=False, num_workers=0)
    ckp = str(tmp_path / "ckp")
    net = SpatialNetwork(101, 2, 1e-4, 0.9, 256, train, test, [10, 20], ckp, gpu=True,
                         weights={k: [t.clone() for t in v] for k, v in w.items()})
    precision, loss = net.execute()
    assert net.epoch == 1 and 0.0 <= precision <= 1.0 and float(loss) > 0
    assert len(net.lastTrainStats) == 2 and all(float(t[0]) > 0 for t in net.lastTrainStats)
    rows = list(csv.reader(open(SpatialNetwork.PERFORMANCE_CSV)))
    assert len(rows) == 2 and float(rows[1][0]) == precision
    assert len(list(csv.reader(open(SpatialNetwork.TRAIN_CSV)))) == 4 and len(list(csv.reader(open(SpatialNetwork.TEST_CSV)))) == 3
    # scheduler.step(loss): the loss value is what MultiStepLR sees as the epoch
    assert net.schedulerLastEpoch == float(loss)
    assert abs(net.currentLr() - 1e-4 * 0.1 ** sum(float(loss) >= ms for ms in (10, 20))) < 1e-12
    ck = torch.load(os.path.join(ckp, "spatial_ckp.pth.tar"), weights_only=True)
    assert set(ck.keys()) >= {"epoch", "model", "highestPrecision", "optimizer"} and ck["epoch"] == 1
    assert list(ck["model"].keys())[:2] == ["module.features.0.weight", "module.features.0.bias"]
    assert len(ck["model"]) == 34 and len(ck["optimizer"]["state"]) == 34
    assert ck["optimizer"]["param_groups"][0]["momentum"] == 0.9
    moved = float((ck["model"]["module.classifier.9.weight"] - w["fc_w"][3]).abs().max())
    assert moved > 0  # the parameters were really updated
    if net.isBest:
        assert os.path.isfile(os.path.join(ckp, "spatial_best.pth.tar"))
    trained = net.model.export_state()
    net.model.close()
    # a fresh object resumes: epoch counter, parameters and momentum come from the checkpoint
    net2 = SpatialNetwork(101, 3, 1e-4, 0.9, 256, train, test, [10, 20], ckp, gpu=True,
                          weights={k: [t.clone() for t in v] for k, v in w.items()})
    assert net2.resume() and net2.startEpoch == 2 and net2.schedulerLastEpoch == 2
    got = net2.model.export_state()
    for k in got:
        for a, b in zip(got[k], trained[k]):
            assert torch.equal(a, b)
    gotm = net2.model.export_state(momentum=True)
    assert torch.equal(gotm["fc_w"][3].cpu(), ck["optimizer"]["state"][32]["momentum_buffer"])
    net2.model.close()
    # no checkpoint directory: resume() reports False
    net3 = SpatialNetwork(101, 1, 1e-4, 0.9, 256, None, test, [10, 20], str(tmp_path / "none"), gpu=True,
                          weights={k: [t.clone() for t in v] for k, v in w.items()})
    assert net3.resume() is False
    net3.model.close()


def test_large_batch_step_is_deterministic():
    """Batch 40 takes the 64-row instantiations of the classifier kernels and crosses a batch brick of the
    convolution tiles.  No CPU oracle at this size (minutes on 8 cores): two runs from the same state must give
    bit-identical statistics, descriptors and parameters (there are no atomics anywhere in the step), and the step
    agrees with torch autograd on the GPU (vendor kernels) at the tolerances of the small-batch oracle tests."""
    from video_analytics_amd import synth, vgg
    w = synth.synth_vgg16_weights(c_in=3, seed=12)
    x = torch.from_numpy(synth.hash_uniform(91, 2, 40 * 3 * 224 * 224).reshape(40, 3, 224, 224) * 4.0 - 2.0).cuda()
    y = torch.arange(40, dtype=torch.int64) % 101
    outs = []
    for _ in range(2):
        m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
        stats, desc = m.train_step(x, y, 1e-4, 0.9, 77)
        st = m.export_state()
        outs.append((stats.cpu(), desc.cpu(), [t.cpu() for k in ("conv_w", "conv_b", "fc_w", "fc_b") for t in st[k]]))
        m.close()
    assert torch.isfinite(outs[0][0]).all() and float(outs[0][0][0]) > 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][2], outs[1][2]))
    assert any(not torch.equal(a, b) for a, b in zip(outs[0][2][:26:2], w["conv_w"]))  # conv weights moved
    # A second witness, which determinism cannot give (two runs overlap their workspace regions the same way): the same step
    # by torch autograd ON THE GPU -- vendor conv / linear kernels in fp32 and torch.optim.SGD, nothing of this library; the
    # precedent is test_fp32_stream_against_an_independent_gpu_implementation -- with the dropout masks of the oracle.
    import time
    t0 = time.time()
    loss_g, state_g = _vendor_autograd_step(w, x, y, 1e-4, 0.9, 77)
    print("batch 40: the vendor-kernel step took %.1f s" % (time.time() - t0))
    loss = float(outs[0][0][0])
    assert abs(loss - loss_g) < 2e-4 * max(1.0, abs(loss_g)), (loss, loss_g)
    keys = [(k, i) for k in ("conv_w", "conv_b", "fc_w", "fc_b") for i in range(len(w[k]))]
    worst = {"conv": (0.0, None), "fc": (0.0, None)}
    for (k, i), got, ref in zip(keys, outs[0][2], state_g):
        w0 = w[k][i].cuda()
        e = _relerr(got.cuda() - w0, ref - w0)
        print("batch 40 %-6s %2d: update err against the vendor-kernel step %.2e" % (k, i, e))
        worst[k[:-2]] = max(worst[k[:-2]], (e, (k, i)))
    assert worst["conv"][0] < TOL_UPDATE, worst["conv"]
    assert worst["fc"][0] < 5e-4, worst["fc"]


def _vendor_autograd_step(w, x, y, lr, mu, seed):
    """One training step by torch autograd on the GPU (fp32 vendor kernels) + torch.optim.SGD from the weights ``w``, with the
    dropout masks of oracle.train_oracle: -> (loss, updated parameters on the GPU in the order conv_w, conv_b, fc_w, fc_b)."""
    import torch.nn.functional as F
    from oracle import train_oracle, vgg_oracle
    p = {k: [t.clone().cuda().requires_grad_(True) for t in v] for k, v in w.items()}
    flat = [t for k in ("conv_w", "conv_b", "fc_w", "fc_b") for t in p[k]]
    opt = torch.optim.SGD(flat, lr, momentum=mu)
    feat = vgg_oracle.features(x.cuda().to(torch.float32), p["conv_w"], p["conv_b"])
    op = feat.reshape(feat.size(0), -1)
    for l in range(3):
        op = F.relu(F.linear(op, p["fc_w"][l], p["fc_b"][l]))
        op = op * train_oracle.dropout_mask(seed, l, tuple(op.shape)).cuda()
    loss = F.cross_entropy(F.linear(op, p["fc_w"][3], p["fc_b"][3]), y.cuda())
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    return float(loss.detach()), [t.detach() for t in flat]


@pytest.mark.parametrize("layer", [12, 9, 4])
def test_activation_gradients_layer_by_layer(layer):
    """The gradient at a conv layer's (post-ReLU, pre-pool) output, read out of the training workspace after the
    backward pass of that layer (VA_OPT_TRAIN_STOP_AT + va_vgg16_train_plan), against autograd's: identical sparsity
    pattern except for the handful of arg-max / ReLU decisions that differ between two fp32 forward passes, and
    values within 1e-3 (deep layers: 1e-2) of the tensor's largest gradient everywhere else."""
    import ctypes
    import torch.nn.functional as F
    from oracle import train_oracle, vgg_oracle
    from video_analytics_amd import _ffi, synth, vgg
    torch.set_num_threads(8)
    B = 2
    w = synth.synth_vgg16_weights(c_in=3, seed=4)
    x = torch.from_numpy(synth.hash_uniform(70, 3, B * 3 * 224 * 224).reshape(B, 3, 224, 224) * 4.0 - 2.0)
    labels = torch.tensor([1, 8], dtype=torch.int64)
    P = {k: [t.clone().requires_grad_(True) for t in v] for k, v in w.items()}
    ys, h, i = [], x, 0
    for v in vgg_oracle.VGG16_CFG:
        if v == "M":
            h = F.max_pool2d(h, 2, 2)
        else:
            h = F.relu(F.conv2d(h, P["conv_w"][i], P["conv_b"][i], padding=1))
            h.retain_grad()
            ys.append(h)
            i += 1
    op = h.reshape(B, -1)
    for l in range(3):
        op = F.relu(F.linear(op, P["fc_w"][l], P["fc_b"][l])) * train_oracle.dropout_mask(5, l, (B, P["fc_w"][l].shape[0]))
    F.cross_entropy(F.linear(op, P["fc_w"][3], P["fc_b"][3]), labels).backward()
    y = ys[layer].detach().permute(0, 2, 3, 1)
    ref = (ys[layer].grad.permute(0, 2, 3, 1) * (y > 0)).contiguous()

    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    m.set_option(_ffi.VA_OPT_TRAIN_STOP_AT, layer)
    with pytest.raises(RuntimeError, match="stopped after the backward pass of conv layer %d" % layer):
        m.train_step(x.cuda(), labels.cuda(), 1e-4, 0.9, 5)  # a cut-short step is an error, never a silent VA_OK
    torch.cuda.synchronize()
    off = (ctypes.c_ulonglong * 30)()
    _ffi.check(_ffi.lib().va_vgg16_train_plan(m._h, B, off))
    ws = [t for k, t in vgg._ws_cache.items() if "train" in str(k)][0]
    n = ref.numel()
    scale = float(ref.abs().max())
    # above the first decision flip the agreement is 1e-3 of the largest gradient; below it the flipped
    # elements' contributions are spread over every gradient by the convolutions (TOL_UPDATE's story)
    tol = 1e-3 if layer >= 9 else 1e-2
    best = None
    for gi in (26, 27):  # the layer's gradient is in one of the two ping-pong buffers
        g = ws[off[gi]:off[gi] + 4 * n].view(torch.float32).view(ref.shape).cpu()
        support = int(((g != 0) != (ref != 0)).sum())
        far = int(((g - ref).abs() > tol * scale).sum())
        if best is None or far < best[1]:
            best = (support, far)
    m.close()
    # (layer 4 measured: identical sparsity pattern, 0.08 % of the elements beyond 1e-2 -- the receptive field of the
    # two windows that flipped at conv4_3)
    assert best[0] <= 64 and best[1] <= (max(64, n // 10000) if layer >= 9 else n // 500), best


def test_training_step_against_the_committed_golden():
    """tests/golden/train_small.npz (two autograd steps on 2 clips, lr 1e-4, momentum 0.9): the first step's loss,
    hits, train-mode descriptors, updated classifier head and its momentum buffer; the second step's loss only
    loosely (two fp32 trajectories after one update of a random-init network)."""
    import os
    from video_analytics_amd import synth, vgg
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_small.npz"))
    w = synth.synth_vgg16_weights(c_in=3, seed=4)
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    for step in range(2):
        x = torch.from_numpy(synth.hash_uniform(70 + step, 3, 2 * 3 * 224 * 224).reshape(2, 3, 224, 224) * 4.0 - 2.0)
        labels = torch.tensor([(7 * i + 3 * step + 1) % 101 for i in range(2)], dtype=torch.int64)
        stats, desc = m.train_step(x.cuda(), labels.cuda(), 1e-4, 0.9, 1000 + step)
        loss_r = float(g["loss_%d" % step])
        assert abs(float(stats[0]) - loss_r) < (2e-4 if step == 0 else 5e-3) * loss_r, (step, float(stats[0]), loss_r)
        if step == 0:
            assert int(stats[1]) == int(g["hits_0"])
            assert _relerr(desc.cpu(), torch.from_numpy(g["desc_0"])) < 1e-3
            head = m.export_state()["fc_w"][3].cpu()
            assert _relerr(head - w["fc_w"][3], torch.from_numpy(g["head_w_0"]) - w["fc_w"][3]) < 5e-4
            assert _relerr(m.export_state(momentum=True)["fc_w"][3].cpu(), torch.from_numpy(g["head_mom_0"])) < 5e-4
    m.close()


def test_loss_goes_down_on_a_fixed_batch():
    """Functional check of the whole loop: 30 momentum-SGD steps on one fixed 8-clip batch (Dropout active)
    bring the mean cross-entropy from its random-init value (tens) down to the level of the label set
    (ln 101 = 4.6; a uniform guess over the 8 labels would be 2.1)."""
    from video_analytics_amd import synth, vgg
    w = synth.synth_vgg16_weights(c_in=3, seed=21)
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
    x = torch.from_numpy(synth.hash_uniform(95, 0, 8 * 3 * 224 * 224).reshape(8, 3, 224, 224) * 4.0 - 2.0).cuda()
    y = torch.tensor([1, 2, 3, 4, 5, 6, 7, 8])
    losses = [float(m.train_step(x, y, 3e-5, 0.9, it)[0][0]) for it in range(30)]
    m.close()
    assert losses[0] > 20.0 and all(l == l for l in losses)          # finite all the way
    assert min(losses[-5:]) < 0.25 * losses[0] and min(losses[-5:]) < 6.0, losses
