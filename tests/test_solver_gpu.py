"""The solver on the device: weight decay, the dropout ratio and frozen layers in every form of the step.

  1. A model whose solver was set to the defaults keeps the bits of one whose solver was never set.
  2. Weight decay against torch.optim.SGD with two param groups (weights, biases), the oracle evaluated under the product's own
     ReLU and pooling decisions, at tests/test_train_gpu.py's tolerances.  The weight decay is chosen for the synthetic
     weights: their gradients are 200 .. 400 times larger than the weights themselves (loss 29 .. 43 at the random init), so a
     decay of 4 is what moves every weight tensor's update by 10 tolerances -- asserted on the oracle's side alone.
  3. The arithmetic exactly: V' and W' of every element within one float32 ulp of the three stated fused multiply-adds, each
     evaluated in float64 on the exported gradient; the fused step against store + apply bit for bit in all three forms.
  4. Clipping acts on the raw gradient: its norm is the raw gradient's, the update is c g, then decay, then momentum.
  5. Dropout(p): the kernel alone against ``synth.hash_uniform``, and a full step with three different ratios.
  6. Frozen layers keep every bit; everything else keeps the bits of the unfrozen step.
  7. ``train_videos(solver=...)`` is ``set_solver`` + the consensus step per stream.
  8. Refusals change nothing.
"""
import ctypes
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_train_gpu import TOL_UPDATE_DECIDED, _relerr, _rmserr
from test_train_kernels_gpu import _bits_equal, _ulp32
from test_video_gpu import SCHEDULE, _synthetic_video

pytestmark = pytest.mark.gpu

LR, MU = 1e-4, 0.9
KEYS = ("conv_w", "conv_b", "fc_w", "fc_b")
HEADS = (3, 5)
TOL_NORM = 1e-7  # tests/test_accum_gpu.py: the device norm against the float64 norm of the device's own gradient
WD_ORACLE = 4.0  # see 2. in the docstring

_W = {}


def _weights(c_in, n_classes=101, seed=4):
    from video_analytics_amd import synth, vgg
    key = (c_in, n_classes, seed)
    if key not in _W:
        w = synth.synth_vgg16_weights(c_in=3, n_classes=n_classes, seed=seed)
        if c_in != 3:
            w["conv_w"][0] = vgg.copy_first_layer(w["conv_w"][0].cuda(), c_in).cpu()
        _W[key] = w
    return _W[key]


def _momentum(c_in, n_classes=101):
    """Non-zero momentum buffers: another draw of the weights' shapes, a tenth of their size."""
    if ("mom", c_in, n_classes) not in _W:
        _W[("mom", c_in, n_classes)] = {k: [0.1 * t for t in v] for k, v in _weights(c_in, n_classes, seed=9).items()}
    return _W[("mom", c_in, n_classes)]


def _stream(c_in, n_classes=101, momentum=False):
    from video_analytics_amd import vgg
    w = _weights(c_in, n_classes)
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], n_classes, 256)
    if momentum:
        m.import_state(_momentum(c_in, n_classes), momentum=True)
    return m


def _x(B, c_in, seed):
    from video_analytics_amd import synth
    return torch.from_numpy(synth.hash_uniform(seed, c_in, B * c_in * 224 * 224).reshape(B, c_in, 224, 224) * 4.0 - 2.0)


def _flat(d):
    return [t for k in KEYS for t in d[k]]


def _state(m):
    """The 34 parameters, then the 34 momentum buffers, on the device (layer l: entries l and 13 + l of the conv lists ...)."""
    return _flat(m.export_state()) + _flat(m.export_state(momentum=True))


def _same(a, b):
    return len(a) == len(b) and all(_bits_equal(u, v) for u, v in zip(a, b))


def _layer_of(j):
    """Layer 0..16 of entry j of ``_flat``: 13 conv weights, 13 conv biases, 4 fc weights, 4 fc biases."""
    return j if j < 13 else j - 13 if j < 26 else 13 + (j - 26) % 4


@pytest.fixture(autouse=True)
def training_workspaces_released():
    yield
    from video_analytics_amd import vgg
    torch.cuda.synchronize()
    for key in [key for key in vgg._ws_cache if "train" in str(key)]:
        del vgg._ws_cache[key]


# form -> (n_classes, images, k, labels, tasks, heads)
FORMS = {
    "plain": (101, 2, 0, [1, 8], None, None),
    "consensus": (101, 2, 2, [8], None, None),     # 1 video x 2 snippets
    "multitask": (8, 4, 2, [1, 3], [0, 1], HEADS),  # two heads
}


def _fused(m, form, x, seed):
    _, _, k, labels, tasks, heads = FORMS[form]
    y = torch.tensor(labels, dtype=torch.int64).cuda()
    if form == "plain":
        return m.train_step(x, y, LR, MU, seed)
    if form == "consensus":
        return m.train_step_consensus(x, y, k, LR, MU, seed)
    return m.train_step_multitask(x, y, torch.tensor(tasks, dtype=torch.int32).cuda(), heads, k, LR, MU, seed)


def _accumulate(m, form, x, seed, first=True):
    _, _, k, labels, tasks, heads = FORMS[form]
    y = torch.tensor(labels, dtype=torch.int64).cuda()
    t = None if tasks is None else torch.tensor(tasks, dtype=torch.int32).cuda()
    return m.train_accumulate(x, y, k=k, tasks=t, heads=heads, scales=None, first=first, dropout_seed=seed)


# ---- the torch side: two param groups and Dropout(p) ----

def _dropout_mask(seed, layer, shape, p):
    """0 / s mask of Dropout(p): kept iff synth.hash_uniform(seed, 100 + layer) >= float32(p), s = 1 / (1 - float32(p)) in float32."""
    from video_analytics_amd import synth
    p32 = np.float32(p)
    keep = synth.hash_uniform(int(seed), 100 + layer, int(np.prod(shape))) >= p32
    s = np.float32(1.0) / (np.float32(1.0) - p32)
    return torch.from_numpy(keep.astype(np.float32) * s).reshape(shape)


def _solver_oracle(weights, lr, momentum, solver):
    from oracle import train_oracle, vgg_oracle

    class SolverOracle(train_oracle.TrainOracle):
        """torch.optim.SGD with the weights in one param group (lr, weight_decay) and the biases in another (lr_t, wd_t), and
        the three Dropout layers at the solver's ratios."""

        def __init__(self):
            super(SolverOracle, self).__init__(weights, lr, momentum)
            p = self.params
            lr32, wd32 = np.float32(lr), np.float32(solver.weight_decay)
            groups = [dict(params=p["conv_w"] + p["fc_w"], lr=float(lr32), weight_decay=float(wd32)),
                      dict(params=p["conv_b"] + p["fc_b"], lr=float(lr32 * np.float32(solver.bias_lr_mult)),
                           weight_decay=float(wd32 * np.float32(solver.bias_decay_mult)))]
            self.opt = torch.optim.SGD(groups, lr, momentum=momentum)

        def step(self, x, labels, seed, decisions=None):
            p = self.params
            if decisions is None:
                feat = vgg_oracle.features(x.to(torch.float32), p["conv_w"], p["conv_b"])
            else:
                feat = train_oracle.features_under_decisions(x.to(torch.float32), p["conv_w"], p["conv_b"], decisions)
            op = feat.reshape(feat.size(0), -1)
            for l in range(3):
                op = F.relu(F.linear(op, p["fc_w"][l], p["fc_b"][l]))
                op = op * _dropout_mask(seed, l, tuple(op.shape), solver.dropout[l])
            desc = op
            logits = F.linear(op, p["fc_w"][3], p["fc_b"][3])
            loss = F.cross_entropy(logits, labels)
            self.opt.zero_grad()
            loss.backward()
            grads = {k: [t.grad.clone() for t in v] for k, v in p.items()}
            self.opt.step()
            return float(loss.detach()), int((logits.argmax(1) == labels).sum()), desc.detach(), grads

    return SolverOracle()


def _decisions(m, B):
    """The ReLU masks and pooling arg-maxima of the product's last forward pass, from the training workspace."""
    from oracle import train_oracle, vgg_oracle
    from video_analytics_amd import _ffi, vgg
    torch.cuda.synchronize()
    off = (ctypes.c_ulonglong * 30)()
    _ffi.check(_ffi.lib().va_vgg16_train_plan(m._h, B, off))
    ws = [t for k, t in vgg._ws_cache.items() if "train" in str(k)][0]
    ys, hw = [], 224
    for i, v in enumerate([c for c in vgg_oracle.VGG16_CFG if c != "M"]):
        n = B * hw * hw * v
        ys.append(ws[off[i]:off[i] + 4 * n].view(torch.float32).view(B, hw, hw, v).permute(0, 3, 1, 2).contiguous().cpu())
        if off[13 + i]:
            hw //= 2
    return train_oracle.decisions_from_activations(ys)


def _check_against_oracle(m, ora, w0, stats, desc, loss_r, corr_r, desc_r, what):
    stats = stats.cpu()
    assert abs(float(stats[0]) - loss_r) < 2e-4 * max(1.0, abs(loss_r)), (what, float(stats[0]), loss_r)
    assert int(stats[1]) == corr_r, what
    assert _relerr(desc.cpu(), desc_r) < 1e-3, what
    got, ref = m.export_state(), ora.weights()
    gotm, refm = m.export_state(momentum=True), ora.momentum()
    worst = []
    for k in KEYS:
        for i, (g, r, o, gm, rm) in enumerate(zip(got[k], ref[k], w0[k], gotm[k], refm[k])):
            e_upd, e_rms, e_mom = _relerr(g.cpu() - o, r - o), _rmserr(g.cpu() - o, r - o), _relerr(gm.cpu(), rm)
            worst.append((max(e_upd, e_rms, e_mom), k, i))
            print("%s %-6s %2d: update err %.2e (rms %.2e)  momentum err %.2e" % (what, k, i, e_upd, e_rms, e_mom))
    assert max(worst)[0] < TOL_UPDATE_DECIDED, (what, max(worst))


# ---- 1: defaults keep bits ----

@pytest.mark.parametrize("c_in,B", [(3, 2), (20, 3)])
def test_default_solver_keeps_the_bits_of_a_model_without_one(c_in, B):
    from video_analytics_amd import vgg
    a, b = _stream(c_in), _stream(c_in)
    b.set_solver(vgg.Solver())
    assert a.solver == b.solver == vgg.Solver()
    x = _x(B, c_in, 80).cuda()
    y = torch.tensor([(7 * i + 1) % 101 for i in range(B)], dtype=torch.int64).cuda()
    for r in range(2):  # the second step moves non-zero momentum buffers
        (sa, da), (sb, db) = a.train_step(x, y, LR, MU, 1000 + r), b.train_step(x, y, LR, MU, 1000 + r)
        assert torch.equal(sa, sb) and torch.equal(da, db) and bool(torch.isfinite(sa).all())
        sta, stb = _state(a), _state(b)
        assert len(sta) == 68 and all(torch.equal(u, v) for u, v in zip(sta, stb)), r
    for m in (a, b):
        m.train_accumulate(x, y, first=True, dropout_seed=1002)
    na, nb = a.train_apply(LR, MU, 0.05), b.train_apply(LR, MU, 0.05)
    assert torch.equal(na, nb) and torch.equal(a.grad(), b.grad())
    assert all(torch.equal(u, v) for u, v in zip(_state(a), _state(b)))
    a.close()
    b.close()


# ---- 2: decay against torch ----

@pytest.mark.parametrize("c_in,B,lr_mult,decay_mult", [pytest.param(3, 2, 2.0, 0.0, id="3-2-caffe-multipliers"),
                                                         pytest.param(20, 3, 1.0, 1.0, id="20-3-torch-multipliers")])
def test_weight_decay_matches_torch_sgd(c_in, B, lr_mult, decay_mult):
    from video_analytics_amd import vgg
    torch.set_num_threads(8)
    w = _weights(c_in)
    solver = vgg.Solver(weight_decay=WD_ORACLE, bias_lr_mult=lr_mult, bias_decay_mult=decay_mult)
    ora = _solver_oracle(w, LR, MU, solver)
    m = _stream(c_in)
    m.set_solver(solver)
    w0 = {k: [t.clone() for t in v] for k, v in w.items()}
    for step in range(2):
        if step == 1:  # from the oracle's own state: parameters and the momentum buffers its first step filled
            m.import_state(ora.weights())
            m.import_state(ora.momentum(), momentum=True)
            w0 = ora.weights()
        x = _x(B, c_in, 70 + step)
        labels = torch.tensor([(7 * i + 3 * step + 1) % 101 for i in range(B)], dtype=torch.int64)
        stats, desc = m.train_step(x.cuda(), labels.cuda(), LR, MU, 1000 + step)
        loss_r, corr_r, desc_r, grads = ora.step(x, labels, 1000 + step, decisions=_decisions(m, B))
        if step == 0:
            # precondition, the oracle alone: V was 0, so without decay the update is -lr g; with it every weight tensor
            # moves differently by at least ten tolerances -- a missing decay cannot pass
            now = ora.weights()
            for k in ("conv_w", "fc_w"):
                for i, (o, n, g) in enumerate(zip(w0[k], now[k], grads[k])):
                    seen = _relerr(n - o, g * -float(np.float32(LR)))
                    assert seen >= 10 * TOL_UPDATE_DECIDED, (k, i, seen)
        _check_against_oracle(m, ora, w0, stats, desc, loss_r, corr_r, desc_r, "step %d" % step)
    m.close()


# ---- 3, 4: the arithmetic, exactly ----

def _f64(v):
    return float(np.float32(v))


def _expected_update(w, v, g, lr_t, wd_t, mu, c=None):
    """The stated fused multiply-adds, each evaluated in float64 and rounded to float32 -> (V', W') float32."""
    w64, v64, g64 = w.double(), v.double(), g.double()
    if c is not None:
        g64 = (_f64(c) * g64).float().double()  # c g: one float32 product
    d = (_f64(wd_t) * w64 + g64).float().double() if wd_t != 0 else g64
    nv = (_f64(mu) * v64 + d).float()
    nw = (-_f64(lr_t) * nv.double() + w64).float()
    return nv, nw


def _assert_update_within_one_ulp(before, after, grad, solver, c=None, frozen=0):
    """before / after: ``_state`` lists; grad: ``_flat(export_grad())``; every V' and W' within one float32 ulp."""
    lr32, wd32 = np.float32(LR), np.float32(solver.weight_decay)
    for j in range(34):
        bias = 13 <= j < 26 or j >= 30
        lr_t = lr32 * np.float32(solver.bias_lr_mult) if bias else lr32
        wd_t = wd32 * np.float32(solver.bias_decay_mult) if bias else wd32
        if _layer_of(j) < frozen:
            assert torch.equal(before[j], after[j]) and torch.equal(before[34 + j], after[34 + j]), j
            continue
        nv, nw = _expected_update(before[j], before[34 + j], grad[j], lr_t, wd_t, MU, c)
        for name, got, ref in (("V", after[34 + j], nv), ("W", after[j], nw)):
            err = (got.double() - ref.double()).abs()
            assert bool((err <= _ulp32(ref.double())).all()), (name, j, float(err.max()))
        if solver.weight_decay > 0 and not (bias and solver.bias_decay_mult == 0):  # the decay is seen: V' is not mu V + g
            plain, _ = _expected_update(before[j], before[34 + j], grad[j], lr_t, 0.0, MU, c)
            assert not torch.equal(after[34 + j], plain), j


def test_decay_arithmetic_is_the_three_fused_multiply_adds():
    from video_analytics_amd import vgg
    solver = vgg.Solver(weight_decay=5e-4, bias_lr_mult=2.0, bias_decay_mult=0.5)
    a, b = _stream(3, momentum=True), _stream(3, momentum=True)
    a.set_solver(solver)
    b.set_solver(solver)
    x = _x(2, 3, 80).cuda()
    before = _state(a)
    assert _same(before, _state(b)) and float(before[34].abs().max()) > 0
    _accumulate(b, "plain", x, 1000)
    grad = _flat(b.export_grad())
    _fused(a, "plain", x, 1000)
    after = _state(a)
    _assert_update_within_one_ulp(before, after, grad, solver)
    # every bias followed its own lr_t and wd_t: with the weights' it would have landed elsewhere
    for j in list(range(13, 26)) + list(range(30, 34)):
        _, as_weight = _expected_update(before[j], before[34 + j], grad[j], np.float32(LR), np.float32(5e-4), MU)
        assert not torch.equal(after[j], as_weight), j
    a.close()
    b.close()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_store_then_apply_is_the_fused_step_under_a_full_solver(form):
    """Decay, both multipliers, three dropout ratios and five frozen layers at once, two steps from non-zero momentum."""
    from video_analytics_amd import vgg
    n_classes, B = FORMS[form][:2]
    solver = vgg.Solver(weight_decay=5e-4, bias_lr_mult=2.0, bias_decay_mult=0.5, dropout=(0.3, 0.7, 0.6), freeze=5)
    a, b = _stream(3, n_classes, momentum=True), _stream(3, n_classes, momentum=True)
    a.set_solver(solver)
    b.set_solver(solver)
    before = _state(a)
    for r in range(2):
        x = _x(B, 3, 80 + r).cuda()
        sf, df = _fused(a, form, x, 1000 + r)
        sa, da = _accumulate(b, form, x, 1000 + r)
        assert b.train_apply(LR, MU) is None
        assert _bits_equal(sf, sa) and _bits_equal(df, da) and bool(torch.isfinite(sa).all()), (form, r)
        assert _same(_state(a), _state(b)), (form, r)
    after = _state(a)
    for j in range(34):
        moved = not (torch.equal(before[j], after[j]) and torch.equal(before[34 + j], after[34 + j]))
        assert moved == (_layer_of(j) >= 5), (form, j)
    a.close()
    b.close()


def test_clipping_acts_on_the_raw_gradient_before_the_decay():
    from video_analytics_amd import vgg
    solver = vgg.Solver(weight_decay=5e-4, bias_lr_mult=2.0, bias_decay_mult=0.5)
    m = _stream(3, momentum=True)
    m.set_solver(solver)
    before = _state(m)
    _accumulate(m, "plain", _x(2, 3, 80).cuda(), 1000)
    grad = _flat(m.export_grad())
    raw = float(torch.sqrt(sum((t.double() ** 2).sum() for t in grad)))
    clip = float(np.float32(0.5 * raw))
    norm = float(m.train_apply(LR, MU, clip).cpu()[0])
    print("norm: device %.17g, float64 of the exported raw gradient %.17g" % (norm, raw))
    assert abs(norm - raw) <= TOL_NORM * raw  # the decay (5e-4 |W|) is not in it
    c = np.float32(clip / (norm + 1e-6))
    assert 0.4 < c < 0.6
    _assert_update_within_one_ulp(before, _state(m), grad, solver, c=c)
    m.close()


# ---- 5: the dropout ratio ----

def test_dropout_kernel_follows_the_hash_at_every_ratio():
    from video_analytics_amd import _ffi, synth, vgg
    n, seed, layer = 4099, 77, 1
    x = (synth.hash_uniform(5, 3, n) * 4.0 - 2.0).astype(np.float32)
    x[17] = np.nan
    assert (x < 0).any() and (x > 0).any()
    u = synth.hash_uniform(seed, 100 + layer, n)
    L = _ffi.lib()

    def run(p):
        t = torch.from_numpy(x.copy()).cuda()
        _ffi.check(L.va_train_dropout_p(_ffi.ctx(0), _ffi.ptr(t), n, seed, layer, p, _ffi.stream_ptr(t)))
        return t.cpu().numpy()

    with np.errstate(invalid="ignore"):
        for p in (0.0, 0.1, 0.5, 0.7, 0.8, 0.9):
            p32 = np.float32(p)
            mask = (u >= p32).astype(np.float32) * (np.float32(1.0) / (np.float32(1.0) - p32))
            want, got = x * mask, run(p)
            assert np.isnan(got[17]) and np.isnan(want[17])  # a dropped NaN stays NaN
            ok = np.arange(n) != 17
            assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok]), p  # -0 for a dropped negative included
            if p == 0.0:
                assert np.array_equal(got.view(np.uint32), x.view(np.uint32))  # untouched
            else:
                assert 0 < int((got[ok] == 0).sum()) < n - 1
            via = torch.from_numpy(x.copy()).cuda()
            vgg.train_dropout(via, seed, layer, p)
            assert np.array_equal(via.cpu().numpy().view(np.uint32), got.view(np.uint32)), p
    old = torch.from_numpy(x.copy()).cuda()
    _ffi.check(L.va_train_dropout(_ffi.ctx(0), _ffi.ptr(old), n, seed, layer, _ffi.stream_ptr(old)))
    assert np.array_equal(old.cpu().numpy().view(np.uint32), run(0.5).view(np.uint32))
    for bad in (1.0, -0.1, float("nan")):
        t = torch.zeros(4).cuda()
        assert L.va_train_dropout_p(_ffi.ctx(0), _ffi.ptr(t), 4, 0, 0, bad, _ffi.stream_ptr(t)) == _ffi.VA_ERR_INVALID
        with pytest.raises(ValueError):
            vgg.train_dropout(t, 0, 0, bad)


def test_step_with_three_dropout_ratios_matches_autograd():
    """Each Dropout layer at its own ratio, forward and backward: the oracle multiplies by the 0 / s_l masks, so a classifier
    backward that used one scale for all three layers (2, or any layer's s) would put dFC1 .. dFC3 off by s_l / s."""
    from video_analytics_amd import vgg
    torch.set_num_threads(8)
    ratios = (0.8, 0.7, 0.9)
    scales = [vgg.dropout_scale(p) for p in ratios]
    assert len(set(scales)) == 3 and all(abs(s / t - 1) > 0.3 for s in scales for t in scales + [2.0] if s != t)
    solver = vgg.Solver(dropout=ratios)
    w = _weights(3)
    ora = _solver_oracle(w, LR, MU, solver)
    m = _stream(3)
    m.set_solver(solver)
    x = _x(2, 3, 70)
    labels = torch.tensor([1, 8], dtype=torch.int64)
    stats, desc = m.train_step(x.cuda(), labels.cuda(), LR, MU, 1000)
    loss_r, corr_r, desc_r, _ = ora.step(x, labels, 1000, decisions=_decisions(m, 2))
    kept = float((desc_r != 0).float().mean())
    assert 0 < kept < 0.2  # Dropout(0.9) on the descriptor layer
    assert float(desc_r.max()) > 0
    _check_against_oracle(m, ora, w, stats, desc, loss_r, corr_r, desc_r, "dropout %s" % (ratios,))
    m.close()


# ---- 6: frozen layers ----

@pytest.fixture(scope="module")
def unfrozen_step():
    """One fused step with weight decay from non-zero momentum, nothing frozen: what every frozen run is compared with."""
    from video_analytics_amd import vgg
    m = _stream(3, momentum=True)
    m.set_solver(vgg.Solver(weight_decay=5e-4))
    before = _state(m)
    x = _x(2, 3, 80).cuda()
    stats, desc = _fused(m, "plain", x, 1000)
    out = dict(before=before, after=_state(m), stats=stats.clone(), desc=desc.clone(), x=x)
    m.close()
    return out


@pytest.mark.parametrize("n", [1, 2, 7, 13, 16])
def test_frozen_layers_keep_every_bit_and_the_rest_keeps_the_unfrozen_steps(unfrozen_step, n):
    from video_analytics_amd import vgg
    ref = unfrozen_step
    solver = vgg.Solver(weight_decay=5e-4, freeze=n)
    a, b = _stream(3, momentum=True), _stream(3, momentum=True)
    a.set_solver(solver)
    b.set_solver(solver)
    assert _same(_state(a), ref["before"])
    stats, desc = _fused(a, "plain", ref["x"], 1000)
    assert torch.equal(stats, ref["stats"]) and torch.equal(desc, ref["desc"])  # loss, hits, descriptors
    after = _state(a)
    for j in range(34):
        for q in (j, 34 + j):  # parameter, momentum buffer
            if _layer_of(j) < n:
                assert torch.equal(after[q], ref["before"][q]), (n, q)
            else:
                assert torch.equal(after[q], ref["after"][q]) and not torch.equal(after[q], ref["before"][q]), (n, q)
    # accumulate: zeros in the frozen segments (over whatever was there), apply leaves frozen tensors alone, the norm is the
    # unfrozen segments'
    g = b.grad()
    g.fill_(1.0)
    _accumulate(b, "plain", ref["x"], 1000)
    off, cnt = b.grad_layout()
    sumsq = 0.0
    for s in range(34):
        seg = g[off[s]:off[s] + cnt[s]]
        if s // 2 < n:
            assert not bool(seg.any()), (n, s)
        else:
            assert bool(seg.any()), (n, s)
            sumsq += float((seg.double() ** 2).sum())
    g[off[0]:off[0] + cnt[0]].fill_(3.0)  # what a frozen segment holds is never read
    raw = sumsq ** 0.5
    norm = float(b.train_apply(LR, MU, 10.0 * raw).cpu()[0])  # c = 1: the update is the fused step's
    assert abs(norm - raw) <= TOL_NORM * raw, (n, norm, raw)
    assert _same(_state(b), after), n
    a.close()
    b.close()


def test_freeze_may_change_between_steps_and_a_frozen_stop_layer_is_never_reached():
    from video_analytics_amd import _ffi, vgg
    m = _stream(3)
    x = _x(2, 3, 80).cuda()
    w0 = _flat(m.export_state())
    m.set_solver(vgg.Solver(freeze=13))
    m.set_option(_ffi.VA_OPT_TRAIN_STOP_AT, 0)  # conv layer 0 is frozen: the step completes
    stats, _ = _fused(m, "plain", x, 1000)
    assert bool(torch.isfinite(stats).all())
    w1 = _flat(m.export_state())
    assert all(torch.equal(w0[j], w1[j]) == (_layer_of(j) < 13) for j in range(34))
    m.set_solver(vgg.Solver(freeze=0))
    with pytest.raises(RuntimeError, match="stopped"):  # now it is reached
        _fused(m, "plain", x, 1001)
    m.set_option(_ffi.VA_OPT_TRAIN_STOP_AT, -1)
    _fused(m, "plain", x, 1002)
    w2 = _flat(m.export_state())
    assert not torch.equal(w2[0], w0[0]) and not torch.equal(w2[13], w0[13])  # layer 0 moves
    m.close()


# ---- 7: the pipeline ----

def test_train_videos_sets_each_streams_solver_then_takes_the_consensus_step():
    from video_analytics_amd import _ffi, augment, pipeline, vgg
    from video_analytics_amd import flow as vflow
    L, k, seed = 10, 3, 5
    vids = [_synthetic_video(25, 240, 320, seed=61), _synthetic_video(37, 240, 320, seed=63)]
    starts = [[0, 3, 14], [2, 13, 26]]
    dev = [(r.cuda(), g.cuda()) for r, g in vids]
    crops = augment.draw_scale_jitter_crops(6, 240, 320, random.Random(3))
    labels = torch.tensor([5, 77])
    solvers = (vgg.Solver(dropout=0.8), vgg.Solver(dropout=0.7, weight_decay=5e-4, freeze=13))
    kw = dict(device=0, tvl1_params=_ffi.default_tvl1_params(**SCHEDULE))
    pipe, other = pipeline.TwoStreamPipeline(**kw), pipeline.TwoStreamPipeline(**kw)
    for bad in (0.8, (solvers[0],), solvers + solvers[:1], (solvers[0], None)):
        with pytest.raises(ValueError, match="solver"):
            pipe.train_videos(dev, labels, k=k, starts=starts, crops=crops, solver=bad)
    assert pipe.spatial.solver == pipe.temporal.solver == vgg.Solver()  # refused before anything changed
    out = pipe.train_videos(dev, labels, k=k, starts=starts, crops=crops, lr=LR, momentum=MU, dropout_seed=seed, solver=solvers)
    torch.cuda.synchronize()
    assert (pipe.spatial.solver, pipe.temporal.solver) == solvers
    first, base = [], 0
    for p in out["plans"]:
        first += [base + j for j in p.index]
        base += len(p.pairs)
    rgb_table, flow_table = augment.snippet_tables(crops, list(range(6)), first, L)
    frames = torch.cat([rgb[torch.tensor(st).cuda()] for (rgb, _), st in zip(dev, starts)])
    runs = [("s", other.spatial, pipe.spatial, augment.resize_images(frames, rgb_table), solvers[0]),
            ("t", other.temporal, pipe.temporal, vflow.resize_flow_to_stack(out["flow"], flow_table).view(6, 2 * L, 224, 224), solvers[1])]
    for name, model, mine, x, sv in runs:
        w0 = _flat(model.export_state())
        model.set_solver(sv)
        stats, desc = model.train_step_consensus(x, labels.cuda(), k, LR, MU, seed)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(stats).all())
        assert torch.equal(out["stats_" + name], stats) and torch.equal(out["desc_" + name], desc), name
        now = _state(mine)
        assert _same(now, _state(model)), name
        moved = [not torch.equal(now[j], w0[j]) for j in range(34)]
        assert moved == [_layer_of(j) >= sv.freeze for j in range(34)], name
    # one Solver for every stream; None leaves them as they are
    pipe.train_videos(dev, labels, k=k, starts=starts, crops=crops, lr=LR, solver=vgg.Solver(freeze=16))
    assert pipe.spatial.solver == pipe.temporal.solver == vgg.Solver(freeze=16)
    assert pipe._check_solver(None) == []
    pipe.close()
    other.close()


# ---- 8: refusals ----

BAD_FIELDS = [
    ("weight_decay", dict(weight_decay=-1e-4)), ("weight_decay", dict(weight_decay=float("nan"))),
    ("weight_decay", dict(weight_decay=float("inf"))),
    ("bias_lr_mult", dict(bias_lr_mult=-1.0)), ("bias_lr_mult", dict(bias_lr_mult=float("inf"))),
    ("bias_lr_mult", dict(bias_lr_mult=float("nan"))),
    ("bias_decay_mult", dict(bias_decay_mult=-1.0)), ("bias_decay_mult", dict(bias_decay_mult=float("nan"))),
    ("bias_decay_mult", dict(bias_decay_mult=float("inf"))),
    ("dropout[0]", dict(dropout=(1.0, 0.5, 0.5))), ("dropout[1]", dict(dropout=(0.5, -0.1, 0.5))),
    ("dropout[2]", dict(dropout=(0.5, 0.5, float("nan")))), ("dropout[1]", dict(dropout=(0.5, 1.5, 0.5))),
    ("frozen_layers", dict(freeze=-1)), ("frozen_layers", dict(freeze=17)),
]


def test_invalid_solvers_are_refused_and_change_nothing():
    from video_analytics_amd import _ffi, vgg
    L = _ffi.lib()
    m = _stream(3)
    good = vgg.Solver(weight_decay=5e-4, bias_lr_mult=2.0, bias_decay_mult=0.0, dropout=(0.8, 0.7, 0.9), freeze=7)
    m.set_solver(good)
    assert m.solver == good
    for field, kw in BAD_FIELDS:
        with pytest.raises(ValueError):  # from Python: the host check
            m.set_solver(vgg.Solver(**kw))
        s = good.to_struct()  # from C: the same value past the host check
        for k, v in kw.items():
            if k == "dropout":
                for i in range(3):
                    s.dropout[i] = v[i]
            else:
                setattr(s, "frozen_layers" if k == "freeze" else k, v)
        assert L.va_vgg16_set_solver(m._h, ctypes.byref(s)) == _ffi.VA_ERR_INVALID, kw
        assert field in L.va_last_error().decode(), (field, L.va_last_error())
        assert m.solver == good, kw
    for bad in (None, 5e-4, dict(weight_decay=5e-4)):
        with pytest.raises(ValueError):
            m.set_solver(bad)
    assert L.va_vgg16_set_solver(m._h, None) == _ffi.VA_ERR_INVALID and m.solver == good
    m.close()
    w = _weights(3)
    half = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, dtype="bf16")
    with pytest.raises(ValueError, match="bf16"):
        half.set_solver(vgg.Solver())
    assert L.va_vgg16_set_solver(half._h, ctypes.byref(vgg.Solver().to_struct())) == _ffi.VA_ERR_INVALID
    assert half.solver == vgg.Solver()
    half.close()
