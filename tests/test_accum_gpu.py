"""Gradient accumulation, clipping and the data-parallel step on the device.

Everything here is derivable; no tolerance was measured:
  1. STORE + apply is the fused step, bit for bit (same kernels, same sums; only the finishing statement differs), and the
     stored gradient is the fused step's momentum buffer after a first step from V = 0 (fmaf(mu, 0, g) = g).
  2. ADD with exact scales: the same micro-batch twice at scale 0.5 is the fused step bit for bit (a power of two is exact
     through every product and sum unless an intermediate goes subnormal).
  3. The per-layer entry points in their STORE and ADD forms at the ``plan_wgrad`` branch shapes of
     tests/test_train_kernels_gpu.py, between canaries.
  4. A ragged batch (micro-batches of 2 and 3 images; 2 + 1 videos of 2 snippets) against torch-CPU autograd of
     ``scale_j loss_j`` + one torch.optim.SGD step, at the plain step's tolerances (tests/test_train_gpu.py).
  5. Clipping against ``clip_grad_norm_`` (evaluated in float64: its float32 norm is itself 1e-3 .. 1e-2 off on tensors of
     10^8 elements); the device norm against the float64 norm of the device's own gradient.
  6. Determinism and argument errors.
  7. ``TwoStreamPipeline.train_videos(micro_videos=)`` against the accumulate / apply calls made by hand.
  8. Two ranks on one GPU over gloo (tests/_train_dist_worker.py).
"""
import ctypes
import os
import random
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_train_gpu import TOL_UPDATE, _relerr
from test_train_kernels_gpu import CONV_CASES, _Box, _Inputs, _bits_equal, _conv_inputs, _ulp32
from test_video_gpu import SCHEDULE, _synthetic_video

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LR, MU = 1e-4, 0.9
HEADS = (3, 5)
KEYS = ("conv_w", "conv_b", "fc_w", "fc_b")

_W = {}  # (c_in, n_classes) -> CPU weights: generated once, never changed


def _weights(c_in, n_classes=101):
    from video_analytics_amd import synth, vgg
    if (c_in, n_classes) not in _W:
        w = synth.synth_vgg16_weights(c_in=3, n_classes=n_classes, seed=4)
        if c_in != 3:
            w["conv_w"][0] = vgg.copy_first_layer(w["conv_w"][0].cuda(), c_in).cpu()
        _W[(c_in, n_classes)] = w
    return _W[(c_in, n_classes)]


def _stream(c_in, n_classes=101):
    from video_analytics_amd import vgg
    w = _weights(c_in, n_classes)
    return vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], n_classes, 256)


def _x(B, c_in, seed):
    from video_analytics_amd import synth
    return torch.from_numpy(synth.hash_uniform(seed, c_in, B * c_in * 224 * 224).reshape(B, c_in, 224, 224) * 4.0 - 2.0)


def _state(m):
    """The 34 parameters, then the 34 momentum buffers, on the device."""
    st, mo = m.export_state(), m.export_state(momentum=True)
    return [t for d in (st, mo) for k in KEYS for t in d[k]]


def _flat(d):
    return [t for k in KEYS for t in d[k]]


def _same(a, b):
    return len(a) == len(b) and all(_bits_equal(u, v) for u, v in zip(a, b))


@pytest.fixture(autouse=True)
def training_workspaces_released():
    """Pipelines keep their streams' training workspaces in slots of their own; tests/test_train_gpu.py expects to find one."""
    yield
    from video_analytics_amd import vgg
    torch.cuda.synchronize()
    for key in [key for key in vgg._ws_cache if "train" in str(key)]:
        del vgg._ws_cache[key]


# form -> (n_classes, images, k, labels, tasks, heads)
FORMS = {
    "plain": (101, 2, 0, [1, 8], None, None),
    "consensus": (101, 4, 2, [1, 8], None, None),
    "multitask": (8, 4, 2, [1, 3], [0, 1], HEADS),
}


def _fused(m, form, x, seed):
    _, _, k, labels, tasks, heads = FORMS[form]
    y = torch.tensor(labels, dtype=torch.int64).cuda()
    if form == "plain":
        return m.train_step(x, y, LR, MU, seed)
    if form == "consensus":
        return m.train_step_consensus(x, y, k, LR, MU, seed)
    return m.train_step_multitask(x, y, torch.tensor(tasks, dtype=torch.int32).cuda(), heads, k, LR, MU, seed)


def _accumulate(m, form, x, seed, scales, first):
    _, _, k, labels, tasks, heads = FORMS[form]
    y = torch.tensor(labels, dtype=torch.int64).cuda()
    t = None if tasks is None else torch.tensor(tasks, dtype=torch.int32).cuda()
    return m.train_accumulate(x, y, k=k, tasks=t, heads=heads, scales=scales, first=first, dropout_seed=seed)


# ---- 1: STORE + apply is the fused step ----

@pytest.mark.parametrize("c_in", [3, 20])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_store_then_apply_is_the_fused_step(form, c_in):
    n_classes, B = FORMS[form][:2]
    a, b = _stream(c_in, n_classes), _stream(c_in, n_classes)
    for r in range(2):
        x = _x(B, c_in, 80 + r).cuda()
        sf, df = _fused(a, form, x, 1000 + r)
        sa, da = _accumulate(b, form, x, 1000 + r, None, True)
        if r == 0:  # V = 0 before the first step: the fused step's momentum buffer IS the gradient
            assert _same(_flat(b.export_grad()), _flat(a.export_state(momentum=True))), (form, c_in, "gradient")
        assert b.train_apply(LR, MU) is None
        assert _bits_equal(sf, sa) and _bits_equal(df, da), (form, c_in, r, sf, sa)
        assert bool(torch.isfinite(sa).all())
        assert _same(_state(a), _state(b)), (form, c_in, r, "state")
    a.close()
    b.close()


# ---- 2: ADD with exact scales ----

@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_same_micro_batch_twice_at_half_scale_is_the_fused_step(form):
    """G = g/2 (STORE), then G + g/2 (ADD): every product and sum of the backward pass scales by 2^-1 exactly, so G = g."""
    n_classes, B = FORMS[form][:2]
    a, b = _stream(3, n_classes), _stream(3, n_classes)
    x = _x(B, 3, 83).cuda()
    sf, df = _fused(a, form, x, 1003)
    half = 0.5 if form != "multitask" else [0.5, 0.5]
    s0, d0 = _accumulate(b, form, x, 1003, half, True)
    s1, d1 = _accumulate(b, form, x, 1003, half, False)
    b.train_apply(LR, MU)
    assert _bits_equal(sf, s0) and _bits_equal(sf, s1) and _bits_equal(df, d0) and _bits_equal(df, d1)  # the loss is not scaled
    assert _same(_state(a), _state(b)), form
    a.close()
    b.close()


# ---- 3: the per-layer entry points ----

@pytest.mark.parametrize("cid", sorted(CONV_CASES))
def test_conv_layer_store_and_add_forms(cid):
    from video_analytics_amd import vgg
    case = CONV_CASES[cid]
    inp = _conv_inputs(case, seed=sum(map(ord, cid)))
    B, hw, cout, cin, cin_pad = case["B"], case["hw"], case["cout"], case["cin"], case["cin_pad"]
    I = _Inputs(dy=inp["dy"], x=inp["x"], mask=inp["mask"], w=inp["w"], zeros=torch.zeros(max(512, cin)))
    sizes, _ = vgg.train_conv_backward_scratch(B, hw, cin, cin_pad, cout)
    g = torch.Generator().manual_seed(7)
    g0w, g0b = torch.randn(cout, 9, cin_pad, generator=g).cuda(), torch.randn(cout, generator=g).cuda()

    def run(mode):
        """mode: "sgd" (from V = 0), "store", "add" (onto g0) -> (gradient-like w, b, dx, plan)"""
        W = _Box(inp["w"].shape, inp["w"])
        Bi = _Box((cout,), inp["b"])
        Gw = _Box(inp["w"].shape, {"sgd": torch.zeros_like(g0w), "store": None, "add": g0w}[mode])
        Gb = _Box((cout,), {"sgd": torch.zeros_like(g0b), "store": None, "add": g0b}[mode])
        dx = _Box((B, hw, hw, cin)) if case["dx"] else None
        scratch = tuple(_Box((n,)) for n in sizes)
        kw = dict(dx=dx.t if dx else None, mask=I.mask if dx else None, zeros=I.zeros, scratch=tuple(s.t for s in scratch))
        if mode == "sgd":
            plan = vgg.train_conv_backward_layer(I.dy, I.x, W.t, Bi.t, Gw.t, Gb.t, LR, MU, cin, **kw)
        else:
            plan = vgg.train_conv_backward_layer_grad(I.dy, I.x, I.w, Gw.t, Gb.t, cin, mode == "add", **kw)
        torch.cuda.synchronize()
        I.check((cid, mode))
        for name, box in (("grad_w", Gw), ("grad_b", Gb), ("slab", scratch[0]), ("bpart", scratch[2]), ("W", W), ("bias", Bi)):
            box.check((cid, mode, name))
        scratch[1].check((cid, mode, "wt"), finite=bool(dx))
        if dx:
            dx.check((cid, mode, "dx"))
        return Gw.t.clone(), Gb.t.clone(), dx.t.clone() if dx else None, plan

    vw, vb, dx_s, plan_s = run("sgd")
    gw, gb, dx_g, plan_g = run("store")
    aw, ab, dx_a, plan_a = run("add")
    assert plan_s == plan_g == plan_a, (plan_s, plan_g, plan_a)
    assert _bits_equal(gw, vw) and _bits_equal(gb, vb), (cid, "STORE is not the momentum buffer of the SGD form from V = 0")
    assert _bits_equal(aw, g0w + gw) and _bits_equal(ab, g0b + gb), (cid, "ADD is not the float32 G0 + g")
    if case["dx"]:
        assert _bits_equal(dx_s, dx_g) and _bits_equal(dx_s, dx_a), (cid, "dx")


@pytest.mark.parametrize("O,I_,B", [(101, 256, 2), (130, 100, 33), (256, 4096, 64), (1, 64, 1)])
def test_fc_layer_store_and_add_forms(O, I_, B):
    from video_analytics_amd import vgg
    g = torch.Generator().manual_seed(1000 * O + I_ + B)
    w, b = torch.randn(O, I_, generator=g) / I_ ** 0.5, torch.randn(O, generator=g) * 0.5
    dz, x = torch.randn(B, O, generator=g), torch.randn(B, I_, generator=g).clamp_min(0.0) * 2.0
    mask = torch.randn(B, I_, generator=g)
    g0w, g0b = torch.randn(O, I_, generator=g).cuda(), torch.randn(O, generator=g).cuda()
    In = _Inputs(dz=dz, x=x, mask=mask, w=w)

    def run(mode):
        W, Bi = _Box(w.shape, w), _Box(b.shape, b)
        Gw = _Box(w.shape, {"sgd": torch.zeros_like(g0w), "store": None, "add": g0w}[mode])
        Gb = _Box(b.shape, {"sgd": torch.zeros_like(g0b), "store": None, "add": g0b}[mode])
        dx = _Box((B, I_))
        if mode == "sgd":
            name = vgg.train_fc_backward_layer(In.dz, In.x, W.t, Bi.t, Gw.t, Gb.t, LR, MU, dx.t, mask=In.mask, scale=2.0)
        else:
            name = vgg.train_fc_backward_layer_grad(In.dz, In.x, In.w, Gw.t, Gb.t, mode == "add", dx.t, mask=In.mask, scale=2.0)
        torch.cuda.synchronize()
        In.check((O, I_, B, mode))
        for nm, box in (("grad_w", Gw), ("grad_b", Gb), ("dx", dx), ("W", W), ("bias", Bi)):
            box.check((O, I_, B, mode, nm))
        return Gw.t.clone(), Gb.t.clone(), dx.t.clone(), name

    vw, vb, dx_s, n_s = run("sgd")
    gw, gb, dx_g, n_g = run("store")
    aw, ab, dx_a, n_a = run("add")
    assert n_s == n_g == n_a == ("k_fc_dx<32>" if B <= 32 else "k_fc_dx<64>")
    assert _bits_equal(gw, vw) and _bits_equal(gb, vb)
    assert _bits_equal(aw, g0w + gw) and _bits_equal(ab, g0b + gb)
    assert _bits_equal(dx_s, dx_g) and _bits_equal(dx_s, dx_a)


# ---- 4, 5: a ragged batch, with and without clipping, against autograd ----

RAGGED = {"plain": (0, [(0, 2), (2, 5)], 5), "consensus": (2, [(0, 2), (2, 3)], 3)}  # form -> (k, micro-batches in videos, n)
_ragged = {}  # form -> everything both tests look at: computed once, never changed
# Conditioning of the inputs, judged by the ORACLE alone: backward passes through the forward pass's decisions, and a hidden
# classifier unit that Dropout keeps and whose pre-activation lies within float32 rounding of zero is open in one correct fp32
# forward pass and shut in another; its whole row of the layer's weight update then differs (tests/test_train_gpu.py's header
# describes the same for the conv stack, where TOL_UPDATE absorbs it).  Input stream 90 has such a unit in FC1 of the second
# consensus micro-batch: |z| = 7.1e-6 in the oracle, beside a layer maximum of 17 and a second-smallest of 2e-4.  On those two
# images the FUSED step itself (va_vgg16_train_step_consensus, n = 1, k = 2) is 0.22 of FC1's largest update away from autograd
# and 2e-2 .. 3.5e-2 on every conv tensor, so nothing about accumulation is learnt there.  FC1 adds 25 088 products of
# magnitude about 1: float32 rounding of such a sum is about sqrt(25088) 2^-24 = 1e-5.  The test therefore requires every kept
# unit of the three hidden layers to be at least ten times that, 1e-4, away from zero IN THE ORACLE, and uses input stream 93,
# the first of 90 .. 93 that the oracle says is (smallest kept |z|: 7.1e-4, 1.4e-3 and 1.9e-2 in the three layers).
RAGGED_INPUT, MIN_MARGIN = 93, 1e-4


def _oracle_backward(params, x, labels, k, seed, scale):
    """scale * loss of one micro-batch, back-propagated into params' .grad (accumulating) -> (loss, hits, margin): margin =
    the smallest |pre-activation| of a hidden classifier unit that Dropout keeps (MIN_MARGIN)"""
    from oracle import train_oracle, vgg_oracle
    feat = vgg_oracle.features(x, params["conv_w"], params["conv_b"])
    op = feat.reshape(feat.size(0), -1)
    margin = float("inf")
    for l in range(3):
        z = F.linear(op, params["fc_w"][l], params["fc_b"][l])
        mask = train_oracle.dropout_mask(seed, l, tuple(z.shape))
        margin = min(margin, float(z.detach()[mask > 0].abs().min()))
        op = F.relu(z) * mask
    logits = F.linear(op, params["fc_w"][3], params["fc_b"][3])
    if k:
        logits = logits.view(-1, k, logits.shape[-1]).mean(1)
    loss = F.cross_entropy(logits, labels)
    (scale * loss).backward()
    return float(loss.detach()), int((logits.argmax(1) == labels).sum()), margin


def _ragged_run(form):
    if form in _ragged:
        return _ragged[form]
    from video_analytics_amd import vgg
    torch.set_num_threads(8)
    k, slices, n = RAGGED[form]
    kk = max(k, 1)
    w = _weights(3)
    x = _x(n * kk, 3, RAGGED_INPUT)
    labels = torch.tensor([(7 * i + 1) % 101 for i in range(n)], dtype=torch.int64)
    scales = vgg.micro_scales(slices)
    assert scales == ([[2 / 5], [3 / 5]] if form == "plain" else [[2 / 3], [1 / 3]])
    # the oracle: scale_j loss_j back-propagated per micro-batch, then one SGD step (twice: unclipped, clipped to half its norm)
    params = {key: [t.clone().requires_grad_(True) for t in v] for key, v in w.items()}
    flat = _flat(params)
    loss_r = hits_r = 0.0
    for j, (lo, hi) in enumerate(slices):
        l, h, margin = _oracle_backward(params, x[lo * kk:hi * kk], labels[lo:hi], k, 3000 + j, scales[j][0])
        assert margin >= MIN_MARGIN, (form, j, margin, "the oracle finds this input ill-conditioned: see MIN_MARGIN")
        loss_r += scales[j][0] * l
        hits_r += h
    grads = [p.grad.clone() for p in flat]
    norm_r = float(torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads)))

    def sgd(clip):
        """torch.optim.SGD on the float32 parameters; ``clip_grad_norm_`` is evaluated on float64 copies of the float32
        gradients and its result rounded to float32.  On float32 tensors it adds the squares in float32: on the 102.8 M
        elements of FC1 alone that norm came out 1.15 % low on a CPU (randn x 1e-2), and 0.15 % off on this case's gradient
        -- the reference's own error, three times the classifier tolerance, and the same factor on every tensor."""
        ps = [p.detach().clone().requires_grad_(True) for p in flat]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        if clip is not None:
            ps64 = [p.detach().double().requires_grad_(True) for p in flat]
            for p, gr in zip(ps64, grads):
                p.grad = gr.double()
            total = torch.nn.utils.clip_grad_norm_(ps64, clip)
            assert abs(float(total) - norm_r) <= 1e-9 * norm_r
            for p, q in zip(ps, ps64):
                p.grad = q.grad.float()
        torch.optim.SGD(ps, LR, momentum=MU).step()
        return [p.detach() for p in ps]
    ref_plain, ref_clip = sgd(None), sgd(0.5 * norm_r)
    # the device
    m = _stream(3)
    stats = []
    for j, (lo, hi) in enumerate(slices):
        st, _ = m.train_accumulate(x[lo * kk:hi * kk].cuda(), labels[lo:hi].cuda(), k=k, scales=scales[j], first=(j == 0),
                                   dropout_seed=3000 + j)
        stats.append(st)
    stats = vgg.combine_micro_stats(stats, scales).cpu()
    gdev = _flat(m.export_grad())
    norm_own = float(torch.sqrt(sum((t.double() ** 2).sum() for t in gdev)))
    out = dict(loss_r=loss_r, hits_r=hits_r, norm_r=norm_r, stats=stats, norm_own=norm_own, w0=_flat(w), ref_plain=ref_plain,
               ref_clip=ref_clip)
    for name, clip in (("plain", None), ("clip", 0.5 * norm_r), ("clip10", 10.0 * norm_r)):
        m.import_state(w)
        m.train_init()  # momentum buffers back to zero
        norm = m.train_apply(LR, MU, clip)
        out["got_" + name] = [t.cpu() for t in _flat(m.export_state())]
        out["norm_" + name] = None if norm is None else float(norm.cpu()[0])
    m.close()
    _ragged[form] = out
    return out


def _check_updates(got, ref, w0, what):
    worst = []
    for i, (g_, r, o) in enumerate(zip(got, ref, w0)):
        worst.append((_relerr(g_ - o, r - o), i))
    print(what, "worst update error %.3g (tensor %d); classifier %.3g" % (max(worst) + (max(worst[26:])[0],)))
    assert max(worst[:26])[0] < TOL_UPDATE, (what, max(worst[:26]))  # _flat: 13 conv weights, 13 conv biases, then the classifier
    assert max(worst[26:])[0] < 5e-4, (what, max(worst[26:]))


@pytest.mark.parametrize("form", sorted(RAGGED))
def test_ragged_batch_against_autograd(form):
    r = _ragged_run(form)
    print(form, "loss", float(r["stats"][0]), r["loss_r"], "hits", float(r["stats"][1]), r["hits_r"])
    assert abs(float(r["stats"][0]) - r["loss_r"]) < 2e-4 * max(1.0, abs(r["loss_r"]))
    assert float(r["stats"][1]) == r["hits_r"]
    assert r["norm_plain"] is None
    _check_updates(r["got_plain"], r["ref_plain"], r["w0"], (form, "unclipped"))


@pytest.mark.parametrize("form", sorted(RAGGED))
def test_clipping_against_autograd(form):
    r = _ragged_run(form)
    print(form, "norm: device %.17g, float64 of the device's gradient %.17g, oracle %.17g" % (r["norm_clip"], r["norm_own"], r["norm_r"]))
    _check_updates(r["got_clip"], r["ref_clip"], r["w0"], (form, "clipped to half the norm"))
    # 135 M terms x 2^-53 = 1.5e-8 for ANY summation order of exact squares: 1e-7 relative
    for name in ("norm_clip", "norm_clip10"):
        assert abs(r[name] - r["norm_own"]) <= 1e-7 * r["norm_own"], (name, r[name], r["norm_own"])
    moved = max(float((a - b).abs().max()) for a, b in zip(r["got_clip"], r["got_plain"]))
    assert moved > 0.0  # the coefficient near 0.5 did something
    for a, b in zip(r["got_clip10"], r["got_plain"]):  # coefficient min(1, 10) = 1
        assert bool(((a.double() - b.double()).abs() <= _ulp32(b.double())).all())


# ---- 6: determinism and errors ----

def test_two_runs_give_identical_bits():
    m = _stream(3)
    x0, x1 = _x(2, 3, 91).cuda(), _x(3, 3, 92).cuda()
    y0, y1 = torch.tensor([4, 9]).cuda(), torch.tensor([0, 100, 17]).cuda()
    w = _weights(3)
    runs = []
    for _ in range(2):
        m.import_state(w)
        m.train_init()
        m.train_accumulate(x0, y0, scales=0.4, first=True, dropout_seed=5)
        m.train_accumulate(x1, y1, scales=0.6, first=False, dropout_seed=6)
        g = m.grad().clone()
        norm = m.train_apply(LR, MU, 0.05)
        runs.append([g, norm.clone()] + _state(m))
    assert float(runs[0][1]) > 0.05  # the clip was active
    assert torch.equal(runs[0][1], runs[1][1]) and _same(runs[0][:1] + runs[0][2:], runs[1][:1] + runs[1][2:])
    off, cnt = m.grad_layout()
    assert len(off) == 34 and all(o % 64 == 0 for o in off) and all(off[i] + cnt[i] <= off[i + 1] for i in range(33))
    assert off[33] + cnt[33] <= m.grad().numel() < off[33] + cnt[33] + 64
    g = runs[0][0]
    for i in range(34):  # the gaps hold zeros
        end = off[i + 1] if i < 33 else g.numel()
        assert not bool(g[off[i] + cnt[i]:end].any()), i
    m.close()


def test_argument_errors_write_nothing():
    from video_analytics_amd import _ffi, vgg
    L = _ffi.lib()
    m = _stream(3, 8)
    m.train_init()
    before = _state(m)
    n_grad = int(L.va_vgg16_train_grad_floats(m._h))
    assert n_grad == m.grad().numel() and n_grad > 134_000_000
    nan = float("nan")
    grad = torch.full((n_grad + 4,), nan, device="cuda")
    x = _x(4, 3, 93).cuda()
    labels, tasks = torch.tensor([1, 2, 0, 1]).cuda(), torch.tensor([0, 1, 0, 1], dtype=torch.int32).cuda()
    desc, loss = torch.full((4, 256), nan, device="cuda"), torch.full((6,), nan, device="cuda")
    ws = torch.empty(L.va_vgg16_train_workspace_bytes(m._h, 4), dtype=torch.uint8, device="cuda")
    heads, one, f32 = (ctypes.c_int * 2)(3, 5), (ctypes.c_float * 2)(1.0, 1.0), ctypes.c_float * 2
    sp = _ffi.stream_ptr(m.device)

    def acc(x=x, labels=labels, tasks=tasks, n=2, k=2, n_heads=2, head_sizes=heads, scales=one, g=grad, ng=n_grad, ws=ws, nws=None):
        return L.va_vgg16_train_accumulate(m._h, _ffi.ptr(x), 0, _ffi.ptr(labels), _ffi.ptr(tasks), n, k, n_heads, head_sizes, scales, 1, 7,
                                           _ffi.ptr(desc), _ffi.ptr(loss), _ffi.ptr(g), ng, _ffi.ptr(ws),
                                           (ws.numel() if ws is not None else 0) if nws is None else nws, sp)

    def app(g=grad, ng=n_grad, lr=LR, clip=1.0, ws=ws, nws=None):
        return L.va_vgg16_train_apply(m._h, _ffi.ptr(g), ng, lr, MU, clip, None, _ffi.ptr(ws), (ws.numel() if ws is not None else 0) if nws is None else nws, sp)
    bad = [acc(n=0), acc(n=33, k=2), acc(k=-1), acc(k=0), acc(ng=n_grad - 1), acc(g=grad[1:]), acc(g=None), acc(x=None), acc(labels=None),
           acc(scales=None), acc(scales=f32(1.0, nan)), acc(scales=f32(float("inf"), 1.0)), acc(head_sizes=(ctypes.c_int * 2)(3, 4)),
           acc(head_sizes=None), acc(n_heads=9), acc(tasks=None), acc(nws=ws.numel() - 1), acc(ws=None),
           app(g=None), app(ng=n_grad - 1), app(g=grad[1:]), app(lr=nan), app(clip=nan), app(nws=8), app(ws=None)]
    torch.cuda.synchronize()
    assert all(rc in (_ffi.VA_ERR_INVALID, _ffi.VA_ERR_WORKSPACE) for rc in bad), bad
    assert bool(torch.isnan(grad).all()) and bool(torch.isnan(desc).all()) and bool(torch.isnan(loss).all())
    assert _same(before, _state(m))
    # the Python surface
    xs = x[:2]
    for kw in (dict(tasks=tasks[:1]), dict(heads=HEADS), dict(k=-1), dict(k=3), dict(scales=[1.0, 2.0]), dict(scales=nan),
               dict(tasks=tasks[:2], heads=HEADS, k=0), dict(tasks=tasks[:2], heads=(3, 4), k=1)):
        with pytest.raises(ValueError):
            m.train_accumulate(xs, labels[:2], first=True, dropout_seed=0, **kw)
    with pytest.raises(ValueError, match="out of bounds"):
        m.train_accumulate(xs, torch.tensor([1, 8]), first=True, dropout_seed=0)
    for clip in (0.0, -1.0, nan, float("inf"), "1", True):
        with pytest.raises(ValueError):
            m.train_apply(LR, MU, clip)
    fresh = _stream(3, 8)
    with pytest.raises(ValueError, match="nothing was accumulated"):
        fresh.train_apply(LR, MU)
    with pytest.raises(ValueError, match="nothing was accumulated"):
        fresh.export_grad()
    fresh.close()
    assert _same(before, _state(m))
    # bad labels / tasks already on the device: nothing out of bounds, a NaN loss
    st, _ = m.train_accumulate(xs, torch.tensor([1, 8]).cuda(), first=True, dropout_seed=0)
    assert bool(torch.isnan(st[0]))
    st, _ = m.train_accumulate(x, labels[:2], k=2, tasks=torch.tensor([0, 2], dtype=torch.int32).cuda(), heads=HEADS, first=True, dropout_seed=0)
    assert bool(torch.isnan(st[0]))
    assert _same(before, _state(m))
    m.close()


# ---- 7: the pipeline ----

def _three_videos():
    vids = [_synthetic_video(25, 240, 320, seed=s) for s in (61, 63, 65)]
    return [(r.cuda(), g.cuda()) for r, g in vids], [[0, 14], [3, 12], [5, 9]]


@pytest.mark.parametrize("heads,rgb_diff", [(None, False), ((51, 101), False), (None, True)], ids=["plain", "heads", "rgbdiff"])
def test_train_videos_with_micro_batches_is_the_accumulate_calls_by_hand(heads, rgb_diff):
    from video_analytics_amd import _ffi, augment, pipeline, rgbdiff, vgg
    from video_analytics_amd import flow as vflow
    L, k, seed, clip = 10, 2, 5, 0.05
    dev, starts = _three_videos()
    crops = augment.draw_scale_jitter_crops(6, 240, 320, random.Random(3))
    labels = torch.tensor([50, 77, 3])
    tasks = None if heads is None else [0, 1, 1]
    kw = dict(device=0, tvl1_params=_ffi.default_tvl1_params(**SCHEDULE), heads=heads, rgb_diff=rgb_diff)
    pipe, other = pipeline.TwoStreamPipeline(**kw), pipeline.TwoStreamPipeline(**kw)
    more = {} if tasks is None else dict(tasks=tasks)
    out = pipe.train_videos(dev, labels, k=k, starts=starts, crops=crops, lr=LR, momentum=MU, dropout_seed=seed, micro_videos=2,
                            clip_norm=clip, **more)
    torch.cuda.synchronize()
    first, base = [], 0
    for p in out["plans"]:
        first += [base + j for j in p.index]
        base += len(p.pairs)
    rgb_table, flow_table = augment.snippet_tables(crops, list(range(6)), first, L)
    frames = torch.cat([rgb[torch.tensor(st).cuda()] for (rgb, _), st in zip(dev, out["starts"])])
    runs = [("s", other.spatial, pipe.spatial, augment.resize_images(frames, rgb_table)),
            ("t", other.temporal, pipe.temporal, vflow.resize_flow_to_stack(out["flow"], flow_table).view(6, 2 * L, 224, 224))]
    if rgb_diff:
        D = pipe.D
        win = torch.cat([rgb[torch.tensor([s + f for s in st for f in range(D + 1)]).cuda()] for (rgb, _), st in zip(dev, out["starts"])])
        runs.append(("d", other.diff, pipe.diff, rgbdiff.rgb_diff_stack(win, rgbdiff.window_table([i * (D + 1) for i in range(6)], crops), D)))
    slices = vgg.micro_slices(3, 2)
    H = 0 if heads is None else len(heads)
    scales = vgg.micro_scales(slices, 3, tasks, H)
    assert slices == [(0, 2), (2, 3)] and scales == ([[2 / 3], [1 / 3]] if heads is None else [[1.0, 0.5], [0.0, 0.5]])
    y = labels.cuda()
    t = None if tasks is None else torch.tensor(tasks, dtype=torch.int32).cuda()
    for name, model, mine, x in runs:
        stats, descs = [], []
        for j, (lo, hi) in enumerate(slices):
            st, d = model.train_accumulate(x[lo * k:hi * k], y[lo:hi], k=k, tasks=None if t is None else t[lo:hi], heads=heads,
                                           scales=scales[j], first=(j == 0), dropout_seed=seed + j)
            stats.append(st)
            descs.append(d)
        norm = model.train_apply(LR, MU, clip)
        stats = vgg.combine_micro_stats(stats, scales, H)
        torch.cuda.synchronize()
        assert tuple(stats.shape) == (2 + 2 * H,) and bool(torch.isfinite(stats).all()) and float(stats[0]) > 0
        assert _bits_equal(out["stats_" + name], stats), (name, out["stats_" + name], stats)
        assert _bits_equal(out["desc_" + name], torch.cat(descs)), name
        assert torch.equal(out["norm_" + name], norm) and float(norm) > clip, (name, norm)
        assert _same(_state(mine), _state(model)), name
    pipe.close()
    other.close()


def test_train_videos_with_defaults_takes_the_fused_step():
    from video_analytics_amd import _ffi, augment, pipeline
    dev, starts = _three_videos()
    crops = augment.draw_scale_jitter_crops(6, 240, 320, random.Random(3))
    labels = torch.tensor([50, 77, 3])
    kw = dict(device=0, tvl1_params=_ffi.default_tvl1_params(**SCHEDULE))
    pipe, other = pipeline.TwoStreamPipeline(**kw), pipeline.TwoStreamPipeline(**kw)
    args = dict(k=2, starts=starts, crops=crops, lr=LR, momentum=MU, dropout_seed=5)
    a = pipe.train_videos(dev, labels, micro_videos=None, clip_norm=None, data_parallel=False, **args)
    b = other.train_videos(dev, labels, **args)
    torch.cuda.synchronize()  # (tests/test_tsn_gpu.py holds the fused train_videos to the consensus step called by hand)
    assert sorted(a) == sorted(b) and "norm_s" not in a
    for key in ("stats_s", "stats_t", "desc_s", "desc_t", "flow"):
        assert _bits_equal(a[key], b[key]), key
    assert _same(_state(pipe.spatial), _state(other.spatial)) and _same(_state(pipe.temporal), _state(other.temporal))
    with pytest.raises(ValueError, match="n\\*k in 1..64"):
        pipe.train_videos(dev * 11, labels.repeat(11), k=2)  # 66 images: still refused without micro_videos
    pipe.close()
    other.close()


# ---- 8: two ranks on one GPU ----

def test_two_ranks_agree_with_one_process():
    """Two ranks on device 0 over gloo (RCCL refuses two ranks on one device; the all-reduce call is the same), started by
    the project's own launcher: tests/_train_dist_worker.py.
      * Stream level: two ranks with identical weights each accumulate a different 2-image micro-batch at scale 1/2,
        all-reduce and apply with clipping; both ranks' 68 state tensors are equal to each other and, bit for bit, to one
        process that accumulated the two micro-batches (STORE, then ADD).  The all-reduce adds TWO terms, g0 + g1, and a
        float sum of two terms is commutative, so no summation order separates the ranks from the single process.
      * Pipeline level: ``train_videos(data_parallel=True)`` with one video per rank equals the single-process
        ``micro_videos=1`` run of both videos.
    The worker exits non-zero on any difference.  The one slow test of this file: 5.7 s of wall time on the MI355X (two
    processes that each import torch, build a stream and a pipeline, and stage 539 MB gradients through the host four times)."""
    from video_analytics_amd import launch
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(VA_DIST_BACKEND="gloo", VA_FORCE_DEVICE="0")
    t0 = time.time()
    rc = launch.spawn_ranks([sys.executable, os.path.join(ROOT, "tests", "_train_dist_worker.py")], 2, env=env, timeout=600)
    print("two ranks: %.1f s" % (time.time() - t0))
    assert rc == 0
