"""Gradient accumulation, host side: a numpy float32 restatement of scale, ADD, clip and apply against
float64 torch.optim.SGD(momentum) + clip_grad_norm_; the micro-batch slicing and scales at known answers; every ValueError
of the new arguments with all paths to the device blocked; ``dist.all_reduce_gradients`` at gloo world 2 on CPU tensors.
tests/test_accum_gpu.py runs the kernels."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


# ---- the arithmetic of S29 / S30, restated in float32 ----

def accumulate_f32(micro_grads, scales):
    """G = s_0 g_0 (STORE), then G = G + s_j g_j (ADD, one rounding).  On the device the scale enters at the logits and the
    backward pass is linear in it; here it multiplies the finished micro-batch gradient, the same number up to rounding."""
    G = None
    for g, s in zip(micro_grads, scales):
        t = (np.float32(s) * g.astype(np.float32)).astype(np.float32)
        G = t if G is None else (G + t).astype(np.float32)
    return G


def norm_f64(tensors):
    """Two-stage float64 sum of squares in a fixed order (any order is within n 2^-53 of any other), then the root."""
    parts = [np.sum(t.astype(np.float64) ** 2) for t in tensors]
    return float(np.sqrt(np.sum(np.array(parts, dtype=np.float64))))


def apply_f32(W, V, G, lr, mu, clip):
    """V = fmaf(mu, V, c G); W = fmaf(-lr, V, W); c = min(1, clip / (norm + 1e-6)) or absent.  The fused multiply-adds are
    formed in float64 and rounded once (exact for float32 operands: a 48-bit product plus a float32 fits 53 bits whenever the
    exponents are within 5 binades, and is within half an ulp of float32 otherwise)."""
    c = None
    if clip is not None:
        cc = clip / (norm_f64(G) + 1e-6)
        c = np.float32(cc) if cc < 1.0 else np.float32(1.0)
    Wn, Vn = [], []
    for w, v, g in zip(W, V, G):
        gg = g if c is None else (c * g).astype(np.float32)
        nv = (np.float64(np.float32(mu)) * v.astype(np.float64) + gg.astype(np.float64)).astype(np.float32)
        nw = (-np.float64(np.float32(lr)) * nv.astype(np.float64) + w.astype(np.float64)).astype(np.float32)
        Vn.append(nv)
        Wn.append(nw)
    return Wn, Vn, c


@pytest.mark.parametrize("clip_factor", [None, 0.5, 0.03, 10.0], ids=["noclip", "c=0.5", "c=0.03", "c>1"])
def test_the_float32_restatement_against_float64_sgd_with_clipping(clip_factor):
    """Three parameter tensors, three ragged micro-batches, two steps (the second one exercises the momentum term): the
    float32 restatement stays within a few float32 roundings of float64 torch.optim.SGD + clip_grad_norm_."""
    rng = np.random.RandomState(3)
    shapes = [(7, 5), (13,), (3, 4, 2)]
    lr, mu = 1e-2, 0.9
    W = [rng.randn(*s).astype(np.float32) for s in shapes]
    V = [np.zeros(s, dtype=np.float32) for s in shapes]
    ps = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in W]
    opt = torch.optim.SGD(ps, lr=float(np.float32(lr)), momentum=float(np.float32(mu)))
    scales = [2 / 7, 3 / 7, 2 / 7]
    err_v = [np.zeros(s) for s in shapes]  # running bounds on |float32 - float64|, from the roundings counted below
    err_w = [np.zeros(s) for s in shapes]
    for step in range(2):
        micro = [[rng.randn(*s).astype(np.float32) for s in shapes] for _ in scales]
        G = [accumulate_f32([m[i] for m in micro], scales) for i in range(len(shapes))]
        exact = [sum(np.float64(np.float32(s)) * m[i].astype(np.float64) for m, s in zip(micro, scales)) for i in range(len(shapes))]
        mag = [sum(np.float64(np.float32(s)) * np.abs(m[i]).astype(np.float64) for m, s in zip(micro, scales)) for i in range(len(shapes))]
        for g, e, a in zip(G, exact, mag):  # three rounded products, two rounded sums: each at most 2^-24 of the magnitude sum
            assert np.all(np.abs(g - e) <= 5 * U * a)
        norm = norm_f64(exact)
        clip = None if clip_factor is None else clip_factor * norm
        for p, e in zip(ps, exact):
            p.grad = torch.tensor(e)
        if clip is not None:
            total = torch.nn.utils.clip_grad_norm_(ps, clip)
            assert abs(float(total) - norm) <= 1e-12 * norm
        opt.step()
        W, V, c = apply_f32(W, V, G, lr, mu, clip)
        cr = 1.0 if clip_factor is None else min(1.0, clip_factor)
        if clip_factor is not None:
            assert abs(float(c) - cr) < 1e-5 and ((clip_factor < 1) == (float(c) < 1.0))
        for i, (w, p, v) in enumerate(zip(W, ps, V)):
            ref_v, ref_w = opt.state[p]["momentum_buffer"].numpy(), p.detach().numpy()
            # G's five roundings, the norm of G in the place of the exact gradient's (relative 5 U), c and c G rounded, then the fused
            # multiply-add's one rounding of V; the same for W.  Twice the sum, so that no constant is tuned.
            err_v[i] = mu * err_v[i] + cr * (5 * U * mag[i]) + 7 * U * cr * np.abs(exact[i]) + U * np.abs(ref_v)
            err_w[i] = err_w[i] + lr * err_v[i] + U * np.abs(ref_w)
            assert np.all(np.abs(v - ref_v) <= 2 * err_v[i]), (step, float((np.abs(v - ref_v) / err_v[i]).max()))
            assert np.all(np.abs(w - ref_w) <= 2 * err_w[i]), (step, float((np.abs(w - ref_w) / err_w[i]).max()))
    if clip_factor == 10.0:  # a coefficient above 1 is 1: the clipped update is the unclipped one
        W2, V2, _ = apply_f32(W, V, G, lr, mu, None)
        W3, V3, c3 = apply_f32(W, V, G, lr, mu, 10.0 * norm_f64(G))
        assert float(c3) == 1.0 and all(np.array_equal(a, b) for a, b in zip(W2 + V2, W3 + V3))


# ---- slicing and scales: known answers ----

def test_micro_slices_and_scales_have_their_known_answers():
    from video_analytics_amd import vgg
    assert vgg.micro_slices(7, 3) == [(0, 3), (3, 6), (6, 7)]
    assert vgg.micro_slices(6, 3) == [(0, 3), (3, 6)] and vgg.micro_slices(2, 8) == [(0, 2)] and vgg.micro_slices(1, 1) == [(0, 1)]
    for bad in ((0, 3), (3, 0), (-1, 2)):
        with pytest.raises(ValueError):
            vgg.micro_slices(*bad)
    s = vgg.micro_scales(vgg.micro_slices(7, 3))
    assert s == [[3 / 7], [3 / 7], [1 / 7]] and abs(sum(x[0] for x in s) - 1.0) < 1e-15
    assert vgg.micro_scales([(0, 2)], n_total=8) == [[0.25]]  # a rank's shard of a data-parallel batch of 8
    # per head: the head's videos in the slice over its videos in the batch
    tasks = [0, 1, 1, 0, 1, 2, 1]
    s = vgg.micro_scales(vgg.micro_slices(7, 3), tasks=tasks, n_heads=4)
    assert s == [[1 / 2, 2 / 4, 0.0, 0.0], [1 / 2, 1 / 4, 1.0, 0.0], [0.0, 1 / 4, 0.0, 0.0]]
    for h in range(3):
        assert abs(sum(row[h] for row in s) - 1.0) < 1e-15
    assert all(row[3] == 0.0 for row in s)  # a head absent from the whole batch: 0, and its gradient is exactly zero anyway
    # totals over all ranks
    assert vgg.micro_scales([(0, 2)], tasks=[0, 1], n_heads=2, head_totals=[4, 2]) == [[0.25, 0.5]]


def test_combine_micro_stats_is_the_weighted_sum_in_order():
    from video_analytics_amd import vgg
    st = [torch.tensor([2.0, 1.0]), torch.tensor([4.0, 2.0]), torch.tensor([1.0, 0.0])]
    sc = [[3 / 7], [3 / 7], [1 / 7]]
    out = vgg.combine_micro_stats(st, sc)
    want = np.float32(0.0)
    for s, t in zip(sc, st):
        want = np.float32(want + np.float32(np.float32(s[0]) * np.float32(t[0])))
    assert out.dtype == torch.float32 and float(out[0]) == float(want) and float(out[1]) == 3.0
    # heads: stats [2 + 2H] = loss, hits, loss per head, hits per head
    st = [torch.tensor([3.0, 2.0, 1.0, 2.0, 1.0, 1.0]), torch.tensor([4.0, 1.0, 0.0, 4.0, 0.0, 1.0])]
    out = vgg.combine_micro_stats(st, [[1.0, 0.5], [0.0, 0.5]], n_heads=2)
    assert out.tolist() == [4.0, 3.0, 1.0, 3.0, 1.0, 2.0]


def test_check_scales_and_clip_norm():
    from video_analytics_amd import vgg
    assert vgg.check_scales(None, 2, "t") == [1.0, 1.0] and vgg.check_scales(0.5, 2, "t") == [0.5, 0.5]
    assert vgg.check_scales([0.25, 1], 2, "t") == [0.25, 1.0]
    for bad in ([1.0], [1.0, float("nan")], [1.0, float("inf")], "ab", [None, 1.0], object()):
        with pytest.raises(ValueError):
            vgg.check_scales(bad, 2, "t")
    assert vgg.check_clip_norm(None, "t") == 0.0 and vgg.check_clip_norm(2, "t") == 2.0
    for bad in (0, -1.0, float("nan"), float("inf"), "1", True, [1.0]):
        with pytest.raises(ValueError):
            vgg.check_clip_norm(bad, "t")


# ---- the pipeline's new arguments: before anything reaches the GPU ----

@pytest.fixture
def no_gpu_calls(monkeypatch):
    """Every path to the device raises AssertionError: a ValueError seen with it comes from a host check."""
    from video_analytics_amd import _ffi, augment
    from video_analytics_amd import flow as vflow

    def boom(*a, **k):
        raise AssertionError("reached the GPU")
    for mod, name in ((_ffi, "ctx"), (_ffi, "lib"), (vflow, "tvl1_flow"), (vflow, "tvl1_flow_concurrent"),
                      (vflow, "resize_flow_to_stack"), (augment, "resize_images"), (augment, "crops_to_device")):
        monkeypatch.setattr(mod, name, boom)


def _bare_pipeline(heads=None):
    from video_analytics_amd import pipeline
    pipe = pipeline.TwoStreamPipeline.__new__(pipeline.TwoStreamPipeline)
    pipe.L, pipe.D, pipe.motion, pipe.mean_flow, pipe.camera, pipe._n = 10, 5, "stack", False, "none", 0
    pipe.device = torch.device("cpu")
    pipe.heads = heads
    pipe.diff = None
    pipe.spatial = pipe.temporal = types.SimpleNamespace(dtype="f32", n_classes=101 if heads is None else sum(heads))
    return pipe


def test_train_videos_refuses_bad_accumulate_arguments_on_the_host(no_gpu_calls):
    pipe = _bare_pipeline()
    vids = [(torch.zeros(25, 3, 240, 320, dtype=torch.uint8), torch.zeros(25, 240, 320, dtype=torch.uint8))] * 3
    labels = [1, 2, 3]
    for kw, match in ((dict(micro_videos=0), "micro_videos"), (dict(micro_videos=-2), "micro_videos"), (dict(micro_videos=2.0), "micro_videos"),
                      (dict(micro_videos=True), "micro_videos"), (dict(micro_videos="2"), "micro_videos"),
                      (dict(micro_videos=33, k=2), "micro_videos\\*k"), (dict(micro_videos=22), "micro_videos\\*k"),
                      (dict(clip_norm=0.0), "clip_norm"), (dict(clip_norm=-1.0), "clip_norm"), (dict(clip_norm=float("nan")), "clip_norm"),
                      (dict(clip_norm=float("inf"), micro_videos=1), "clip_norm"), (dict(clip_norm="1"), "clip_norm"),
                      (dict(data_parallel=True), "process group"), (dict(data_parallel=1), "data_parallel"),
                      (dict(data_parallel=True, micro_videos=1, clip_norm=1.0), "process group")):
        with pytest.raises(ValueError, match=match):
            pipe.train_videos(vids, labels, **kw)
    # clip_norm alone does not lift the limit on n*k; micro_videos does (the next check then refuses the CPU tensors)
    with pytest.raises(ValueError, match="micro_videos= takes larger batches"):
        pipe.train_videos(vids * 11, labels * 11, k=2, clip_norm=1.0)
    with pytest.raises(ValueError, match="n\\*k in 1..64"):
        pipe.train_videos(vids * 11, labels * 11, k=2)
    with pytest.raises(ValueError, match="must be on"):
        pipe.train_videos(vids * 11, labels * 11, k=2, micro_videos=8)
    with pytest.raises(ValueError, match="no videos"):
        pipe.train_videos([], [], micro_videos=2)
    # the heads' checks still come first for their arguments
    with pytest.raises(ValueError, match="tasks="):
        _bare_pipeline((51, 101)).train_videos(vids, labels, micro_videos=2)


def test_stream_refuses_bad_accumulate_arguments_on_the_host(no_gpu_calls):
    from video_analytics_amd import vgg
    m = vgg.Vgg16Stream.__new__(vgg.Vgg16Stream)
    m.c_in, m.n_classes, m.desc_dim, m.device, m._h = 3, 8, 256, torch.device("cpu"), None
    x = torch.zeros(2, 3, 224, 224)
    for kw in (dict(tasks=[0, 1]), dict(heads=(3, 5)), dict(k=-1), dict(tasks=[0, 1], heads=(3, 5), k=0), dict(tasks=[0, 1], heads=(3, 4), k=1),
               dict(scales=[1.0, 1.0]), dict(scales=float("nan")), dict(tasks=[0, 1], heads=(3, 5), k=1, scales=[1.0])):
        with pytest.raises(ValueError):
            m.train_accumulate(x, torch.tensor([0, 1]), first=True, dropout_seed=0, **kw)
    with pytest.raises(ValueError, match="CUDA"):
        m.train_accumulate(x, torch.tensor([0, 1]), first=True, dropout_seed=0)
    with pytest.raises(TypeError):
        m.train_accumulate(x, torch.tensor([0, 1]), dropout_seed=0)  # first= has no default: STORE or ADD is the caller's decision
    for clip in (0, -1.0, float("nan"), "x"):
        with pytest.raises(ValueError, match="clip_norm"):
            m.train_apply(1e-3, 0.9, clip)
    with pytest.raises(ValueError, match="nothing was accumulated"):
        m.train_apply(1e-3, 0.9)
    with pytest.raises(ValueError, match="nothing was accumulated"):
        m.export_grad()


# ---- dist.all_reduce_gradients at gloo world 2 ----

_WORKER = r"""
import sys, torch
sys.path.insert(0, %r)
from video_analytics_amd import dist as vdist
rank, _, world = vdist.init("gloo")
assert world == 2 and vdist.rank_world() == (rank, 2)
g = torch.arange(1000, dtype=torch.float32) * (rank + 1) + 0.25 * rank
g[-7:] = 0.0  # an alignment gap: zeros on every rank stay zeros
out = vdist.all_reduce_gradients(g)
want = torch.arange(1000, dtype=torch.float32) * 3 + 0.25
want[-7:] = 0.0
assert out is g and torch.equal(g, want), (rank, g[:4])
c = vdist.all_reduce_sum(torch.tensor([rank + 1, 10 * rank], dtype=torch.int64))
assert c.tolist() == [3, 10]
for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(2, 2), torch.zeros(8)[::2], [1.0]):
    try:
        vdist.all_reduce_gradients(bad)
    except ValueError:
        continue
    raise SystemExit("a bad gradient tensor was accepted")
vdist.barrier()
"""


def test_all_reduce_gradients_at_gloo_world_two(tmp_path):
    from video_analytics_amd import dist as vdist, launch
    g = torch.arange(8, dtype=torch.float32)
    assert vdist.all_reduce_gradients(g) is g and vdist.rank_world() == (0, 1)  # without a group: the identity
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % ROOT)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["VA_DIST_BACKEND"] = "gloo"
    assert launch.spawn_ranks([sys.executable, str(script)], 2, env=env, timeout=120) == 0
