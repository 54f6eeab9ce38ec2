"""Multi-task training on the device: k_ce_multitask_fwd_bwd against the float64 witness of
tests/test_multitask_host.py and, bit for bit, against the existing loss kernels on every head's rows and columns; bad rows
and bad arguments; the one-head step against the consensus step (bit for bit); the two-head step against torch-CPU autograd
+ torch.optim.SGD, with an absent head coasting on its momentum; TwoStreamPipeline.train_videos(tasks=) and
run_video(task=) against the same pieces called one by one."""
import ctypes
import random

import numpy as np
import pytest
import torch

from test_multitask_host import CASES, case_id, check_against_witness, make_case, mt_rows, offsets, witness
from test_train_gpu import TOL_UPDATE, _relerr, _rmserr
from test_train_kernels_gpu import TOL_DLOGITS, _Box, _Inputs, _bits_equal, _ulp32
from test_tsn_gpu import _state, _videos
from test_video_gpu import SCHEDULE, _synthetic_video

pytestmark = pytest.mark.gpu

HEADS2 = (51, 101)
_runs = {}  # case id -> what the kernel gave for it: computed once, shared by the tests of the loss kernel, never changed


def _run_mt(z, labels, tasks, heads, K, what):
    """va_train_loss_multitask twice on NaN-prefilled outputs between canaries -> (dz [n,k,C], out [2+2H]), both runs'
    bits identical."""
    from video_analytics_amd import vgg
    n, kk, C = z.shape
    In = _Inputs(z=z.reshape(n, C) if K == 0 else z, labels=labels, tasks=tasks)
    outs = []
    for _ in range(2):
        dz, out = _Box(In.z.shape), _Box((2 + 2 * len(heads),))
        vgg.train_loss_multitask(In.z, In.labels, In.tasks, heads, dz.t, out.t, k=K)
        torch.cuda.synchronize()
        In.check(what)
        dz.check(what + ("dlogits",), finite=False)
        out.check(what + ("out",), finite=False)
        outs.append((dz.t.clone().reshape(n, kk, C), out.t.clone()))
    assert _bits_equal(outs[0][0], outs[1][0]) and _bits_equal(outs[0][1], outs[1][1]), (what, "not deterministic")
    return outs[0]


def _case_run(case):
    cid = case_id(case)
    if cid not in _runs:
        z, labels, tasks = make_case(*case)
        dz, out = _run_mt(z, labels, tasks, case[0], case[2], ("multitask", cid))
        _runs[cid] = (z, labels, tasks, dz, out)
    return _runs[cid]


# ---- 1: the loss kernel against the witness ----

@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_loss_kernel_against_float64(case):
    """The batches of tests/test_multitask_host.py (its header: rows whose label is the arg-max keep a miss of 1/32, which the
    bound needs of a block that is one such row).  The worst figure per case is printed before the assertions."""
    heads = case[0]
    z, labels, tasks, dz, out = _case_run(case)
    assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(out).all()), (case_id(case), "an output was not written")
    # the figure first, then the assertions
    _, _, _, dz_r = witness(z, labels, tasks, heads)
    off = offsets(heads)
    worst = 0.0
    for t in range(len(heads)):
        rows = [v for v in range(z.shape[0]) if int(tasks[v]) == t]
        if rows:
            ref = dz_r[rows][:, :, off[t]:off[t] + heads[t]]
            err = float((dz.cpu()[rows][:, :, off[t]:off[t] + heads[t]].double() - ref).abs().max())
            scale = float(ref.abs().max())
            worst = max(worst, err / scale if scale > 0 else err)
    print("%s: worst gradient error / largest reference entry of the block %.3e (bound %.0e)" % (case_id(case), worst, TOL_DLOGITS))
    check_against_witness(case_id(case), out.cpu(), dz.cpu(), z, labels, tasks, heads)


# ---- 2: against the existing kernels, bit for bit ----

@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_every_head_is_the_existing_loss_on_its_rows_and_columns(case):
    from video_analytics_amd import vgg
    heads, n, K, _ = case
    z, labels, tasks, dz, out = _case_run(case)
    H, off, kk = len(heads), offsets(heads), max(K, 1)
    for t in range(H):
        rows = [v for v in range(n) if int(tasks[v]) == t]
        if not rows:
            continue
        zs = z[rows][:, :, off[t]:off[t] + heads[t]].contiguous().cuda()   # [n_t][k][C_t]
        if K == 0:
            zs = zs.reshape(len(rows), heads[t])
        d1 = torch.full_like(zs, float("nan"))
        o1 = torch.full((2,), float("nan"), device="cuda")
        vgg.train_loss(zs, labels[rows].cuda(), d1, o1, k=K)
        torch.cuda.synchronize()
        blk = dz[rows][:, :, off[t]:off[t] + heads[t]]
        assert _bits_equal(d1.reshape(len(rows), kk, heads[t]), blk), (case_id(case), t, "gradient block")
        assert _bits_equal(o1[0:1], out[2 + t:3 + t]) and _bits_equal(o1[1:2], out[2 + H + t:3 + H + t]), (case_id(case), t, o1, out)
    if H == 1:  # the whole output is va_train_loss's, at k = 0 and k >= 1 alike
        zz = (z.reshape(n, heads[0]) if K == 0 else z).cuda()
        d1 = torch.full_like(zz, float("nan"))
        o1 = torch.full((2,), float("nan"), device="cuda")
        vgg.train_loss(zz, labels.cuda(), d1, o1, k=K)
        torch.cuda.synchronize()
        assert _bits_equal(d1.reshape(n, kk, heads[0]), dz) and _bits_equal(o1, out[:2]) and _bits_equal(o1, out[2:4]), case_id(case)


# ---- 3: bad rows, bad arguments ----

@pytest.mark.parametrize("K", [0, 3])
@pytest.mark.parametrize("bad", [("task", -1), ("task", 2), ("label", 101), ("label", -1)], ids=lambda b: "%s_%d" % b)
def test_a_bad_row_is_nan_for_that_video_only(K, bad):
    """Video 1 of 3 is the only video of head 1: with a bad task head 1 is absent and head 0 keeps its two videos."""
    g = torch.Generator().manual_seed(9)
    tasks = torch.tensor([0, 1, 0], dtype=torch.int32)
    z, labels = mt_rows(3, K, HEADS2, tasks, g)
    dz0, out0 = _run_mt(z, labels, tasks, HEADS2, K, ("good", K))
    assert bool(torch.isfinite(dz0).all()) and bool(torch.isfinite(out0).all())
    what, value = bad
    if what == "task":
        tasks = tasks.clone()
        tasks[1] = value
    else:
        labels = labels.clone()
        labels[1] = value
    dz, out = _run_mt(z, labels, tasks, HEADS2, K, ("bad", what, value, K))
    assert bool(torch.isnan(out[0])) and bool(torch.isfinite(out[1]))
    assert bool(torch.isnan(dz[1]).all()), "every entry of the video's K x C gradient rows is NaN"
    for v in (0, 2):
        assert bool(torch.isfinite(dz[v]).all()) and _bits_equal(dz[v], dz0[v]), v
    assert _bits_equal(out[2:3], out0[2:3]) and _bits_equal(out[4:5], out0[4:5])  # head 0 is untouched
    if what == "task":
        assert float(out[3]) == 0.0 and float(out[5]) == 0.0   # head 1 has no video
    else:
        assert bool(torch.isnan(out[3])) and float(out[5]) == 0.0


def test_argument_errors_launch_nothing():
    from video_analytics_amd import _ffi, synth, vgg
    L, c = _ffi.lib(), _ffi.ctx(0)
    st = _ffi.stream_ptr(torch.device("cuda", 0))
    z = torch.zeros(3, 2, 152, device="cuda")
    y = torch.zeros(3, dtype=torch.int64, device="cuda")
    t = torch.zeros(3, dtype=torch.int32, device="cuda")
    dz = torch.full_like(z, float("nan"))
    out = torch.full((6,), float("nan"), device="cuda")
    hs = lambda *v: (ctypes.c_int * max(1, len(v)))(*v)

    def call(logits=z, labels=y, tasks=t, n=3, k=2, nh=2, heads=hs(51, 101), dl=dz, o=out):
        return L.va_train_loss_multitask(c, _ffi.ptr(logits), _ffi.ptr(labels), _ffi.ptr(tasks), n, k, nh, heads, _ffi.ptr(dl), _ffi.ptr(o), st)
    for kw in (dict(n=0), dict(n=-1), dict(k=-1), dict(n=33, k=2), dict(n=65, k=0), dict(nh=0), dict(nh=9, heads=hs(*([1] * 9))),
               dict(heads=hs(51, 0)), dict(heads=hs(-5, 101)), dict(heads=None), dict(heads=hs(1 << 20, 1)), dict(heads=hs(1 << 21, 1)),
               dict(logits=None), dict(labels=None), dict(tasks=None), dict(dl=None), dict(o=None)):
        assert call(**kw) == _ffi.VA_ERR_INVALID, kw
        assert _ffi.lib().va_last_error()
    assert L.va_train_loss_multitask(None, _ffi.ptr(z), _ffi.ptr(y), _ffi.ptr(t), 3, 2, 2, hs(51, 101), _ffi.ptr(dz), _ffi.ptr(out), st) \
        == _ffi.VA_ERR_INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(dz).all()) and bool(torch.isnan(out).all())
    assert call() == _ffi.VA_OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(out).all())
    # the step's entry point
    w = synth.synth_vgg16_weights(c_in=3, n_classes=152, seed=4)
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 152, 256)
    m.train_init()
    before = _state(m)
    x = torch.zeros(4, 3, 224, 224, device="cuda")
    y4 = torch.zeros(2, dtype=torch.int64, device="cuda")
    t4 = torch.zeros(2, dtype=torch.int32, device="cuda")
    stats = torch.full((6,), float("nan"), device="cuda")
    desc = torch.full((4, 256), float("nan"), device="cuda")
    nbytes = L.va_vgg16_train_workspace_bytes(m._h, 4)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def step(model=m._h, xx=x, labels=y4, tasks=t4, n=2, k=2, nh=2, heads=hs(51, 101), o=stats):
        return L.va_vgg16_train_step_multitask(model, _ffi.ptr(xx), 0, _ffi.ptr(labels), _ffi.ptr(tasks), n, k, nh, heads, 1e-4, 0.9, 0,
                                               _ffi.ptr(desc), _ffi.ptr(o), _ffi.ptr(ws), ws.numel(), st)
    for kw in (dict(model=None), dict(xx=None), dict(labels=None), dict(tasks=None), dict(o=None), dict(n=0), dict(k=0), dict(n=13, k=5),
               dict(nh=0), dict(nh=9, heads=hs(*([1] * 9))), dict(heads=None), dict(heads=hs(51, 100)), dict(heads=hs(152, 0)),
               dict(nh=1, heads=hs(101))):
        assert step(**kw) == _ffi.VA_ERR_INVALID, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(stats).all()) and bool(torch.isnan(desc).all())
    assert all(torch.equal(a, b) for a, b in zip(before, _state(m)))
    # the wrapper's own checks
    xs = torch.zeros(6, 3, 224, 224, device="cuda")
    for labels, tasks, heads, k in (([1, 101], [0, 1], HEADS2, 3), ([51, 1], [0, 1], HEADS2, 3), ([1, 1], [0, 2], HEADS2, 3),
                                    ([1, 1], [0], HEADS2, 3), ([1], [0, 1], HEADS2, 3), ([1, 1], [0, 1], (51, 100), 3),
                                    ([1, 1], [0, 1], HEADS2, 4), ([1, 1], [0, 1], HEADS2, 0), ([1, 1], [0, 1], (), 3)):
        with pytest.raises(ValueError):
            m.train_step_multitask(xs, labels, tasks, heads, k, 1e-4, 0.9, 0)
    assert all(torch.equal(a, b) for a, b in zip(before, _state(m)))
    # on the device nothing is copied back: a bad row gives a NaN loss, as the consensus step does
    s, _ = m.train_step_multitask(xs, torch.tensor([1, 101]).cuda(), torch.tensor([0, 1], dtype=torch.int32).cuda(), HEADS2, 3, 1e-4, 0.9, 0)
    assert bool(torch.isnan(s.cpu()[0]))
    m.close()


# ---- 4: one head is the plain consensus step ----

@pytest.mark.parametrize("c_in,B,k", [(3, 4, 1), (20, 4, 2)])
def test_one_head_is_the_consensus_step(c_in, B, k):
    from video_analytics_amd import synth, vgg
    w = synth.synth_vgg16_weights(c_in=3, seed=4)
    if c_in != 3:
        w["conv_w"][0] = vgg.copy_first_layer(w["conv_w"][0].cuda(), c_in).cpu()
    x = torch.from_numpy(synth.hash_uniform(71, c_in, B * c_in * 224 * 224).reshape(B, c_in, 224, 224) * 4.0 - 2.0).cuda()
    n = B // k
    labels = torch.tensor([(7 * i + 1) % 101 for i in range(n)], dtype=torch.int64).cuda()
    tasks = torch.zeros(n, dtype=torch.int32).cuda()
    res = []
    for multi in (False, True):
        m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256)
        for step in range(2):  # the second step exercises the momentum buffers
            if multi:
                stats, desc = m.train_step_multitask(x, labels, tasks, (101,), k, 1e-4, 0.9, 1000 + step)
            else:
                stats, desc = m.train_step_consensus(x, labels, k, 1e-4, 0.9, 1000 + step)
        res.append((stats.cpu(), desc.cpu(), _state(m)))
        m.close()
    assert torch.isfinite(res[0][0]).all() and float(res[0][0][0]) > 0 and tuple(res[1][0].shape) == (4,)
    assert _bits_equal(res[0][0], res[1][0][:2]) and _bits_equal(res[0][0], res[1][0][2:]) and _bits_equal(res[0][1], res[1][1])
    assert len(res[0][2]) == 68 and all(_bits_equal(a, b) for a, b in zip(res[0][2], res[1][2]))


# ---- 5: two heads against autograd; an absent head coasts on its momentum ----

def test_two_heads_match_autograd_and_an_absent_head_coasts():
    """n = 6 videos of k = 2 snippets, heads (51, 101), tasks [0,1,1,0,1,1], against torch-CPU autograd of the sum of the two
    heads' cross-entropies on the snippet means + torch.optim.SGD with the same dropout masks, at the tolerances of
    tests/test_tsn_gpu.py's consensus step.  Then a step with every video in head 1: head 0's rows of the last layer get an
    exactly zero gradient, V' = mu V and W' = W - lr V'."""
    import torch.nn.functional as F
    from oracle import train_oracle, vgg_oracle
    from video_analytics_amd import synth, vgg
    torch.set_num_threads(8)
    n, k = 6, 2
    B = n * k
    w = synth.synth_vgg16_weights(c_in=3, n_classes=152, seed=4)
    lr, mu, seed = 1e-4, 0.9, 1003
    x = torch.from_numpy(synth.hash_uniform(72, 3, B * 3 * 224 * 224).reshape(B, 3, 224, 224) * 4.0 - 2.0)
    tasks = torch.tensor([0, 1, 1, 0, 1, 1], dtype=torch.int32)
    labels = torch.tensor([(7 * i + 1) % HEADS2[int(tasks[i])] for i in range(n)], dtype=torch.int64)
    ora = train_oracle.TrainOracle(w, lr, mu)
    p = ora.params
    op = vgg_oracle.features(x, p["conv_w"], p["conv_b"]).reshape(B, -1)
    for l in range(3):
        op = F.relu(F.linear(op, p["fc_w"][l], p["fc_b"][l]))
        op = op * train_oracle.dropout_mask(seed, l, tuple(op.shape))
    desc_r = op.detach()
    cons = F.linear(op, p["fc_w"][3], p["fc_b"][3]).view(n, k, -1).mean(1)
    loss, loss_t, hits_t = None, [], []
    for t, (o, c) in enumerate(zip(offsets(HEADS2), HEADS2)):
        idx = torch.nonzero(tasks.long() == t).flatten()
        sl = cons[idx][:, o:o + c]
        lt = F.cross_entropy(sl, labels[idx])
        loss = lt if loss is None else loss + lt
        loss_t.append(float(lt.detach()))
        hits_t.append(int((sl.argmax(1) == labels[idx]).sum()))
    ora.opt.zero_grad()
    loss.backward()
    ora.opt.step()
    loss_r = float(loss.detach())

    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 152, 256)
    stats, desc = m.train_step_multitask(x.cuda(), labels, tasks, HEADS2, k, lr, mu, seed)
    stats = stats.cpu()
    print("multi-task loss %.6f (autograd %.6f), per head %s (%s), hits %s (%s)"
          % (float(stats[0]), loss_r, stats[2:4].tolist(), loss_t, stats[4:6].tolist(), hits_t))
    assert tuple(stats.shape) == (6,)
    assert abs(float(stats[0]) - loss_r) < 2e-4 * max(1.0, abs(loss_r)), (float(stats[0]), loss_r)
    assert int(stats[1]) == sum(hits_t)
    for t in range(2):
        assert abs(float(stats[2 + t]) - loss_t[t]) < 2e-4 * max(1.0, abs(loss_t[t])), (t, float(stats[2 + t]), loss_t[t])
        assert int(stats[4 + t]) == hits_t[t], t
    assert tuple(desc.shape) == (B, 256) and _relerr(desc.cpu(), desc_r) < 1e-3
    got, ref = m.export_state(), ora.weights()
    gotm, refm = m.export_state(momentum=True), ora.momentum()
    worst, rms = [], []
    for key in ("conv_w", "conv_b", "fc_w", "fc_b"):
        for i, (g, r, o, gm, rm) in enumerate(zip(got[key], ref[key], w[key], gotm[key], refm[key])):
            e_upd, e_mom, e_rms = _relerr(g.cpu() - o, r - o), _relerr(gm.cpu(), rm), _rmserr(g.cpu() - o, r - o)
            worst.append((max(e_upd, e_mom), key, i))
            rms.append((e_rms, key, i))
            print("%-6s %2d: update err %.2e (rms %.2e)  momentum err %.2e" % (key, i, e_upd, e_rms, e_mom))
    assert max(worst)[0] < TOL_UPDATE, max(worst)
    assert max(rms)[0] < TOL_UPDATE, max(rms)
    tight = [e for e, key, i in worst if key.startswith("fc")]
    assert max(tight) < 5e-4, max(tight)

    # the second step: every video in head 1, head 0 (rows [0, 51) of the last layer) is absent
    W0, b0 = got["fc_w"][3].cpu(), got["fc_b"][3].cpu()
    V0, vb0 = gotm["fc_w"][3].cpu(), gotm["fc_b"][3].cpu()
    assert bool(V0[:51].abs().max() > 0) and bool(vb0[:51].abs().max() > 0)  # the first step did move head 0
    labels1 = torch.tensor([(7 * i + 1) % 101 for i in range(n)], dtype=torch.int64)
    stats1, _ = m.train_step_multitask(x.cuda(), labels1, torch.ones(n, dtype=torch.int32), HEADS2, k, lr, mu, seed + 1)
    stats1 = stats1.cpu()
    assert float(stats1[2]) == 0.0 and float(stats1[4]) == 0.0 and _bits_equal(stats1[0:1], stats1[3:4]) and bool(torch.isfinite(stats1).all())
    W1, b1 = m.export_state()["fc_w"][3].cpu(), m.export_state()["fc_b"][3].cpu()
    V1, vb1 = m.export_state(momentum=True)["fc_w"][3].cpu(), m.export_state(momentum=True)["fc_b"][3].cpu()
    mu32, lr32 = torch.tensor(mu, dtype=torch.float32), torch.tensor(lr, dtype=torch.float32)
    zero = torch.tensor(0.0, dtype=torch.float32)
    for name, Wb, Wa, Vb, Va in (("fc_w[3]", W0, W1, V0, V1), ("fc_b[3]", b0, b1, vb0, vb1)):
        coast = mu32 * Vb[:51] + zero       # V' = mu V + g with g = +0.0 exactly, in float32
        assert _bits_equal(Va[:51], coast), (name, "momentum rows of the absent head")
        tgt = Wb[:51] - lr32 * coast        # float32 on the host
        assert bool(((Wa[:51].double() - tgt.double()).abs() <= _ulp32(tgt.double())).all()), (name, "W' is not W - lr (mu V) within one ulp")
        assert not _bits_equal(Va[51:], mu32 * Vb[51:] + zero), (name, "head 1 did receive a gradient")
    m.close()


# ---- 6: train_videos(tasks=) ----

@pytest.mark.parametrize("rgb_diff", [False, True])
def test_train_videos_with_tasks_is_the_gathers_then_the_multitask_step(rgb_diff):
    from video_analytics_amd import _ffi, augment, pipeline, rgbdiff
    from video_analytics_amd import flow as vflow
    L, k, lr, mu, seed = 10, 3, 1e-4, 0.9, 5
    vids, starts = _videos()  # two 320x240 videos of 25 and 37 frames
    dev = [(r.cuda(), g.cuda()) for r, g in vids]
    crops = augment.draw_scale_jitter_crops(6, 240, 320, random.Random(3))
    labels, tasks = torch.tensor([50, 77]), [0, 1]
    params = _ffi.default_tvl1_params(**SCHEDULE)
    kw = dict(device=0, tvl1_params=params, heads=HEADS2, rgb_diff=rgb_diff)
    pipe, other = pipeline.TwoStreamPipeline(**kw), pipeline.TwoStreamPipeline(**kw)
    assert pipe.spatial.n_classes == pipe.temporal.n_classes == 152 and pipe.heads == HEADS2
    out = pipe.train_videos(dev, labels, k=k, starts=starts, crops=crops, lr=lr, momentum=mu, dropout_seed=seed, tasks=tasks)
    torch.cuda.synchronize()
    assert out["starts"] == starts and torch.equal(out["crops"], crops)
    # the inputs again, from what train_videos returned, through the public gathers
    first, base = [], 0
    for p in out["plans"]:
        first += [base + j for j in p.index]
        base += len(p.pairs)
    rgb_table, flow_table = augment.snippet_tables(crops, list(range(6)), first, L)
    frames = torch.cat([rgb[torch.tensor(st).cuda()] for (rgb, _), st in zip(dev, out["starts"])])
    xs = augment.resize_images(frames, rgb_table)
    xt = vflow.resize_flow_to_stack(out["flow"], flow_table).view(6, 2 * L, 224, 224)
    runs = [("s", other.spatial, pipe.spatial, xs), ("t", other.temporal, pipe.temporal, xt)]
    if rgb_diff:
        D = pipe.D
        win = torch.cat([rgb[torch.tensor([s + f for s in st for f in range(D + 1)]).cuda()] for (rgb, _), st in zip(dev, out["starts"])])
        xd = rgbdiff.rgb_diff_stack(win, rgbdiff.window_table([i * (D + 1) for i in range(6)], crops), D)
        runs.append(("d", other.diff, pipe.diff, xd))
    y, t = labels.cuda(), torch.tensor(tasks, dtype=torch.int32).cuda()
    for name, model, mine, x in runs:
        stats, desc = model.train_step_multitask(x, y, t, HEADS2, k, lr, mu, seed)
        torch.cuda.synchronize()
        assert tuple(stats.shape) == (6,) and bool(torch.isfinite(stats).all()) and float(stats[2]) > 0 and float(stats[3]) > 0
        assert _bits_equal(out["stats_" + name], stats), (name, out["stats_" + name], stats)
        assert _bits_equal(out["desc_" + name], desc), name
        a, b = _state(mine), _state(model)
        assert len(a) == 68 and all(_bits_equal(u, v) for u, v in zip(a, b)), name
    pipe.close()
    other.close()


# ---- 7: run_video(task=) ----

def test_run_video_scores_the_videos_own_head():
    from video_analytics_amd import _ffi, augment, fusion, pipeline, vgg
    from video_analytics_amd.video import evaluateVideos
    rgb, gray = _synthetic_video(20, 240, 320, seed=71)
    rgb, gray = rgb.cuda(), gray.cuda()
    views = augment.ten_crop_views(240, 320)
    vs, vt = views[4:6], views[7:9]
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(**SCHEDULE), heads=HEADS2)
    outs = []
    for task in (0, 1):
        out = pipe.run_video(rgb, gray, n_snippets=3, views=(vs, vt), fusion_weights=(1.0, 1.5), task=task)
        torch.cuda.synchronize()
        assert out["task"] == task
        assert tuple(out["logits_s_items"].shape) == (3, 2, 152) and tuple(out["logits_t_items"].shape) == (3, 2, 152)
        ref = {}
        for s in "st":
            ref[s] = fusion.score_consensus(vgg.head_logits(out["logits_%s_items" % s], HEADS2, task).unsqueeze(0))
            assert ref[s].shape[-1] == HEADS2[task] == out["scores_" + s].shape[-1]
            assert _bits_equal(out["scores_" + s].reshape(-1), ref[s].reshape(-1)), (task, s)
        fused, pred = fusion.fuse_scores(ref["s"], ref["t"], (1.0, 1.5))
        assert _bits_equal(out["scores"].reshape(-1), fused.reshape(-1)) and out["scores"].shape[-1] == HEADS2[task]
        assert int(out["pred"]) == int(pred[0]) == int(fused[0].argmax()) and 0 <= int(out["pred"]) < HEADS2[task]
        outs.append({key: out[key].clone() for key in ("logits_s_items", "logits_t_items", "desc_s", "desc_t")})
    for key in outs[0]:
        assert _bits_equal(outs[0][key], outs[1][key]), key  # the task changes the scores only
    res = evaluateVideos(pipe, [(rgb, gray)], [3], n_snippets=3, views=(vs, vt), task=0)
    assert len(res) == 4 and all(a in (0.0, 1.0) for a in res[:3]) and res[3].shape == (1, 512) and res[3].dtype == np.float32
    pipe.close()
