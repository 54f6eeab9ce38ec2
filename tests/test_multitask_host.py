"""Multi-task training, host side: a float32 numpy restatement of the multi-task consensus loss, in the
order S26 states, held to float64 autograd of the sum of the heads' cross-entropies; ``vgg.check_heads`` /
``vgg.head_logits``; and every ValueError of the new pipeline arguments with all paths to the device blocked.
tests/test_multitask_gpu.py runs the kernel on the cases built here.

Conditioning of the rows (``MIN_MISS``).  Every kernel of the family computes the label's gradient entry as
``fl(softmax) - 1``: the subtraction is exact, so the entry inherits the ABSOLUTE error of a float32 number next to 1, about
2^-24, however small the entry itself is.  The issue's bound is relative to the largest reference entry of a head's block, and
in a row whose label is its arg-max every entry is at most 1 - softmax[label] in magnitude.  A block made of one such row can
therefore meet 1e-5 only when 1 - softmax[label] >= 2^-24 / 1e-5 = 0.006; with the project's fourfold headroom, 0.024.  Rows
of the pattern "label = arg-max" are the only ones that can stand alone in a block with a small miss (n = 1, or one video per
head), so the generator caps their label's softmax at 31/32 (miss 1/32 >= 0.024) by lowering the arg-max logit; the label
stays the arg-max.  In tests/test_train_kernels_gpu.py the same effect hides behind batches whose largest entry is about 1/B.
Without the cap two one-row batches of 134 drew misses of 5.7e-5 and 3.9e-3 and no float32 evaluation of S26's expressions,
k_ce_fwd_bwd's included, can reach the bound on them."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_train_kernels_gpu import TOL_DLOGITS, TOL_LOSS

F32 = np.float32

HEADS = [(101,), (51, 101), (1, 2, 7), (3, 1, 5, 2, 4, 6, 8, 9), (4096, 1)]
SHAPES = [(n, k) for n in (1, 3, 64) for k in (0, 1, 3, 8) if n * max(k, 1) <= 64]
PATTERNS = ("round_robin", "one_head", "single_video", "last_absent")
MIN_MISS = 1.0 / 32.0  # least 1 - softmax[label] of a row whose label is its arg-max (the header: >= 4 * 2^-24 / 1e-5)


def offsets(heads):
    return [int(sum(heads[:t])) for t in range(len(heads))]


def task_pattern(name, n, H):
    """tasks [n] of one pattern: round-robin over the heads; every video in one head (all others absent); head 0 with a
    single video (the last one) and the rest round-robin over the other heads; round-robin without the last head."""
    if name == "round_robin":
        t = [v % H for v in range(n)]
    elif name == "one_head":
        t = [min(1, H - 1)] * n
    elif name == "single_video":
        t = [(1 + v % (H - 1)) if H > 1 else 0 for v in range(n)]
        t[-1] = 0
    else:
        t = [v % max(1, H - 1) for v in range(n)]
    return np.array(t, dtype=np.int32)


def cases():
    """(heads, n, k, pattern) without the patterns that coincide for that n and H."""
    out = []
    for heads in HEADS:
        for n, k in SHAPES:
            seen = set()
            for p in PATTERNS:
                key = tuple(task_pattern(p, n, len(heads)).tolist())
                if key not in seen:
                    seen.add(key)
                    out.append((heads, n, k, p))
    return out


CASES = cases()


def case_id(c):
    return "h%s_n%d_k%d_%s" % ("x".join(str(h) for h in c[0]), c[1], c[2], c[3])


def case_seed(heads, n, k, pattern):
    return 1000 * sum((i + 1) * h for i, h in enumerate(heads)) % 9973 + 100 * n + 10 * k + PATTERNS.index(pattern)


def mt_rows(n, k, heads, tasks, g):
    """Logits [n][max(k, 1)][C] and LOCAL labels [n].  The row patterns of tests/test_train_kernels_gpu.py's ``_loss_rows``
    on the video's own head, by v % 5: 0 = random, label = the head's arg-max; 1 = random, label != arg-max; 2 = all of the
    head's logits equal (the first index is the arg-max; label 0 for v % 10 == 2, else C_t - 1); 3 = +80 and -80 among random
    logits; 4 = random, random label.  The columns of the other heads are random (they must not matter).  Pattern 0 keeps
    1 - softmax[label] >= MIN_MISS (the module's header): the arg-max logit of every snippet is lowered where it is not."""
    kk, C, off = max(k, 1), int(sum(heads)), offsets(heads)
    z = torch.randn(n, kk, C, generator=g) * 3.0
    labels = torch.zeros(n, dtype=torch.int64)
    for v in range(n):
        t = int(tasks[v])
        o, c = off[t], int(heads[t])
        labels[v] = int(torch.randint(0, c, (1,), generator=g))
        am = int(z[v, :, o:o + c].double().mean(0).argmax())
        if v % 5 == 0:
            labels[v] = am
            if c > 1:
                m = z[v, :, o:o + c].double().mean(0)
                cap = float(torch.logsumexp(torch.cat([m[:am], m[am + 1:]]), 0)) + math.log(1.0 / MIN_MISS - 1.0)
                if float(m[am]) > cap:  # softmax[label] = 1 - MIN_MISS at the cap, which lies above every other logit
                    z[v, :, o + am] -= float(m[am]) - cap
        elif v % 5 == 1:
            labels[v] = (am + 1) % c
        elif v % 5 == 2:
            z[v, :, o:o + c] = torch.randn(kk, 1, generator=g).expand(kk, c)
            labels[v] = 0 if v % 10 == 2 else c - 1
        elif v % 5 == 3:
            z[v, :, o + int(labels[v])] = 80.0 if v % 2 else -80.0
            z[v, :, o + (int(labels[v]) + 1) % c] = -80.0 if v % 2 else 80.0
    return z, labels


def make_case(heads, n, k, pattern):
    tasks = task_pattern(pattern, n, len(heads))
    g = torch.Generator().manual_seed(case_seed(heads, n, k, pattern))
    z, labels = mt_rows(n, k, heads, tasks, g)
    return z, labels, torch.from_numpy(tasks)


# ---- S26: the restatement ----

def s26_multitask_loss(z, y, tasks, heads):
    """S26 in float32, in its stated order: z [n,k,C], local labels [n], tasks [n], heads (C_0 .. C_{H-1}) ->
    (out f32 [2+2H] = loss, hits, loss_t, hits_t; dz f32 [n,k,C])."""
    z = np.asarray(z, dtype=F32)
    n, k, C = z.shape
    H, off = len(heads), offsets(heads)
    assert C == sum(heads)
    counts = [int(sum(1 for v in range(n) if int(tasks[v]) == t)) for t in range(H)]
    m = z[:, 0].copy()
    for j in range(1, k):
        m = m + z[:, j]
    m = m / F32(k)
    dz = np.zeros_like(z)
    ell, hit = np.zeros(n, dtype=F32), np.zeros(n, dtype=np.int64)
    for v in range(n):
        t, yv = int(tasks[v]), int(y[v])
        o, c = off[t], int(heads[t])
        inv_t = F32(1.0) / F32(counts[t])
        l = m[v, o:o + c]
        am = int(np.argmax(l))  # the first maximum
        mx = l[am]
        e = np.exp(l - mx)
        assert e.dtype == F32
        se = np.add.accumulate(np.concatenate([np.zeros(1, dtype=F32), e]), dtype=F32)[-1]  # 0 + e_0 + e_1 + ... in class order
        ell[v] = (np.log(se) + mx) - l[yv]
        hit[v] = int(am == yv)
        onehot = np.zeros(c, dtype=F32)
        onehot[yv] = 1.0
        g = (e * (F32(1.0) / se) - onehot) * inv_t
        dz[v, :, o:o + c] = (g / F32(k))[None, :]
    out = np.zeros(2 + 2 * H, dtype=F32)
    total, first = F32(0.0), True
    for t in range(H):
        L, hc = F32(0.0), 0
        for v in range(n):
            if int(tasks[v]) == t:
                L = F32(L + ell[v])
                hc += int(hit[v])
        if counts[t]:
            lt = F32(L * (F32(1.0) / F32(counts[t])))
            total = lt if first else F32(total + lt)
            first = False
            out[2 + t] = lt
        out[2 + H + t] = hc
    out[0], out[1] = total, hit.sum()
    return out, dz


def witness(z, y, tasks, heads):
    """float64 autograd of sum over the present heads of cross_entropy(z.mean(1)[idx_t][:, o_t:o_t+C_t], y[idx_t]) ->
    (loss, loss_t [H], hits_t [H], dz [n,k,C]), everything float64 / int."""
    zt = z.double().clone().requires_grad_(True)
    m = zt.mean(1)
    off, H = offsets(heads), len(heads)
    loss_t, hits_t, total = [0.0] * H, [0] * H, None
    for t in range(H):
        idx = torch.nonzero(torch.as_tensor(tasks).long() == t).flatten()
        if idx.numel() == 0:
            continue
        sl = m[idx][:, off[t]:off[t] + heads[t]]
        lt = F.cross_entropy(sl, y[idx])
        loss_t[t] = float(lt.detach())
        hits_t[t] = int((sl.argmax(1) == y[idx]).sum())
        total = lt if total is None else total + lt
    total.backward()
    return float(total.detach()), loss_t, hits_t, zt.grad


def check_against_witness(what, out, dz, z, labels, tasks, heads):
    """The assertions both the restatement (here) and the kernel (tests/test_multitask_gpu.py) are held to.  out f32 [2+2H],
    dz [n,k,C] as CPU tensors.  Returns the worst gradient error relative to its block's largest reference entry."""
    H, off, n = len(heads), offsets(heads), z.shape[0]
    loss_r, loss_t, hits_t, dz_r = witness(z, labels, tasks, heads)
    assert abs(float(out[0]) - loss_r) < TOL_LOSS * max(1.0, abs(loss_r)), (what, float(out[0]), loss_r)
    assert int(out[1]) == sum(hits_t), (what, int(out[1]), hits_t)
    worst = 0.0
    for t in range(H):
        assert abs(float(out[2 + t]) - loss_t[t]) < TOL_LOSS * max(1.0, abs(loss_t[t])), (what, t, float(out[2 + t]), loss_t[t])
        assert int(out[2 + H + t]) == hits_t[t], (what, t)
        rows = [v for v in range(n) if int(tasks[v]) == t]
        if not rows:
            assert float(out[2 + t]) == 0.0 and float(out[2 + H + t]) == 0.0, (what, t, "an absent head reports 0")
            continue
        blk = dz[rows][:, :, off[t]:off[t] + heads[t]].double()
        ref = dz_r[rows][:, :, off[t]:off[t] + heads[t]]
        scale = float(ref.abs().max())
        e = float((blk - ref).abs().max()) / scale if scale > 0 else float(blk.abs().max())
        worst = max(worst, e)
        assert e < TOL_DLOGITS, (what, "head %d gradient block" % t, e)
        bits = dz[rows].contiguous().view(torch.int32)
        assert bool((bits[:, :, :off[t]] == 0).all()) and bool((bits[:, :, off[t] + heads[t]:] == 0).all()), \
            (what, t, "not exactly 0.0 outside the head")
    return worst


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_restatement_against_float64_autograd(case):
    heads, n, k, pattern = case
    z, labels, tasks = make_case(*case)
    out, dz = s26_multitask_loss(z.numpy(), labels.numpy(), tasks.numpy(), heads)
    assert out.dtype == F32 and dz.dtype == F32 and np.isfinite(out).all() and np.isfinite(dz).all()
    worst = check_against_witness(case_id(case), torch.from_numpy(out), torch.from_numpy(dz), z, labels, tasks, heads)
    print("%s: worst gradient error / largest reference entry of the block %.3e" % (case_id(case), worst))
    assert all(np.array_equal(dz[:, 0], dz[:, j]) for j in range(dz.shape[1]))


def test_the_cases_cover_what_they_claim():
    # one head: every pattern is the same batch; one video: two distinct batches (head 0 or head 1); else three or four
    assert {c[0] for c in CASES} == set(HEADS) and {(c[1], c[2]) for c in CASES} == set(SHAPES)
    assert {c[3] for c in CASES if c[1] >= 3 and len(c[0]) >= 3} == set(PATTERNS)
    absent = single = ties = big = capped = 0
    for case in CASES:
        heads, n, k, pattern = case
        z, labels, tasks = make_case(*case)
        counts = np.bincount(tasks.numpy(), minlength=len(heads))
        absent += int((counts == 0).any())
        single += int((counts == 1).any() and n > 1)
        off = offsets(heads)
        for v in range(n):
            t = int(tasks[v])
            sl = z[v, :, off[t]:off[t] + heads[t]]
            ties += int(heads[t] > 1 and bool((sl == sl[:, :1]).all()))
            big += int(float(sl.abs().max()) == 80.0)
            if v % 5 == 0 and heads[t] > 1:  # label = arg-max, and not too confidently
                p = torch.softmax(sl.double().mean(0), 0)
                assert int(p.argmax()) == int(labels[v]) and 1.0 - float(p[int(labels[v])]) >= MIN_MISS * (1.0 - 1e-5), (case_id(case), v)
                capped += int(1.0 - float(p[int(labels[v])]) <= MIN_MISS * (1.0 + 1e-5))
        assert int(labels.min()) >= 0 and all(int(labels[v]) < heads[int(tasks[v])] for v in range(n))
    print("cases %d: %d with an absent head, %d with a head of one video, %d tie rows, %d rows with +-80" % (len(CASES), absent, single, ties, big))
    assert absent > 0 and single > 0 and ties > 0 and big > 0 and capped > 0, (absent, single, ties, big, capped)
    # with one head every pattern is the same batch: one case per shape
    assert sum(1 for c in CASES if c[0] == (101,)) == len(SHAPES)


def test_one_head_restates_the_consensus_loss():
    """H = 1: S26 is S20 (tests/test_tsn_host.py's restatement) value for value."""
    from test_tsn_host import s20_consensus_loss
    g = torch.Generator().manual_seed(5)
    for n, k, c in ((8, 3, 101), (2, 1, 7), (5, 7, 33)):
        z = (torch.randn(n, k, c, generator=g) * 3.0).numpy()
        y = torch.randint(0, c, (n,), generator=g).numpy()
        out, dz = s26_multitask_loss(z, y, np.zeros(n, dtype=np.int32), (c,))
        loss, hits, dz20, _ = s20_consensus_loss(z, y)
        assert out[0] == loss == out[2] and int(out[1]) == hits == int(out[3])
        assert np.array_equal(dz, dz20)


# ---- coverage ----

# kernel of csrc/multitask.hip -> the tests of tests/test_multitask_gpu.py that hold it
COVERAGE = {"k_ce_multitask_fwd_bwd": ("test_loss_kernel_against_float64", "test_every_head_is_the_existing_loss_on_its_rows_and_columns",
                                       "test_a_bad_row_is_nan_for_that_video_only")}


def test_every_kernel_of_the_multitask_file_is_covered():
    """tests/test_train_kernels_gpu.py keeps this table for train.hip; the multi-task kernel lives in csrc/multitask.hip and
    is held here the same way: every kernel the file defines is launched, named in COVERAGE, and its tests exist; and the
    step's ``loss_layer`` and both entry points reach it through ``va_ce_multitask``."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"//[^\n]*", "", open(os.path.join(root, "video_analytics_amd", "csrc", "multitask.hip")).read())
    launched = set(re.findall(r"\b(k_\w+)\s*(?:<[^;<>()]*>)?\s*<<<", src))
    defined = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(k_\w+)", src))
    assert launched == defined == set(COVERAGE), (launched, defined)
    tests = open(os.path.join(root, "tests", "test_multitask_gpu.py")).read()
    for names in COVERAGE.values():
        for name in names:
            assert re.search(r"^def %s\(" % name, tests, flags=re.M), name
    train = re.sub(r"//[^\n]*", "", open(os.path.join(root, "video_analytics_amd", "csrc", "train.hip")).read())
    assert len(re.findall(r"\bva_ce_multitask\(", train)) == 1 and len(re.findall(r"\bloss_layer\([^;]*&mt\)", train)) == 1
    assert len(re.findall(r"\bloss_layer\([^;]*, mt\)", train)) == 1  # train_step hands its heads on


# ---- check_heads, head_logits ----

def test_check_heads_known_answers_and_errors():
    from video_analytics_amd import vgg
    assert vgg.check_heads((51, 101), 152, "x") == (0, 51)
    assert vgg.check_heads([101], 101, "x") == (0,)
    assert vgg.check_heads((1, 2, 7), 10, "x") == (0, 1, 3)
    assert vgg.check_heads((3, 1, 5, 2, 4, 6, 8, 9), 38, "x") == (0, 3, 4, 9, 11, 15, 21, 29)
    assert vgg.check_heads((np.int64(4096), 1), 4097, "x") == (0, 4096)
    assert vgg.check_heads((51, 101), None, "x") == (0, 51)
    for heads, total in (((), 0), ((1,) * 9, 9), ((51, 0), 51), ((51, -1), 50), ((51.0, 101), 152), ((51, 101), 151),
                         ((51, 101), 101), ((True, 100), 101), (("51", 101), 152), (152, 152), (None, 152)):
        with pytest.raises(ValueError):
            vgg.check_heads(heads, total, "x")
    for heads in ((), (1,) * 9, (51, 0), (2.5,)):
        with pytest.raises(ValueError):
            vgg.check_heads(heads, None, "x")


def test_head_logits_is_the_slice():
    from video_analytics_amd import vgg
    heads = (3, 1, 5)
    for shape in ((9,), (4, 9), (2, 3, 9), (2, 3, 2, 9)):
        t = torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape)
        for task, (o, c) in enumerate(zip((0, 3, 4), heads)):
            got = vgg.head_logits(t, heads, task)
            assert got.is_contiguous() and torch.equal(got, t[..., o:o + c]) and got.shape[-1] == c
    t = torch.zeros(2, 9)
    for heads_, task in (((3, 1, 5), 3), ((3, 1, 5), -1), ((3, 1, 4), 0), ((3, 1, 5), 1.0), ((3, 1, 5), True), ((3, 1, 5), None)):
        with pytest.raises(ValueError):
            vgg.head_logits(t, heads_, task)
    with pytest.raises(ValueError):
        vgg.head_logits([0.0] * 9, (3, 1, 5), 0)


def test_check_tasks_on_the_host():
    from video_analytics_amd import vgg
    heads = (51, 101)
    labels, tasks = vgg.check_tasks([50, 100, 0], [0, 1, 1], heads, 3, "x")
    assert labels.dtype == torch.int64 and tasks.dtype == torch.int32 and tasks.tolist() == [0, 1, 1]
    vgg.check_tasks(torch.tensor([50, 100]), torch.tensor([0, 1], dtype=torch.int32), heads, 2, "x")
    with pytest.raises(ValueError, match="out of bounds for 51 classes"):
        vgg.check_tasks([51, 100, 0], [0, 1, 1], heads, 3, "x")     # 51 is a label of head 1, not of head 0
    with pytest.raises(ValueError, match="out of bounds for 101 classes"):
        vgg.check_tasks([50, 101, 0], [0, 1, 1], heads, 3, "x")
    with pytest.raises(ValueError, match="out of bounds"):
        vgg.check_tasks([50, -1, 0], [0, 1, 1], heads, 3, "x")
    for bad in ([0, 2, 1], [0, -1, 1]):
        with pytest.raises(ValueError, match="not one of the 2 heads"):
            vgg.check_tasks([0, 0, 0], bad, heads, 3, "x")
    for bad_l, bad_t in (([0, 0], [0, 1, 1]), ([0, 0, 0], [0, 1]), ([0, 0, 0], None), (None, [0, 1, 1]), ([0, 0, 0], ["a", 1, 1]),
                         (torch.zeros(3), [0, 1, 1]), ([0, 0, 0], torch.zeros(3))):
        with pytest.raises(ValueError):
            vgg.check_tasks(bad_l, bad_t, heads, 3, "x")


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


def _bare_pipeline(heads, diff=False):
    """A pipeline object without a device behind it: only what the host checks read."""
    from video_analytics_amd import pipeline
    pipe = pipeline.TwoStreamPipeline.__new__(pipeline.TwoStreamPipeline)
    pipe.L, pipe.D, pipe.motion, pipe.mean_flow, pipe.camera, pipe._n = 10, 5, "stack", False, "none", 0
    pipe.device = torch.device("cpu")
    pipe.heads = heads
    n_classes = 101 if heads is None else sum(heads)
    pipe.diff = types.SimpleNamespace(dtype="f32", n_classes=n_classes) if diff else None
    pipe.spatial = pipe.temporal = types.SimpleNamespace(dtype="f32", n_classes=n_classes)
    return pipe


def test_the_constructor_refuses_bad_heads_on_the_host(no_gpu_calls, monkeypatch):
    import inspect
    from video_analytics_amd import pipeline

    def boom(*a, **k):
        raise AssertionError("reached the GPU")
    assert inspect.signature(pipeline.build_stream_weights).parameters["n_classes"].default == 101
    monkeypatch.setattr(pipeline, "build_stream_weights", boom)
    monkeypatch.setattr(pipeline.vgg, "Vgg16Stream", boom)
    for heads in ((), (1,) * 9, (51, 0), (51.0, 101), 152, (True, 3)):
        with pytest.raises(ValueError, match="TwoStreamPipeline"):
            pipeline.TwoStreamPipeline(device=0, heads=heads)
    p = inspect.signature(pipeline.TwoStreamPipeline.__init__).parameters
    assert p["heads"].default is None
    for f, name in ((pipeline.TwoStreamPipeline.train_videos, "tasks"), (pipeline.TwoStreamPipeline.submit_video, "task"),
                    (pipeline.TwoStreamPipeline.run_video, "task")):
        assert inspect.signature(f).parameters[name].default is None


@pytest.mark.parametrize("diff", [False, True])
def test_train_videos_refuses_bad_tasks_on_the_host(no_gpu_calls, diff):
    rgb, gray = torch.zeros(25, 3, 240, 320, dtype=torch.uint8), torch.zeros(25, 240, 320, dtype=torch.uint8)
    vids = [(rgb, gray), (rgb, gray)]
    plain, multi = _bare_pipeline(None, diff), _bare_pipeline((51, 101), diff)
    with pytest.raises(ValueError, match="tasks= needs a pipeline built with heads="):
        plain.train_videos(vids, [1, 2], k=3, tasks=[0, 1])
    with pytest.raises(ValueError, match="tasks= must name every video's head"):
        multi.train_videos(vids, [1, 2], k=3)
    for bad in ([0, 2], [-1, 1]):
        with pytest.raises(ValueError, match="not one of the 2 heads"):
            multi.train_videos(vids, [1, 2], k=3, tasks=bad)
    with pytest.raises(ValueError, match="out of bounds for 51 classes"):
        multi.train_videos(vids, [51, 2], k=3, tasks=[0, 1])
    with pytest.raises(ValueError, match="out of bounds for 101 classes"):
        multi.train_videos(vids, [50, 101], k=3, tasks=[0, 1])
    with pytest.raises(ValueError, match="out of bounds"):
        multi.train_videos(vids, [50, -1], k=3, tasks=[0, 1])
    for bad in ([0], [0, 1, 1], torch.zeros(2, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"tasks must be \[2\]"):
            multi.train_videos(vids, [1, 2], k=3, tasks=bad)
    with pytest.raises(ValueError, match=r"labels must be \[2\]"):
        multi.train_videos(vids, [1], k=3, tasks=[0, 1])
    with pytest.raises(ValueError, match="tasks must be"):
        multi.train_videos(vids, [1, 2], k=3, tasks=[0.5, "a"])
    # good tasks (and none on a plain pipeline) pass the new rules and stop at the next one: the videos are on the host
    for pipe, kw in ((multi, dict(tasks=[0, 1])), (multi, dict(tasks=torch.tensor([1, 1], dtype=torch.int32))), (plain, {})):
        with pytest.raises(ValueError, match="must be on"):
            pipe.train_videos(vids, [50, 100], k=3, **kw)


@pytest.mark.parametrize("diff", [False, True])
def test_run_video_refuses_a_bad_task_on_the_host(no_gpu_calls, diff):
    from video_analytics_amd import augment
    rgb, gray = torch.zeros(37, 3, 240, 320, dtype=torch.uint8), torch.zeros(37, 240, 320, dtype=torch.uint8)
    v = augment.ten_crop_views(240, 320)
    plain, multi = _bare_pipeline(None, diff), _bare_pipeline((51, 101), diff)
    for call in (multi.run_video, multi.submit_video):
        with pytest.raises(ValueError, match="task= must name the video's head"):
            call(rgb, gray, views=(v, v))
        for bad in (2, -1, 1.0, True, "0"):
            with pytest.raises(ValueError, match="task must be the index of one of the 2 heads"):
                call(rgb, gray, views=(v, v), task=bad)
    for call in (plain.run_video, plain.submit_video):
        with pytest.raises(ValueError, match="task= needs a pipeline built with heads="):
            call(rgb, gray, views=(v, v), task=0)
    for pipe, kw in ((multi, dict(task=0)), (multi, dict(task=1)), (plain, {})):
        with pytest.raises(ValueError, match="must be on"):
            pipe.run_video(rgb, gray, views=(v, v), **kw)
