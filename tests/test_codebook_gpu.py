"""Bag of words on the device (csrc/codebook.hip) against the numpy restatement of tests/codebook_oracle.py:
every kernel on its own, then ``kmeans_fit`` and ``StipClassifier`` end to end.

Labels are held by the gap rule: a row is decided when the restatement's second-best score exceeds its best by more than
``GAP x scale_i``, ``scale_i = max_j sum_c |x_ic c_jc| + 1/2 max_j |c_j|^2``; on decided rows the labels are equal, on the
others the device's choice scores within that margin of the best, and at most 0.1 % of a case's rows may be undecided (a
condition on the inputs, asserted on the restatement).  ``d2``, the seeding's rows and ``m`` and the histograms' counts are
exact.  What is summed in another order -- centres, ``shift2``, the inertia -- is scaled by the sum of the absolute values
of its terms and ``hold`` asserts 16 x the largest scaled deviation recorded on an MI355X over the cases of this file
(``RECORDED``), never more than 1e-9.  float32 outputs get ``hold32`` of test_fisher_gpu.py: 1 ulp for the rounding."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import codebook_oracle as co  # noqa: E402

pytestmark = pytest.mark.gpu

CAP, GAP = 1e-9, 1e-9
# the largest scaled deviation from the restatement over the cases of this file, recorded on an MI355X
RECORDED = {
    "centres": 5.16e-16,     # updated centres / (sum |x| of the cluster / its count)
    "shift2": 7.78e-16,      # shift2 / itself (a sum of squares)
    "inertia": 3.29e-16,     # the inertia / itself (a sum of squares)
    "hist": 0.0,             # histograms beyond 1 ulp of float32 (scale 1)
    "fit_centres": 1.49e-16,  # centres of kmeans_fit / the largest magnitude of the restatement's
    "fit_inertia": 3.30e-16,  # inertia of kmeans_fit / itself
}
SEEN = {}


def hold(name, got, want, scale):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isfinite(got).all(), name
    diff = np.abs(got - want)
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), diff.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, diff / scale, np.where(diff > 0, np.inf, 0.0))
    dev = float(rel.max()) if rel.size else 0.0
    SEEN[name] = max(SEEN.get(name, 0.0), dev)
    print("DEV %s %.3e (largest so far %.3e)" % (name, dev, SEEN[name]))
    assert dev <= min(16.0 * RECORDED[name], CAP), (name, dev)


def hold32(name, got32, want64, scale):
    """float32 output against the float64 reference rounded to float32: 1 ulp is free, the rest is held like a float64"""
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32
    w32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    ulp = np.spacing(np.abs(w32)).astype(np.float64)
    excess = np.maximum(np.abs(got32.astype(np.float64) - w32.astype(np.float64)) - ulp, 0.0)
    hold(name, excess, np.zeros_like(excess), scale)


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def cpu(t):
    return t.cpu().numpy()


def rows(n, d, seed):
    """non-negative float32 rows, of unit norm when there are columns enough for that to leave them distinct"""
    rng = np.random.RandomState(seed)
    x = rng.rand(n, d)
    if d >= 8:
        x = x ** 3
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def centres_for(x, k, seed):
    """k centres drawn from the rows, or from their distribution when there are fewer rows than that"""
    n, d = x.shape
    if k <= n:
        return x[np.random.RandomState(seed).permutation(n)[:k]].astype(np.float64)
    return rows(k, d, seed + 1).astype(np.float64)


def check_assign(x, c, labels, d2):
    want, _want_d2, s = co.assign(x, c)
    scale = co.score_scale(x, c)
    gap = co.gaps(s, scale)
    decided = gap > GAP
    share = 1.0 - float(decided.mean())
    print("GAP smallest %.3e undecided share %.2e" % (float(gap.min()), share))
    assert share <= 1e-3, share
    assert labels.dtype == np.int32 and labels.min() >= 0 and labels.max() < len(c)
    assert np.array_equal(labels[decided], want[decided])
    idx = np.arange(len(x))
    assert (s[idx, labels] - s.min(axis=1) <= GAP * scale).all()
    assert np.array_equal(d2, co.direct_d2(x, c, labels))  # bit for bit given the label
    assert (d2 >= 0).all()
    return want


# ---- assignment ---------------------------------------------------------------------------------------------------------------

TILE = 64  # va_kmeans_tile_centres(), asserted below
ASSIGN_CASES = [
    (1, 1, 1), (1, 144, 256), (15, 3, 2), (15, 512, 16), (16, 4, 15), (16, 1, 17), (17, 5, 16), (17, 3, 255), (63, 143, 17), (63, 4, 256),
    (64, 144, 255), (64, 5, 257), (65, 145, 256), (65, 143, 1000), (1000, 512, 257), (1000, 144, 15), (1000, 3, 4096), (1000, 145, 2),
    (5000, 144, 1000), (5000, 1, 16), (5000, 4, 1), (5000, 512, 4096),
    (65, 4, TILE - 1), (63, 5, TILE), (17, 144, TILE + 1), (1000, 143, TILE - 1), (64, 512, TILE), (16, 145, TILE + 1),
    (5000, 3, 2 * TILE - 1), (1000, 5, 2 * TILE + 1), (64, 1, 2 * TILE),
]


@pytest.mark.parametrize("n,d,k", ASSIGN_CASES)
def test_assign(n, d, k):
    """rows at 1, 15 .. 17, 63 .. 65 (one 16-row block, one wave, one workgroup of 128, more) and 1000, 5000; columns at 1,
    3 .. 5, 143 .. 145 (a ragged 64-column tile) and 512; centres at 1, 2, 15 .. 17 (one MFMA column group), 255 .. 257, 1000,
    4096 and around one and two tiles of 64"""
    from video_analytics_amd import _ffi, codebook
    assert _ffi.lib().va_kmeans_tile_centres() == TILE
    x = rows(n, d, 100 * n + d + k)
    c = centres_for(x, k, k + d)
    labels, d2, inertia, changed = codebook.assign(dev(x), c)
    labels, d2 = cpu(labels), cpu(d2)
    check_assign(x, c, labels, d2)
    assert int(changed.item()) == n
    hold("inertia", cpu(inertia)[0], d2.sum(), d2.sum())
    # a second call: the same bits; the rows that moved against labels shifted by one place; no d2 when it is not asked for
    prev = np.roll(labels, 1)
    again, none, inertia2, moved = codebook.assign(dev(x), c, dev(prev), want_d2=False)
    assert none is None and np.array_equal(cpu(again), labels) and cpu(inertia2)[0] == cpu(inertia)[0]
    assert int(moved.item()) == int((prev != labels).sum())


def test_assign_planted_ties():
    """duplicated centres: in one lane (columns 3 and 19 of a tile), across the lanes of one butterfly (5 and 9), across two
    tiles (2 and 70; 66 and 130) -- the lowest index wins exactly, and a row equal to a centre is at distance 0.0"""
    from video_analytics_amd import codebook
    x = rows(200, 144, 5)
    c = x[:140].astype(np.float64)
    c[19], c[9], c[70], c[130] = c[3], c[5], c[2], c[66]
    pick = np.random.RandomState(0).choice([3, 5, 2, 66], size=320)  # each of them in every lane group and both row blocks
    labels, d2, _i, _ch = codebook.assign(dev(x[pick]), c)
    assert np.array_equal(cpu(labels), pick.astype(np.int32))
    assert (cpu(d2) == 0.0).all()
    # all centres equal: every row takes centre 0
    same = np.repeat(c[:1], 200, axis=0)
    labels, _d2, _i, _ch = codebook.assign(dev(x), same)
    assert not cpu(labels).any()


def test_assign_agrees_with_the_mixtures_hard_posteriors():
    """GMMModel.posteriors(mode="hard") at equal weights and unit variances: an independent device implementation"""
    from video_analytics_amd import codebook, fisher
    x = rows(3000, 30, 8)
    for k in (17, 256):
        c = centres_for(x, k, k)
        labels = cpu(codebook.assign(dev(x), c)[0])
        g = fisher.GMMModel(np.full(k, 1.0 / k), c, np.ones_like(c)).posteriors(dev(x), "hard")
        _l, _d2, s = co.assign(x, c)
        decided = co.gaps(s, co.score_scale(x, c)) > GAP
        assert decided.mean() >= 0.999
        assert np.array_equal(np.argmax(g, axis=1)[decided], labels[decided])


# ---- update -------------------------------------------------------------------------------------------------------------------

def check_update(x, labels, c, got):
    counts, new, shift2 = (cpu(t) for t in got)
    want_counts, _sums, want_new, want_shift2, abs_sums = co.update(x, labels, c)
    assert counts.dtype == np.int64 and np.array_equal(counts, want_counts)
    full = want_counts > 0
    hold("centres", new[full], want_new[full], abs_sums[full] / want_counts[full, None])
    assert np.array_equal(new[~full], c[~full])  # an empty cluster keeps its centre, bits unchanged
    terms = ((want_new - c) ** 2).sum()
    hold("shift2", shift2[0], want_shift2, terms)
    return counts, new, shift2


UPDATE_CASES = [("random", 5000, 144, 256), ("empties", 1000, 5, 4096), ("one_each", 65, 3, 65), ("all_in_one", 5000, 145, 3),
                ("random", 1000, 512, 17), ("random", 17, 1, 2)]


@pytest.mark.parametrize("kind,n,d,k", UPDATE_CASES)
def test_update(kind, n, d, k):
    from video_analytics_amd import codebook
    x = rows(n, d, n + d + k)
    rng = np.random.RandomState(k)
    c = rows(k, d, 77).astype(np.float64)
    if kind == "one_each":
        labels = rng.permutation(n).astype(np.int32)
    elif kind == "all_in_one":
        labels = np.full(n, 1, dtype=np.int32)
    else:
        labels = rng.randint(0, k, size=n).astype(np.int32)
        if k > 2:
            labels[labels == 2] = 0  # a planted empty cluster
    first = check_update(x, labels, c, codebook.update(dev(x), dev(labels), c))
    if kind in ("empties", "all_in_one") or k > 2 and kind == "random":
        assert (first[0] == 0).any()
    for chunk in (64, 256, 1024, None):  # the same bits under every chunk size and on a second call
        again = codebook.update(dev(x), dev(labels), c, chunk_rows=chunk)
        for a, b in zip(first, again):
            assert np.array_equal(a, cpu(b)), chunk


def test_update_after_assign_moves_the_centres_to_the_means():
    from video_analytics_amd import codebook
    x = rows(5000, 144, 21)
    c = centres_for(x, 256, 3)
    labels = codebook.assign(dev(x), c)[0]
    counts, new, _shift2 = check_update(x, cpu(labels), c, codebook.update(dev(x), labels, c))
    assert counts.sum() == 5000 and counts.min() >= 1  # every centre is a row, so no cluster is empty


# ---- seeding ------------------------------------------------------------------------------------------------------------------

SEED_CASES = [(1, 3, 1), (64, 5, 64), (65, 144, 30), (5000, 144, 300), (5000, 3, 17), (64, 1, 2)]


@pytest.mark.parametrize("n,d,k", SEED_CASES)
def test_seed(n, d, k):
    from video_analytics_amd import codebook
    x = rows(n, d, 31 * n + d)
    u = np.random.RandomState(n + k).random_sample(k)
    want_rows, want_centres, want_m = co.seed(x, k, u)
    centres, picked, m = codebook.seed(dev(x), k, u)
    assert np.array_equal(cpu(picked), want_rows)
    assert np.array_equal(cpu(centres), want_centres)
    assert np.array_equal(cpu(m), want_m)  # bit for bit after the last step
    again = codebook.seed(dev(x), k, u)
    assert torch.equal(again[1], picked) and torch.equal(again[2], m)


def test_seed_on_duplicated_rows():
    """fewer distinct rows than centres: once every distinct row is chosen the total is 0 and the row is floor(u n)"""
    from video_analytics_amd import codebook
    x = np.repeat(rows(3, 4, 5), 100, axis=0)  # 300 rows: two blocks of 256
    u = np.random.RandomState(0).random_sample(7)
    want_rows, want_centres, want_m = co.seed(x, 7, u)
    centres, picked, m = codebook.seed(dev(x), 7, u)
    assert np.array_equal(cpu(picked), want_rows) and np.array_equal(cpu(centres), want_centres)
    assert np.array_equal(cpu(m), want_m) and not want_m.any()
    assert [int(r) for r in want_rows[3:]] == [int(np.floor(v * 300)) for v in u[3:]]


# ---- histograms ---------------------------------------------------------------------------------------------------------------

def segments_with_empties(n, s, seed):
    """s segments over n rows, the first, the last and some in the middle empty"""
    rng = np.random.RandomState(seed)
    cuts = np.sort(rng.randint(0, n + 1, size=s - 1))
    seg = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    if s >= 5:
        seg[1] = 0
        seg[-2] = n
        seg[s // 2 + 1] = seg[s // 2]
    return seg


@pytest.mark.parametrize("norm", ["l2", "l1", "none"])
@pytest.mark.parametrize("n,k,s", [(5000, 256, 300), (1000, 4096, 1), (777, 17, 7), (64, 1, 5), (3000, 1000, 40)])
def test_histograms(n, k, s, norm):
    from video_analytics_amd import codebook
    labels = np.random.RandomState(n + k).randint(0, k, size=n).astype(np.int32)
    seg = segments_with_empties(n, s, s)
    want, counts = co.histograms(labels, seg, k, norm)
    got = cpu(codebook.bow_histograms(dev(labels), seg, k, norm))
    assert got.shape == (s, k) and got.dtype == np.float32
    if s >= 5:
        empty = np.diff(seg) == 0
        assert empty[0] and empty[-1] and empty[1:-1].any() and not got[empty].any()
    if norm == "none":
        assert np.array_equal(got, counts.astype(np.float32))  # integer-exact
    hold32("hist", got, want, 1.0)
    raw = cpu(codebook.bow_histograms(dev(labels), seg, k, "none"))
    assert np.array_equal(raw.astype(np.int64), counts)


def test_encode_is_assignment_followed_by_histograms():
    from video_analytics_amd import codebook
    x = rows(5000, 144, 4)
    c = centres_for(x, 257, 9)
    seg = segments_with_empties(5000, 100, 2)
    labels = codebook.assign(dev(x), c)[0]
    for norm in ("l2", "l1", "none"):
        assert torch.equal(codebook.bow_encode(dev(x), seg, c, norm), codebook.bow_histograms(labels, seg, 257, norm))
    cb = codebook.Codebook(c)
    assert torch.equal(cb.histograms(dev(x), seg), codebook.bow_histograms(labels, seg, 257, "l2"))
    assert torch.equal(cb.assign(dev(x)), labels)
    none = torch.empty((0, 144), dtype=torch.float32, device="cuda")
    assert cb.assign(none).shape == (0,) and not cpu(cb.histograms(none, [0, 0, 0])).any()
    for bad in (dict(norm="max"), dict(segments=[0, 10])):
        with pytest.raises(ValueError):
            cb.histograms(dev(x), **dict(dict(segments=seg, norm="l2"), **bad))


# ---- kmeans_fit ---------------------------------------------------------------------------------------------------------------

FIT = {}


def fit_data():
    if not FIT:
        x = rows(3000, 30, 12)
        FIT["x"], FIT["c0"] = x, centres_for(x, 17, 5)
    return FIT["x"], FIT["c0"]


def check_fit(got, want):
    assert want["min_gap"] > GAP, want["min_gap"]  # the inputs decide every row at every iteration
    assert (got.n_iter, got.converged) == (want["n_iter"], want["converged"])
    assert np.array_equal(got.counts, want["counts"])
    hold("fit_centres", got.centres, want["centres"], np.abs(want["centres"]).max())
    hold("fit_inertia", got.inertia, want["inertia"], want["inertia"])


@pytest.mark.parametrize("steps", [1, 2, 10])
def test_kmeans_fit_steps_from_a_given_init(steps):
    from video_analytics_amd import codebook
    x, c0 = fit_data()
    want = co.fit(x, c0, max_iter=steps, tol=0.0)
    assert want["n_iter"] == steps and not want["converged"]
    check_fit(codebook.kmeans_fit(dev(x), 17, init=c0, max_iter=steps, tol=0.0), want)


def test_kmeans_fit_converges():
    from video_analytics_amd import codebook
    x, c0 = fit_data()
    want = co.fit(x, c0)
    assert want["converged"] and 2 < want["n_iter"] < 300
    check_fit(codebook.kmeans_fit(dev(x), 17, init=c0), want)
    strict = co.fit(x, c0, tol=0.0)  # tol = 0: runs until no label changes
    assert strict["converged"] and strict["n_iter"] >= want["n_iter"]
    got = codebook.kmeans_fit([dev(x[:1000]), torch.empty((0, 30), dtype=torch.float32, device="cuda"), dev(x[1000:])], 17, init=c0, tol=0.0)
    check_fit(got, strict)


@pytest.mark.parametrize("init", ["k-means++", "random"])
def test_kmeans_fit_end_to_end(init):
    from video_analytics_amd import codebook
    x, _c0 = fit_data()
    if init == "k-means++":
        c0 = co.seed(x, 17, np.random.RandomState(3).random_sample(17))[1]
    else:
        c0 = x[np.random.RandomState(3).permutation(len(x))[:17]].astype(np.float64)
    want = co.fit(x, c0, max_iter=25)
    got = codebook.kmeans_fit(dev(x), 17, init=init, seed=3, max_iter=25)
    check_fit(got, want)
    best = codebook.kmeans_fit(dev(x), 17, init=init, seed=3, max_iter=25, n_init=2)  # seeds 3 and 4
    other = codebook.kmeans_fit(dev(x), 17, init=init, seed=4, max_iter=25)
    assert best.inertia == min(got.inertia, other.inertia)
    with pytest.raises(ValueError, match="n_clusters"):
        codebook.kmeans_fit(dev(x[:10]), 17)


# ---- StipClassifier -------------------------------------------------------------------------------------------------------------

def planted_videos(seed, per_class=6):
    """three classes of videos: a class draws its descriptors around four prototypes of its own"""
    rng = np.random.RandomState(seed)
    protos = rows(12, 144, 50)
    videos, labels = [], []
    for cls in range(3):
        for _ in range(per_class):
            which = rng.randint(4 * cls, 4 * cls + 4, size=rng.randint(40, 80))
            v = protos[which] + 0.01 * rng.randn(len(which), 144).astype(np.float32)
            videos.append(v.astype(np.float32))
            labels.append("class%d" % cls)
    return videos, labels


def test_stip_classifier_on_planted_classes(tmp_path):
    from video_analytics_amd import stip
    videos, labels = planted_videos(0)
    videos.append(np.zeros((0, 144), dtype=np.float32))  # a video without points
    labels.append("class0")
    dv = [dev(v) for v in videos]
    m = stip.StipClassifier().fit(dv, labels, n_words=12, seed=1)
    assert m.codebook.n_words == 12 and m.codebook.counts.sum() == sum(len(v) for v in videos)
    h = cpu(m.encode(dv))
    assert h.shape == (19, 12) and not h[-1].any() and np.allclose(np.linalg.norm(h[:-1], axis=1), 1.0, atol=1e-6)
    pred = m.predict(dv)
    assert list(pred[:-1]) == labels[:-1] and len(pred) == 19
    test_videos, test_labels = planted_videos(1)
    assert list(m.predict([dev(v) for v in test_videos])) == test_labels
    path = str(tmp_path / "stip.npz")
    m.save(path)
    back = stip.StipClassifier.load(path)
    assert list(back.predict(dv)) == list(pred)
    assert torch.equal(back.encode(dv), m.encode(dv))
    with pytest.raises(ValueError, match="labels"):
        stip.StipClassifier().fit(dv, labels[:-1])
    with pytest.raises(ValueError, match="norm"):
        stip.StipClassifier().fit(dv, labels, norm="max")


def test_stip_classifier_from_interest_points():
    """the whole of Sheet01's chain once: detector and descriptors on the smallest scene, codebook, histograms, SVM"""
    import stip_scenes as scenes
    from video_analytics_amd import stip
    descs = []
    for seed in (3, 4, 5, 6):
        gray, flow, _event = scenes.events(seed=seed)
        out = stip.space_time_interest_points(dev(gray), dev(flow))  # 48 x 40 x 12, all twelve scale pairs: 15 to 32 points
        assert out["count"] >= 8 and out["desc"].shape[1] == 144
        descs.append(out["desc"])
    labels = [0, 1, 0, 1]
    m = stip.StipClassifier().fit(descs, labels, n_words=8)
    h = cpu(m.encode(descs))
    rows_all = np.concatenate([cpu(v) for v in descs])
    seg = np.concatenate([[0], np.cumsum([len(v) for v in descs])])
    want, _counts = co.histograms(cpu(m.codebook.assign(torch.cat(descs, 0))), seg, 8, "l2")
    hold32("hist", h, want, 1.0)
    assert len(rows_all) == seg[-1] and list(m.predict(descs)) == labels
