"""Bag of words without a device: the numpy restatement of tests/codebook_oracle.py against scikit-learn's Lloyd iterations
and against literal per-row witnesses, then the host side of ``video_analytics_amd.codebook`` and ``stip.StipClassifier`` --
argument checks, the stopping rule, ``n_init`` selection, file formats and the binding."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import codebook_oracle as co  # noqa: E402
from video_analytics_amd import codebook as _product  # noqa: E402,F401  (what this file is about: without it nothing here runs)

CAP = 1e-9
# the largest deviation of the restatement's centres from scikit-learn's over the cases of this file (absolute: the rows
# have unit norm), as measured where this file was written
RECORDED = {"sklearn": 2.22e-16}


def unit_rows(n, d, seed):
    """non-negative float32 rows of unit norm, as Sheet01's normalised HOG/HOF descriptors are"""
    rng = np.random.RandomState(seed)
    x = rng.rand(n, d) ** 3
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


SKLEARN_CASES = [(6000, 144, 64), (5000, 144, 256), (3000, 30, 17)]


@pytest.mark.parametrize("n,d,k", SKLEARN_CASES)
def test_the_restatement_follows_sklearns_lloyd_iterations(n, d, k):
    cluster = pytest.importorskip("sklearn.cluster")
    x = unit_rows(n, d, 7 * n + k)
    c0 = x[np.random.RandomState(k).permutation(n)[:k]].astype(np.float64)
    x64 = x.astype(np.float64)
    for steps in (1, 5, 20):
        got, least, _gap = co.lloyd(x, c0, steps)
        assert least > 0, "a cluster emptied: the two sides differ there by design"
        km = cluster.KMeans(n_clusters=k, init=c0.copy(), n_init=1, algorithm="lloyd", tol=0, max_iter=steps).fit(x64.copy())
        dev = float(np.abs(got - km.cluster_centers_).max())
        print("DEV sklearn n=%d d=%d k=%d steps=%d %.3e" % (n, d, k, steps, dev))
        assert dev <= min(16.0 * RECORDED["sklearn"], CAP), dev


def test_the_restatement_against_a_literal_witness():
    for n, d, k, seed in ((200, 7, 5, 0), (150, 30, 17, 1), (64, 1, 3, 2), (50, 144, 50, 3)):
        x = unit_rows(n, max(d, 2), seed)[:, :d]
        c = x[np.random.RandomState(seed).permutation(n)[:k]].astype(np.float64) + 1e-3
        labels, d2, s = co.assign(x, c)
        want, want_d2 = co.assign_witness(x, c)
        decided = co.gaps(s, co.score_scale(x, c)) > 1e-9
        assert decided.mean() > 0.99
        assert np.array_equal(labels[decided], want[decided])
        assert np.abs(d2[decided] - want_d2[decided]).max() <= 1e-13 * max(1.0, float(want_d2.max()))
        assert (d2 >= 0).all()
    # a planted tie goes to the lower index, and a row equal to a centre is at distance exactly 0
    x = unit_rows(40, 12, 9)
    c = np.concatenate([x[:6].astype(np.float64), x[2:4].astype(np.float64)])
    labels, d2, _s = co.assign(x, c)
    assert labels[2] == 2 and labels[3] == 3 and (d2[:6] == 0.0).all()
    counts, sums, new, shift2, _abs = co.update(x, labels, c)
    assert counts[6] == 0 and counts[7] == 0 and np.array_equal(new[6:], c[6:])  # an empty cluster keeps its centre
    assert counts.sum() == 40 and shift2 >= 0.0
    for j in range(6):
        assert np.allclose(sums[j], x[labels == j].astype(np.float64).sum(axis=0), rtol=0, atol=1e-13)


def test_seeding_against_a_per_row_restatement():
    for n, d, k, seed in ((1, 3, 1, 0), (64, 5, 9, 1), (65, 2, 20, 2), (300, 4, 12, 3), (600, 3, 7, 4)):
        x = unit_rows(n, max(d, 2), 10 + seed)[:, :d]
        u = np.random.RandomState(seed).random_sample(k)
        rows, centres, m = co.seed(x, k, u)
        want_rows, want_m = co.seed_witness(x, k, u)
        assert np.array_equal(rows, want_rows), (n, d, k)
        assert np.array_equal(m, want_m)
        assert np.array_equal(centres, x[rows].astype(np.float64))
    # duplicated rows: once every distinct row is a centre the total is 0 and the row is floor(u n)
    x = np.repeat(unit_rows(3, 4, 5), 4, axis=0)
    u = np.random.RandomState(0).random_sample(6)
    rows, _c, m = co.seed(x, 6, u)
    want_rows, _m = co.seed_witness(x, 6, u)
    assert np.array_equal(rows, want_rows) and (m == 0.0).all()
    assert len(set(r // 4 for r in rows[:3])) == 3
    assert [int(r) for r in rows[4:]] == [int(np.floor(v * 12)) for v in u[4:]]


def test_seeding_picks_every_one_of_three_separated_points():
    x = np.array([[0.0, 0.0], [100.0, 0.0], [0.0, 100.0]], dtype=np.float32)
    firsts = set()
    for seed in range(200):
        u = np.random.RandomState(seed).random_sample(3)
        rows, _c, _m = co.seed(x, 3, u)
        assert sorted(rows.tolist()) == [0, 1, 2], (seed, rows)
        firsts.add(int(rows[0]))
    assert firsts == {0, 1, 2}  # floor(u_0 n) reaches every row


def test_histograms_of_the_restatement():
    labels = np.array([0, 2, 2, 1, 2, 0, 0], dtype=np.int32)
    seg = np.array([0, 0, 3, 3, 7, 7])
    h, counts = co.histograms(labels, seg, 4, "l2")
    assert counts.tolist() == [[0, 0, 0, 0], [1, 0, 2, 0], [0, 0, 0, 0], [2, 1, 1, 0], [0, 0, 0, 0]]
    assert np.array_equal(h[1], np.array([1, 0, 2, 0]) / np.sqrt(5.0)) and not h[0].any() and not h[4].any()
    assert np.array_equal(co.histograms(labels, seg, 4, "l1")[0][3], np.array([2, 1, 1, 0]) / 4.0)
    assert np.array_equal(co.histograms(labels, seg, 4, "none")[0], counts.astype(np.float64))


# ---- the host side of the library ---------------------------------------------------------------------------------------------

def test_the_stopping_rule_and_its_variance_scale():
    from video_analytics_amd import codebook
    x = unit_rows(500, 9, 3).astype(np.float64)
    xtx = np.triu(x.T @ x)  # what fisher.pca_moments returns: the upper triangle
    got = codebook.tolerance(float(len(x)), x.sum(axis=0), xtx, 1e-4)
    want = 1e-4 * np.mean(np.var(x, axis=0))
    assert abs(got - want) <= 1e-12 * want and abs(co.tolerance(x, 1e-4) - want) <= 1e-15 * want
    assert codebook.tolerance(4.0, np.array([4.0]), np.array([[4.0]]), 1.0) == 0.0  # a constant column
    stop = codebook.lloyd_stop
    assert stop(1, None, 1.0, 0.5, 300) == (False, False)        # the first step has no labels to compare with
    assert stop(2, 0, 1.0, 0.5, 300) == (True, True)             # no label changed
    assert stop(2, 3, 0.5, 0.5, 300) == (True, True)             # shift2 <= tol: sklearn's "<="
    assert stop(2, 3, 0.5000001, 0.5, 300) == (False, False)
    assert stop(300, 3, 1.0, 0.5, 300) == (True, False)          # max_iter: stopped, not converged
    assert stop(1, None, 0.0, 0.0, 300) == (True, True)          # tol = 0 still stops when nothing moved


def test_n_init_keeps_the_lowest_inertia_and_the_first_on_ties():
    from video_analytics_amd import codebook
    assert codebook.best_run([3.0]) == 0
    assert codebook.best_run([3.0, 2.0, 2.5]) == 1
    assert codebook.best_run([2.0, 3.0, 2.0]) == 0
    assert codebook.best_run([5.0, 4.0, 4.0, 4.0]) == 1


BAD_ARGS = [
    (dict(n_clusters=0), "n_clusters"), (dict(n_clusters=4097), "n_clusters"), (dict(n_clusters=2.0), "n_clusters"),
    (dict(n_clusters=True), "n_clusters"), (dict(n_clusters=101), "n_clusters"),  # n < K
    (dict(n_init=0), "n_init"), (dict(max_iter=0), "max_iter"), (dict(seed=-1), "seed"), (dict(seed=2 ** 32 - 1, n_init=2), "seed"),
    (dict(tol=-1e-4), "tol"), (dict(tol=float("nan")), "tol"), (dict(tol="x"), "tol"),
    (dict(init="kmeans"), "init"), (dict(init=np.zeros((4, 3))), "init"), (dict(init=np.full((8, 5), np.nan)), "init"),
    (dict(init=object()), "init"), (dict(d=0), "x"), (dict(d=513), "x"),
]


@pytest.mark.parametrize("over,name", BAD_ARGS, ids=["%d" % i for i in range(len(BAD_ARGS))])
def test_argument_errors_name_the_argument(over, name):
    from video_analytics_amd import codebook
    kw = dict(n=100, d=5, n_clusters=8, init="k-means++", n_init=1, max_iter=300, tol=1e-4, seed=0)
    codebook.check_kmeans_fit_args(**kw)
    codebook.check_kmeans_fit_args(**dict(kw, init="random", tol=0, n_clusters=100))
    codebook.check_kmeans_fit_args(**dict(kw, init=np.zeros((8, 5))))
    kw.update(over)
    with pytest.raises(ValueError, match="kmeans_fit: .*%s" % name):
        codebook.check_kmeans_fit_args(**kw)


def test_codebook_npz_round_trip(tmp_path):
    from video_analytics_amd import codebook
    rng = np.random.RandomState(0)
    cb = codebook.Codebook(rng.randn(7, 5), 12.5, 9, True, np.arange(7))
    path = str(tmp_path / "cb.npz")
    cb.save(path)
    back = codebook.Codebook.load(path)
    assert np.array_equal(back.centres, cb.centres) and back.centres.dtype == np.float64
    assert (back.inertia, back.n_iter, back.converged, back.n_words) == (12.5, 9, True, 7)
    assert np.array_equal(back.counts, np.arange(7)) and back.counts.dtype == np.int64
    with np.load(path) as z:
        assert sorted(z.files) == ["centres", "converged", "counts", "inertia", "n_iter"]
    for bad in (np.zeros((0, 5)), np.zeros(5), np.zeros((4097, 2)), np.zeros((2, 513))):
        with pytest.raises(ValueError, match="centres"):
            codebook.Codebook(bad)
    with pytest.raises(ValueError, match="counts"):
        codebook.Codebook(np.zeros((3, 2)), counts=np.zeros(4))


def test_stip_classifier_files_without_a_device(tmp_path):
    from video_analytics_amd import codebook, stip
    m = stip.StipClassifier()
    with pytest.raises(ValueError, match="not fitted"):
        m.save(str(tmp_path / "m.npz"))
    with pytest.raises(ValueError, match="not fitted"):
        m.predict([])
    with pytest.raises(ValueError, match="not fitted"):
        m.encode([])
    rng = np.random.RandomState(1)
    m.codebook = codebook.Codebook(rng.randn(6, 144), 3.0, 4, False, np.array([1, 2, 3, 0, 5, 6]))
    m.norm, m.coef, m.intercept, m.classes = "l1", rng.randn(3, 6), rng.randn(3), np.array(["a", "b", "c"])
    path = str(tmp_path / "m.npz")
    m.save(path)
    back = stip.StipClassifier.load(path)
    assert back.norm == "l1" and isinstance(back.norm, str)
    assert np.array_equal(back.codebook.centres, m.codebook.centres) and np.array_equal(back.codebook.counts, m.codebook.counts)
    assert (back.codebook.inertia, back.codebook.n_iter, back.codebook.converged) == (3.0, 4, False)
    assert np.array_equal(back.coef, m.coef) and np.array_equal(back.intercept, m.intercept) and back.classes.tolist() == ["a", "b", "c"]
    with np.load(path) as z:
        assert sorted(z.files) == ["centres", "classes", "coef", "converged", "counts", "inertia", "intercept", "n_iter", "norm"]
    for bad in ([], "x", [np.zeros((2, 3))]):
        with pytest.raises(ValueError, match="descs_per_video"):
            back.encode(bad)


def test_binding_struct_sizes_exports_and_limits():
    import __graft_entry__
    from video_analytics_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        __graft_entry__.build()
    L = _ffi.lib()
    names = ("va_kmeans_default_params", "va_kmeans_workspace_bytes", "va_kmeans_tile_centres", "va_kmeans_assign", "va_kmeans_update",
             "va_kmeans_seed", "va_bow_histograms", "va_bow_encode")
    for name in names:
        assert name in _ffi.EXPORTS and hasattr(L, name), name
    assert ctypes.sizeof(_ffi.KmeansParams) == 32
    p = _ffi.default_kmeans_params()
    assert (p.struct_bytes, p.chunk_rows) == (32, 8192) and not any(p.reserved)
    assert (_ffi.VA_BOW_NONE, _ffi.VA_BOW_L1, _ffi.VA_BOW_L2) == (0, 1, 2)
    assert L.va_kmeans_tile_centres() == 64
    hdr = open(os.path.join(os.path.dirname(_ffi.LIB_PATH), "..", "include", "va.h")).read()
    for text in ("#define VA_BOW_NONE 0", "#define VA_BOW_L1 1", "#define VA_BOW_L2 2", "int reserved[6];"):
        assert text in hdr
    # the limits: 0 and the field's name
    ok = L.va_kmeans_workspace_bytes(2 ** 31 - 1, 512, 4096, 65536, None)
    assert ok > 0
    for args, field in (((0, 4, 4, 1), "n out"), ((-1, 4, 4, 1), "n out"), ((10, 0, 4, 1), "d out"), ((10, 513, 4, 1), "d out"),
                        ((10, 4, 0, 1), "k out"), ((10, 4, 4097, 1), "k out"), ((10, 4, 4, 0), "n_segments"), ((10, 4, 4, 65537), "n_segments")):
        assert L.va_kmeans_workspace_bytes(*args, None) == 0, args
        assert field in L.va_last_error().decode(), (args, L.va_last_error())
    for chunk in (63, 2 ** 20 + 1):
        with pytest.raises(ValueError, match="chunk_rows"):
            _ffi.default_kmeans_params(chunk_rows=chunk)
    short = _ffi.KmeansParams(16, 8192)
    assert L.va_kmeans_workspace_bytes(10, 4, 4, 1, ctypes.byref(short)) == 0 and b"struct_bytes" in L.va_last_error()
    # the workspace grows with n only by O(n) integers: nothing of size n x K
    small, big = L.va_kmeans_workspace_bytes(100000, 144, 4096, 1, None), L.va_kmeans_workspace_bytes(1100000, 144, 4096, 1, None)
    assert (big - small) / 1e6 <= 16.0  # bytes per added row: two int32, two float64 / 256, K int32 / chunk_rows
    # no result depends on chunk_rows; the size does
    assert L.va_kmeans_workspace_bytes(100000, 144, 4096, 1, ctypes.byref(_ffi.default_kmeans_params(chunk_rows=64))) > small
