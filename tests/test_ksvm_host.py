"""The kernel SVM's numpy restatement (tests/ksvm_oracle.py) held to independent witnesses, and the host-side argument checks
of ``video_analytics_amd.ksvm``; no GPU.  The chi-square kernel is held to sklearn's, the solver to scipy's NNLS and to
``svm_fit_oracle.newton_cg`` through the two bounds strong convexity gives: ``|alpha - alpha*| <= 2C |pg|`` in the dual and
``|w - w*| <= |grad f(w)|`` in the primal.  No other tolerance enters."""
import numpy as np
import pytest
import torch

import ksvm_oracle as ko
import svm_fit_oracle as so
from video_analytics_amd import _ffi, ksvm

TOL = 1e-8


def test_chi2_restatement_against_sklearn_and_long_double():
    sk = pytest.importorskip("sklearn.metrics.pairwise")
    x, y = ko.histograms(40, 23, seed=0), ko.histograms(17, 23, seed=1)
    D = ko.chi2_distance(x, y)
    assert np.allclose(np.exp(-0.5 * D), sk.chi2_kernel(x, y, gamma=0.5), rtol=1e-13, atol=0)  # no factor 1/2 in D
    assert np.allclose(D, ko.chi2_distance_witness(x, y).astype(np.float64), rtol=1e-14, atol=0)
    S = ko.chi2_distance(x)
    assert np.array_equal(S, S.T) and not S.diagonal().any() and np.array_equal(S, ko.chi2_distance(x, x.copy()))
    assert np.allclose(ko.chi2_distance(x, y, (0, 7)) + ko.chi2_distance(x, y, (7, 23)), D, rtol=1e-14, atol=0)  # column ranges add up
    K, scales = ko.chi2_kernel(x, channels=[(0, 7), (7, 23)])
    assert (K.diagonal() == 1.0).all() and np.array_equal(K, K.T)
    assert np.allclose(scales, [1.0 / ko.upper_mean(ko.chi2_distance(x, None, ch)) for ch in [(0, 7), (7, 23)]], rtol=0, atol=0)
    assert np.allclose(ko.chi2_kernel(x, gamma=0.7)[0], sk.chi2_kernel(x, gamma=0.7), rtol=1e-13, atol=0)


def gpu_problems():
    """The problems tests/test_ksvm_gpu.py fits."""
    return [(name,) + ko.solver_problem(name) for name in ko.PROBLEMS]


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name, X, labels, C, s, kernel in gpu_problems():
        K = ko.linear_gram(X) if kernel == "linear" else ko.chi2_kernel(X)[0]
        out[name] = (X, labels, C, s, K) + ko.dual_fit(K, labels, C, TOL, 100, s)
    return out


def test_restated_solver_meets_the_stop_rule_on_every_gpu_problem(solved):
    want_zero = {"three_classes": 0.95, "sixty_five_classes": 0.82, "two_classes": 0.97}
    for name, (X, labels, C, s, K, beta, intercept, classes, info) in solved.items():
        Y = so.signs(labels, classes)
        n = len(labels)
        pg = ko.pg_norms(beta, K, Y, C, s)
        assert info["converged"] and info["n_iter"] <= 100 and (pg <= TOL * np.sqrt(n)).all(), (name, pg.max())
        assert (Y * beta >= 0.0).all()
        witness = ko.nnls_witness(K, Y, C, s)
        pgw = ko.pg_norms(witness, K, Y, C, s)
        assert (pgw <= 1e-10 * np.sqrt(n)).all(), (name, pgw.max())
        assert (np.linalg.norm(beta - witness, axis=1) <= 2.0 * C * (pg + pgw)).all(), name
        assert np.array_equal(intercept, s * s * beta.sum(1))
        zeros = (beta == 0.0).mean()
        if name in want_zero:  # the structure the problems were chosen for: most alpha at exactly zero, zeros in every row
            assert abs(zeros - want_zero[name]) < 0.03 and ((beta == 0.0).sum(1) > 0).all(), (name, zeros)
        if name == "tiny_C":
            assert (Y * beta > 0.0).all()
    steps = solved["sixty_five_classes"][8]["steps"]
    assert steps.max() - steps.min() >= 2  # rows finish several outer steps apart


def test_linear_kernel_solves_the_primal_problem(solved):
    """Fact 1: W = beta [X, s] minimises linear_svm_fit's f_r; against newton_cg within |grad f(W)| + |grad f(W_ref)|."""
    for name in ("three_classes", "two_classes", "wide", "no_intercept", "tiny_C"):
        X, labels, C, s, K, beta, intercept, classes, info = solved[name]
        W = ko.primal_weights(beta, X, s)
        coef, b, _, _, _ = so.newton_cg(X, labels, C=C, tol=1e-12, intercept_scaling=s)
        Wp = so.pack(coef, b, s)
        Xa, Y = so.augmented(X, s), so.signs(labels, classes)
        bound = np.linalg.norm(so.gradient(W, Xa, Y, C), axis=1) + np.linalg.norm(so.gradient(Wp, Xa, Y, C), axis=1)
        assert (np.linalg.norm(W - Wp, axis=1) <= bound).all(), name
        assert np.allclose(intercept, s * W[:, -1], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("i", range(so.N_PROBLEMS))
def test_linear_kernel_on_the_golden_problems(i):
    p = so.load_golden()[i]
    beta, intercept, classes, info = ko.dual_fit(ko.linear_gram(p["X"]), p["labels"], 1.0, TOL)
    assert info["converged"] and np.array_equal(classes, p["classes"])
    W, ref = ko.primal_weights(beta, p["X"]), so.pack(p["coef"], p["intercept"])
    Xa, Y = so.augmented(p["X"]), so.signs(p["labels"], classes)
    bound = np.linalg.norm(so.gradient(W, Xa, Y), axis=1) + np.linalg.norm(so.gradient(ref, Xa, Y), axis=1)
    assert (np.linalg.norm(W - ref, axis=1) <= bound).all()


def test_error_bound_holds_along_the_iterates():
    """Fact 2 on feasible points that are far from optimal: |alpha - alpha*| <= 2C |pg(alpha)|."""
    X, labels = ko.blobs(40, 5, 3, 2.0, seed=7)
    K, C = ko.linear_gram(X), 3.0
    Y = so.signs(labels, np.unique(labels))
    star = ko.nnls_witness(K, Y, C)
    rng = np.random.RandomState(0)
    for scale in (0.0, 1e-3, 1.0):
        beta = Y * np.maximum(0.0, Y * star + scale * rng.randn(*star.shape))
        pg = ko.pg_norms(beta, K, Y, C)
        assert (np.linalg.norm(beta - star, axis=1) <= 2.0 * C * (pg + ko.pg_norms(star, K, Y, C))).all()


K_OK = np.eye(4) + 1.0
BAD_FIT = [
    ("not_square", dict(K=np.ones((3, 4))), "square"), ("one_row", dict(K=np.ones((1, 1)), labels=[0]), "2 <= n"),
    ("three_d", dict(K=np.ones((2, 2, 2))), "square"), ("float32", dict(K=torch.ones(4, 4)), "float64"),
    ("too_many_rows", dict(K=torch.zeros(1, dtype=torch.float64).expand(16385, 16385), labels=np.arange(16385) % 2), "n <= 16384"),
    ("nan", dict(K=np.where(np.eye(4) > 0, np.nan, 1.0)), "non-finite"), ("inf", dict(K=K_OK * np.inf), "non-finite"),
    ("asymmetric", dict(K=K_OK + np.triu(np.ones((4, 4)), 1)), "not symmetric"),
    ("labels_short", dict(labels=[0, 1, 0]), "labels of shape"), ("one_label", dict(labels=[3, 3, 3, 3]), "2 .. 1024 distinct"),
    ("nan_label", dict(labels=[0.0, 1.0, np.nan, 1.0]), "labels hold non-finite"),
    ("C_zero", dict(C=0.0), "C must"), ("C_nan", dict(C=float("nan")), "C must"), ("C_bool", dict(C=True), "C must"),
    ("tol_zero", dict(tol=0.0), "tol must"), ("tol_inf", dict(tol=float("inf")), "tol must"),
    ("max_iter_zero", dict(max_iter=0), "max_iter must"), ("max_iter_float", dict(max_iter=2.5), "max_iter must"),
    ("scale_zero", dict(intercept_scaling=0.0), "intercept_scaling must"), ("scale_neg", dict(intercept_scaling=-1.0, fit_intercept=False), "intercept_scaling must"),
]


@pytest.mark.parametrize("name,over,msg", BAD_FIT, ids=[b[0] for b in BAD_FIT])
def test_fit_argument_checks(name, over, msg):
    kw = dict(K=K_OK, labels=[0, 1, 0, 1])
    kw.update(over)
    with pytest.raises(ValueError, match=msg):
        ksvm.check_kernel_svm_fit_args(**kw)


def test_fit_argument_checks_accept_and_count_labels():
    classes, y = ksvm.check_kernel_svm_fit_args(K_OK, ["b", "a", "b", "c"])
    assert classes.tolist() == ["a", "b", "c"] and y.tolist() == [1, 0, 1, 2] and y.dtype == np.int32
    ksvm.check_kernel_svm_fit_args(K_OK, [0, 1, 0, 1], fit_intercept=False, intercept_scaling=0.0)
    n = 1025
    with pytest.raises(ValueError, match="2 .. 1024 distinct"):
        ksvm.check_kernel_svm_fit_args(torch.zeros(1, dtype=torch.float64).expand(n, n), np.arange(n))
    with pytest.raises(ValueError, match="CUDA float64"):
        ksvm.kernel_svm_fit(K_OK, [0, 1, 0, 1])


def test_kernel_argument_checks():
    assert ksvm.check_columns(None, 9) == (0, 9) and ksvm.check_columns((2, 9), 9) == (2, 9)
    for bad in ((3, 3), (-1, 2), (0, 10), (2.0, 3), (1,), "ab", (True, 2)):
        with pytest.raises(ValueError):
            ksvm.check_columns(bad, 9)
    assert ksvm.check_channels(None, 9) == [(0, 9)] and ksvm.check_channels([(0, 4), (4, 9)], 9) == [(0, 4), (4, 9)]
    for bad in ([], (0, 4), [(0, 4)] * 17, [(4, 2)]):
        with pytest.raises(ValueError):
            ksvm.check_channels(bad, 9)
    assert ksvm.check_scales([0.5, 2], 2) == [0.5, 2.0]
    for bad, k in (([0.5], 2), ([-1.0, 1.0], 2), ([np.nan], 1), ("x", 1)):
        with pytest.raises(ValueError):
            ksvm.check_scales(bad, k)
    for bad in (0.0, -1.0, float("nan"), True, "1"):
        with pytest.raises(ValueError, match="gamma"):
            ksvm.check_gamma(bad)
    assert ksvm.scales_from_means([2.0, 0.5]) == [0.5, 2.0]
    with pytest.raises(ValueError, match="channel 1"):  # A = 0: every row equal on the channel
        ksvm.scales_from_means([2.0, 0.0])
    with pytest.raises(ValueError, match="channel 0"):
        ksvm.scales_from_means([float("nan")])
    x = torch.as_tensor(ko.histograms(6, 4))
    ksvm.check_histograms(x)
    bad = x.clone()
    bad[2, 1] = -1e-9
    with pytest.raises(ValueError, match="negative"):
        ksvm.check_histograms(bad)
    bad[2, 1] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        ksvm.check_histograms(bad)
    for call in (ksvm.chi2_distance, ksvm.linear_gram, ksvm.chi2_kernel):
        with pytest.raises(ValueError, match="CUDA"):
            call(x)
    with pytest.raises(ValueError, match="kernel must be"):
        ksvm.KernelSvm("rbf")


def test_library_limits_without_a_device():
    L = _ffi.lib()
    assert L.va_kernel_svm_fit_workspace_bytes(130, 3) > 0 and L.va_kernel_svm_fit_workspace_bytes(130, 1) > 0
    for n, rows in ((1, 3), (16385, 3), (10, 0), (10, 2), (10, 1025)):
        assert L.va_kernel_svm_fit_workspace_bytes(n, rows) == 0 and "va_kernel_svm_fit" in _ffi.last_error(), (n, rows)
    import ctypes
    off = (ctypes.c_size_t * len(_ffi.KSVM_FIT_FIELDS))()
    total = L.va_kernel_svm_fit_layout(130, 3, off, len(off))
    assert total == L.va_kernel_svm_fit_workspace_bytes(130, 3) and list(off) == sorted(off) and off[0] == 0
    assert L.va_kernel_svm_fit_layout(130, 3, off, len(off) - 1) == 0 and "exactly 21 fields" in _ffi.last_error()
    assert L.va_kernel_svm_fit_layout(130, 3, None, len(off)) == 0
    hdr = open(ksvm.__file__.replace("video_analytics_amd/ksvm.py", "include/va.h")).read()
    assert "#define VA_KSVM_FIT_FIELDS %d\n" % len(_ffi.KSVM_FIT_FIELDS) in hdr and "#define VA_CHI2_MAX_CHANNELS %d\n" % _ffi.CHI2_MAX_CHANNELS in hdr
    for i, name in enumerate(_ffi.KSVM_PHASES):
        assert "#define VA_KSVM_PHASE_%s %d\n" % (name.upper(), i) in hdr
    assert (ksvm.MAX_ROWS, ksvm.MAX_CLASSES, ksvm.MAX_DIM) == (16384, 1024, 65536)


def test_classifier_routes_are_refused_by_name_on_the_host():
    from video_analytics_amd import stip, trajectories
    with pytest.raises(ValueError, match="svm must be 'primal' or 'dual'"):  # refused before anything else is looked at
        trajectories.TrajectoryClassifier().fit([], [], svm="kernel")
    with pytest.raises(ValueError, match="svm must be 'linear' or 'chi2'"):
        stip.StipClassifier().fit([], [], svm="rbf")
    assert trajectories.TrajectoryClassifier.SVM_MAX_DIM == 8192
    assert stip.StipClassifier().kernel_svm is None
