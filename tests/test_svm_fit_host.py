"""The fusion SVM's fit, the parts that need no GPU: the numpy restatement (tests/svm_fit_oracle.py) against the stored
``LinearSVC(tol=1e-12)`` solutions of tests/golden/svm_fit_small.npz, the binary row convention, and every rejection of
``fusion.check_svm_fit_args``."""
import numpy as np
import pytest
import torch

import svm_fit_oracle as so
from video_analytics_amd import combinedModel, fusion
from video_analytics_amd.fusion import check_svm_fit_args, linear_svm_fit


@pytest.fixture(scope="module")
def golden():
    return so.load_golden()


@pytest.fixture(scope="module")
def restated(golden):
    return [so.newton_cg(p["X"], p["labels"]) for p in golden]


def test_golden_file_is_what_the_issue_describes(golden):
    shapes = [(p["X"].shape, len(p["classes"])) for p in golden]
    assert shapes == [((97, 37), 3), ((64, 24), 2), ((40, 64), 4), ((210, 33), 70), ((300, 202), 101), ((257, 129), 5)]
    for p in golden:
        X = p["X"]
        assert p["X_test"].shape == (200, X.shape[1]) and (X >= 0).all()
        assert (X == 0).all(0).any(), "one all-zero column"
        assert np.array_equal(X[0], X[-1]) and p["labels"][0] == p["labels"][-1], "one repeated row"
        assert np.array_equal(np.unique(p["labels"]), p["classes"]), "every class present"
        assert p["coef"].shape == (1 if len(p["classes"]) == 2 else len(p["classes"]), X.shape[1])
    assert golden[0]["classes"].tolist() == [1, 2, 3] and golden[1]["classes"].tolist() == [4, 9]


@pytest.mark.parametrize("i", range(so.N_PROBLEMS))
def test_restatement_agrees_with_sklearn_within_the_strong_convexity_bound(golden, restated, i):
    p = golden[i]
    coef, intercept, classes, steps, _ = restated[i]
    assert np.array_equal(classes, p["classes"]) and coef.shape == p["coef"].shape and steps.max() <= 25
    g_or, g0 = so.model_gradient_norms(coef, intercept, p["X"], p["labels"], classes)
    g_sk, _ = so.model_gradient_norms(p["coef"], p["intercept"], p["X"], p["labels"], p["classes"])
    assert (g_or <= 1e-10 * g0).all() and (g_sk <= 1e-5).all()
    dist = np.linalg.norm(so.pack(coef, intercept) - so.pack(p["coef"], p["intercept"]), axis=1)
    assert (dist <= g_or + g_sk).all(), (dist, g_or + g_sk)
    assert np.array_equal(so.predict(p["X_test"], coef, intercept, classes), so.predict(p["X_test"], p["coef"], p["intercept"], p["classes"]))


def test_oracle_gradient_is_the_derivative_of_its_objective(golden):
    p = golden[0]
    Xa, Y = so.augmented(p["X"]), so.signs(p["labels"], p["classes"])
    rng = np.random.RandomState(0)
    W, V = 0.1 * rng.randn(3, 38), rng.randn(3, 38)
    eps = 1e-6
    num = (so.objective(W + eps * V, Xa, Y) - so.objective(W - eps * V, Xa, Y)) / (2 * eps)
    assert np.allclose(num, (so.gradient(W, Xa, Y) * V).sum(1), rtol=1e-6)


def test_binary_problem_is_one_row_for_the_second_class(golden, restated):
    p = golden[1]
    Y = so.signs(p["labels"], p["classes"])
    assert Y.shape == (1, 64) and np.array_equal(Y[0] > 0, p["labels"] == 9)
    coef, intercept, classes, _, _ = restated[1]
    assert coef.shape == (1, 24) and intercept.shape == (1,) and classes.tolist() == [4, 9]
    train = so.predict(p["X"], coef, intercept, classes)
    assert (train == p["labels"]).mean() > 0.8  # a positive score means classes[1]
    cl, y = check_svm_fit_args(p["X"], p["labels"])
    assert cl.tolist() == [4, 9] and y.dtype == np.int32 and np.array_equal(cl[y], p["labels"])


X_OK = np.abs(np.random.RandomState(1).randn(6, 3))
Y_OK = [0, 1, 2, 0, 1, 2]
BAD_ARGS = [
    ("one_label", dict(labels=[5] * 6), "distinct labels"),
    ("length", dict(labels=[0, 1, 2]), "labels of shape"),
    ("labels_2d", dict(labels=[[0, 1, 2, 0, 1, 2]]), "labels of shape"),
    ("nan", dict(descriptors=np.where(np.eye(6, 3) > 0, np.nan, X_OK)), "non-finite"),
    ("inf", dict(descriptors=np.where(np.eye(6, 3) > 0, np.inf, X_OK)), "non-finite"),
    ("inf_tensor", dict(descriptors=torch.full((6, 3), float("inf"))), "non-finite"),
    ("int_tensor", dict(descriptors=torch.zeros((6, 3), dtype=torch.int32)), "float32 or float64"),
    ("x_1d", dict(descriptors=X_OK[:, 0]), "2-D"),
    ("x_3d", dict(descriptors=X_OK[None]), "2-D"),
    ("one_row", dict(descriptors=X_OK[:1], labels=[0]), "n >= 2"),
    ("no_columns", dict(descriptors=np.zeros((6, 0))), "1 <= d"),
    ("wide", dict(descriptors=np.zeros((6, 8193))), "d <= 8192"),
    ("C_zero", dict(C=0.0), "C must"), ("C_neg", dict(C=-1.0), "C must"), ("C_nan", dict(C=float("nan")), "C must"),
    ("C_inf", dict(C=float("inf")), "C must"), ("C_str", dict(C="1"), "C must"),
    ("tol_zero", dict(tol=0.0), "tol must"), ("tol_nan", dict(tol=float("nan")), "tol must"),
    ("max_iter_zero", dict(max_iter=0), "max_iter"), ("max_iter_float", dict(max_iter=2.5), "max_iter"),
    ("scaling_zero", dict(intercept_scaling=0.0), "intercept_scaling"), ("scaling_neg", dict(intercept_scaling=-1.0, fit_intercept=False), "intercept_scaling"),
    ("scaling_inf", dict(intercept_scaling=float("inf")), "intercept_scaling"),
]


@pytest.mark.parametrize("name,over,msg", BAD_ARGS, ids=[b[0] for b in BAD_ARGS])
def test_check_svm_fit_args_rejects(name, over, msg):
    kw = dict(descriptors=X_OK, labels=Y_OK)
    kw.update(over)
    with pytest.raises(ValueError, match=msg):
        check_svm_fit_args(**kw)
    with pytest.raises(ValueError, match=msg):  # the public call checks before it looks for a GPU
        linear_svm_fit(**kw)


def test_check_svm_fit_args_accepts_and_maps_labels():
    classes, y = check_svm_fit_args(X_OK, ["b", "a", "c", "b", "a", "c"])
    assert classes.tolist() == ["a", "b", "c"] and y.tolist() == [1, 0, 2, 1, 0, 2]
    classes, y = check_svm_fit_args(torch.as_tensor(X_OK, dtype=torch.float32), torch.tensor(Y_OK), C=10, tol=1e-3, max_iter=1,
                                    fit_intercept=False, intercept_scaling=0.0)
    assert classes.tolist() == [0, 1, 2] and y.tolist() == Y_OK


def test_fit_without_a_gpu_raises_after_the_argument_check():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no GPU visible; the hot path has no CPU fallback"):
        linear_svm_fit(X_OK, Y_OK)
    with pytest.raises(RuntimeError, match="no GPU visible"):
        combinedModel.linearSvmFit(X_OK, Y_OK, C=2.0)
    with pytest.raises(ValueError, match="distinct labels"):
        combinedModel.linearSvmFit(X_OK, [1] * 6)


def test_workspace_query_needs_no_gpu_and_rejects_bad_sizes():
    from video_analytics_amd import _ffi
    L = _ffi.lib()
    assert L.va_linear_svm_fit_workspace_bytes(9537, 512, 101) > 9537 * 101 * 8 * 3
    assert L.va_linear_svm_fit_workspace_bytes(2, 1, 1) > 0
    for bad in ((1, 8, 3), (10, 0, 3), (10, 8193, 3), (10, 8, 0), (10, 8, 2), (10, 8, 4097)):
        assert L.va_linear_svm_fit_workspace_bytes(*bad) == 0, bad
        assert b"va_linear_svm_fit: need n >= 2" in L.va_last_error()


def test_main_keeps_the_reference_fit_by_default():
    import inspect
    assert inspect.signature(combinedModel.main).parameters["fit"].default == "sklearn"
    with pytest.raises(ValueError, match="fit must be"):
        combinedModel.main(fit="liblinear")
