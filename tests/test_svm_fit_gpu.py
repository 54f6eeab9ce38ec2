"""The fusion SVM fitted on the device (``va_linear_svm_fit``) on the six problems of
tests/golden/svm_fit_small.npz, checked by the numpy restatement of the problem (tests/svm_fit_oracle.py) and against the
stored ``LinearSVC(tol=1e-12)`` solutions.  The one tolerance between two solutions is the bound 1-strong convexity gives:
``|w_a - w_b| <= |grad f(w_a)| + |grad f(w_b)|``."""
import ctypes
import sys
import warnings

import numpy as np
import pytest
import torch

import svm_fit_oracle as so
from video_analytics_amd import _ffi, combinedModel, fusion

pytestmark = pytest.mark.gpu

TOL = 1e-8


@pytest.fixture(scope="module")
def golden():
    return so.load_golden()


@pytest.fixture(scope="module")
def fits(golden):
    """Every golden problem fitted once: (coef, intercept, classes, info)."""
    return [fusion.linear_svm_fit(p["X"], p["labels"], tol=TOL, return_info=True) for p in golden]


def check_optimal(coef, intercept, X, labels, classes, **kw):
    g, g0 = so.model_gradient_norms(coef, intercept, X, labels, classes, **kw)
    print("max |g| / |g0| = %.3g" % (g / g0).max())
    assert (g <= 2 * TOL * g0).all(), (g / g0).max()
    return g


def check_against(coef, intercept, ref_coef, ref_intercept, X, labels, classes, **kw):
    g, _ = so.model_gradient_norms(coef, intercept, X, labels, classes, **kw)
    g_ref, _ = so.model_gradient_norms(ref_coef, ref_intercept, X, labels, classes, **kw)
    s = kw.get("intercept_scaling", 1.0)
    dist = np.linalg.norm(so.pack(coef, intercept, s) - so.pack(ref_coef, ref_intercept, s), axis=1)
    print("max distance / bound = %.3g" % (dist / (g + g_ref)).max())
    assert (dist <= g + g_ref).all(), (dist, g + g_ref)


@pytest.mark.parametrize("i", range(so.N_PROBLEMS))
def test_fit_is_optimal_by_the_independent_gradient(golden, fits, i):
    p, (coef, intercept, classes, info) = golden[i], fits[i]
    rows = 1 if len(p["classes"]) == 2 else len(p["classes"])
    assert coef.shape == (rows, p["X"].shape[1]) and coef.dtype == np.float64 and intercept.shape == (rows,)
    assert np.array_equal(classes, p["classes"])
    print("problem %d: n_iter %d" % (i + 1, info["n_iter"]))
    check_optimal(coef, intercept, p["X"], p["labels"], classes)
    assert info["converged"] is True and info["n_iter"] <= 100 and (info["rel_grad"] <= TOL).all()
    assert info["n_iter"] == info["steps"].max() and (info["steps"] >= 1).all() and (info["cg_steps"] >= info["steps"]).all()
    W = so.pack(coef, intercept)
    f = so.objective(W, so.augmented(p["X"]), so.signs(p["labels"], classes))
    assert np.allclose(info["objective"], f, rtol=1e-12, atol=0)


@pytest.mark.parametrize("i", range(so.N_PROBLEMS))
def test_fit_agrees_with_sklearn_within_the_strong_convexity_bound(golden, fits, i):
    p, (coef, intercept, classes, _) = golden[i], fits[i]
    check_against(coef, intercept, p["coef"], p["intercept"], p["X"], p["labels"], classes)


@pytest.mark.parametrize("i", range(so.N_PROBLEMS))
def test_held_out_predictions_equal_sklearns(golden, fits, i):
    p, (coef, intercept, classes, _) = golden[i], fits[i]
    ours = fusion.linear_svm_predict(p["X_test"], coef, intercept, classes)
    theirs = fusion.linear_svm_predict(p["X_test"], p["coef"], p["intercept"], p["classes"])
    assert ours.shape == (200,) and np.array_equal(ours, theirs)
    assert np.array_equal(theirs, so.predict(p["X_test"], p["coef"], p["intercept"], p["classes"]))


def test_two_fits_and_chunked_fits_give_the_same_bits(golden, fits, monkeypatch):
    p, (coef, intercept, _, info) = golden[4], fits[4]
    for chunk in (fusion.SVM_FIT_NEWTON_CHUNK, 1, 32):  # again; one Newton step per call; every step in one call
        monkeypatch.setattr(fusion, "SVM_FIT_NEWTON_CHUNK", chunk)
        c2, b2, _, info2 = fusion.linear_svm_fit(p["X"], p["labels"], tol=TOL, return_info=True)
        assert np.array_equal(c2, coef) and np.array_equal(b2, intercept), chunk
        assert np.array_equal(info2["objective"], info["objective"]) and np.array_equal(info2["steps"], info["steps"])
    assert info["n_iter"] <= 32


class Raw(object):
    """The C entry points called directly: device buffers for one problem, one call per ``step()``."""

    def __init__(self, X, y, n_classes, C=1.0, scale=1.0, tol=TOL):
        self.L = _ffi.lib()
        self.n, self.d = X.shape
        self.n_classes, self.rows = n_classes, 1 if n_classes == 2 else n_classes
        self.scalars = dict(C=C, scale=scale, tol=tol)
        self.x = torch.as_tensor(np.ascontiguousarray(X, dtype=np.float64)).cuda()
        self.y = torch.as_tensor(np.ascontiguousarray(y, dtype=np.int32)).cuda()
        self.need = self.L.va_linear_svm_fit_workspace_bytes(self.n, self.d, self.rows)
        assert self.need > 0
        self.work = torch.empty((self.need // 8,), dtype=torch.float64, device="cuda")
        self.coef = torch.zeros((self.rows, self.d), dtype=torch.float64, device="cuda")
        self.intercept = torch.zeros((self.rows,), dtype=torch.float64, device="cuda")
        self.stats = torch.zeros((self.rows, 4), dtype=torch.float64, device="cuda")

    def call(self, newton_iters, restart, **over):
        a = dict(self.scalars, n=self.n, d=self.d, n_classes=self.n_classes, need=self.need, x=_ffi.ptr(self.x), y=_ffi.ptr(self.y),
                 coef=_ffi.ptr(self.coef), work=_ffi.ptr(self.work))
        a.update(over)
        return self.L.va_linear_svm_fit(_ffi.ctx(0), a["x"], a["y"], a["n"], a["d"], a["n_classes"], a["C"], a["scale"], a["tol"],
                                        newton_iters, restart, a["coef"], _ffi.ptr(self.intercept), _ffi.ptr(self.stats), a["work"],
                                        a["need"], _ffi.stream_ptr(self.x))


def test_early_converging_class_is_frozen_while_the_others_go_on(golden):
    p = golden[3]
    X = p["X"].copy()
    X[p["labels"] == 0] += 10.0  # class 0 moved far out: trivially separable
    classes, y = fusion.check_svm_fit_args(X, p["labels"])
    raw = Raw(X, y, len(classes))
    steps, coefs = [], []
    for call in range(40):
        assert raw.call(1, 1 if call == 0 else 0) == _ffi.VA_OK
        st = raw.stats.cpu().numpy()
        steps.append(st[:, 3].copy())
        coefs.append(raw.coef[0].cpu().numpy())
        if (st[:, 1] <= TOL * st[:, 2]).all():
            break
    steps = np.array(steps)
    print("Newton steps per class row:", steps[-1].astype(int).tolist())
    assert (st[:, 1] <= TOL * st[:, 2]).all() and steps[-1].max() <= 25
    assert steps[-1, 0] < steps[-1, 1:].max(), "class 0 converges in fewer steps than the slowest of the rest"
    k = int(steps[-1, 0])  # the call (1-based) that took class 0's last step
    assert (steps[k - 1:, 0] == k).all() and len(steps) > k
    assert (np.diff(steps[k - 1:, 1:].max(axis=1)) > 0).all(), "the others go on"
    assert all(np.array_equal(c, coefs[k - 1]) for c in coefs[k:]), "a stopped class keeps its bits"
    coef, intercept = raw.coef.cpu().numpy(), raw.intercept.cpu().numpy()
    check_optimal(coef, intercept, X, p["labels"], classes)
    ref = so.newton_cg(X, p["labels"], tol=1e-10)
    check_against(coef, intercept, ref[0], ref[1], X, p["labels"], classes)
    # the public call enqueues the same operations
    c2, b2, _ = fusion.linear_svm_fit(X, p["labels"], tol=TOL)
    assert np.array_equal(c2, coef) and np.array_equal(b2, intercept)


def test_fit_without_an_intercept(golden):
    p = golden[0]
    coef, intercept, classes, info = fusion.linear_svm_fit(p["X"], p["labels"], tol=TOL, fit_intercept=False, return_info=True)
    assert info["converged"] and np.array_equal(intercept, np.zeros(3))
    check_optimal(coef, intercept, p["X"], p["labels"], classes, intercept_scaling=0.0)
    ref = so.newton_cg(p["X"], p["labels"], tol=1e-10, intercept_scaling=0.0)
    assert np.array_equal(ref[1], np.zeros(3))
    check_against(coef, intercept, ref[0], ref[1], p["X"], p["labels"], classes, intercept_scaling=0.0)


@pytest.mark.parametrize("kw", [dict(C=0.01), dict(C=10.0), dict(intercept_scaling=2.5)], ids=["C=0.01", "C=10", "intercept_scaling=2.5"])
def test_fit_with_other_C_and_intercept_scaling(golden, kw):
    p = golden[0]
    coef, intercept, classes, info = fusion.linear_svm_fit(p["X"], p["labels"], tol=TOL, return_info=True, **kw)
    assert info["converged"] and info["n_iter"] <= 100
    check_optimal(coef, intercept, p["X"], p["labels"], classes, **kw)
    ref = so.newton_cg(p["X"], p["labels"], tol=1e-10, **kw)
    check_against(coef, intercept, ref[0], ref[1], p["X"], p["labels"], classes, **kw)


def test_float32_device_tensor_gives_the_bits_of_float64_input(golden, fits):
    p, (coef, intercept, classes, _) = golden[0], fits[0]
    x32 = torch.as_tensor(p["X"].astype(np.float32)).cuda()
    assert np.array_equal(x32.cpu().numpy().astype(np.float64), p["X"])
    for x in (x32, x32.double(), x32.cpu()):
        c2, b2, cl2 = combinedModel.linearSvmFit(x, torch.as_tensor(p["labels"]), tol=TOL)
        assert np.array_equal(c2, coef) and np.array_equal(b2, intercept) and np.array_equal(cl2, classes)


def test_max_iter_reached_warns_and_returns_the_iterate(golden):
    p = golden[0]
    with pytest.warns(RuntimeWarning, match="not converged"):
        coef, intercept, classes, info = fusion.linear_svm_fit(p["X"], p["labels"], tol=TOL, max_iter=1, return_info=True)
    assert info["converged"] is False and info["n_iter"] == 1 and (info["rel_grad"] > TOL).any()
    assert np.isfinite(coef).all() and np.abs(coef).max() > 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fusion.linear_svm_fit(p["X"], p["labels"], tol=TOL)  # the default max_iter is enough: no warning


def test_c_entry_points_reject_bad_arguments_before_any_launch(golden):
    p = golden[0]
    classes, y = fusion.check_svm_fit_args(p["X"], p["labels"])
    raw = Raw(p["X"], y, len(classes))
    L, nan, inf = raw.L, float("nan"), float("inf")
    null = ctypes.c_void_p(0)
    bad = [(dict(C=0.0), "C must"), (dict(C=-1.0), "C must"), (dict(C=nan), "C must"), (dict(C=inf), "C must"),
           (dict(tol=0.0), "tol must"), (dict(tol=nan), "tol must"), (dict(tol=inf), "tol must"),
           (dict(scale=-1.0), "intercept_scaling must"), (dict(scale=nan), "intercept_scaling must"), (dict(scale=inf), "intercept_scaling must"),
           (dict(n=1), "n >= 2"), (dict(d=0), "1 <= dim"), (dict(d=8193), "1 <= dim"), (dict(n_classes=1), "n_classes"),
           (dict(n_classes=4097), "n_classes"), (dict(x=null), "NULL pointer"), (dict(y=null), "NULL pointer"),
           (dict(coef=null), "NULL pointer"), (dict(work=null), "NULL pointer")]
    for over, msg in bad:
        assert raw.call(1, 1, **over) == _ffi.VA_ERR_INVALID, over
        assert msg in L.va_last_error().decode(), (over, L.va_last_error())
    for iters, restart, msg in ((-1, 1, "newton_iters"), (1001, 1, "newton_iters"), (1, 2, "restart"), (1, -1, "restart")):
        assert raw.call(iters, restart) == _ffi.VA_ERR_INVALID
        assert msg in L.va_last_error().decode()
    assert L.va_linear_svm_fit(None, _ffi.ptr(raw.x), _ffi.ptr(raw.y), raw.n, raw.d, 3, 1.0, 1.0, TOL, 1, 1, _ffi.ptr(raw.coef),
                               _ffi.ptr(raw.intercept), _ffi.ptr(raw.stats), _ffi.ptr(raw.work), raw.need, None) == _ffi.VA_ERR_INVALID
    assert b"ctx is NULL" in L.va_last_error()
    # a workspace one byte short: the library's code for that, and the size it wants in the message
    assert raw.call(1, 1, need=raw.need - 1) == _ffi.VA_ERR_WORKSPACE
    assert str(raw.need) in L.va_last_error().decode()
    with pytest.raises(ValueError, match="workspace"):
        _ffi.check(_ffi.VA_ERR_WORKSPACE)
    for sizes in ((1, 8, 3), (10, 0, 3), (10, 8193, 3), (10, 8, 0), (10, 8, 2), (10, 8, 4097)):
        assert L.va_linear_svm_fit_workspace_bytes(*sizes) == 0 and b"need n >= 2" in L.va_last_error()
    cg = torch.zeros((raw.rows,), dtype=torch.float64, device="cuda")
    for (n, d, rows, work, need, out), code, msg in (((1, raw.d, 3, raw.work, raw.need, cg), _ffi.VA_ERR_INVALID, "need n >= 2"),
                                                     ((raw.n, raw.d, 2, raw.work, raw.need, cg), _ffi.VA_ERR_INVALID, "n_class_rows"),
                                                     ((raw.n, raw.d, 3, None, raw.need, cg), _ffi.VA_ERR_INVALID, "NULL pointer"),
                                                     ((raw.n, raw.d, 3, raw.work, raw.need, None), _ffi.VA_ERR_INVALID, "NULL pointer"),
                                                     ((raw.n, raw.d, 3, raw.work, raw.need - 1, cg), _ffi.VA_ERR_WORKSPACE, str(raw.need))):
        assert L.va_linear_svm_fit_cg_steps(_ffi.ctx(0), n, d, rows, _ffi.ptr(work), need, _ffi.ptr(out), None) == code
        assert msg in L.va_last_error().decode()
    torch.cuda.synchronize()
    assert torch.count_nonzero(raw.coef).item() == 0 and torch.count_nonzero(raw.stats).item() == 0  # nothing ran
    assert raw.call(0, 1) == _ffi.VA_OK  # and the same buffers are fine with good arguments: W = 0, |g| = |g(0)|
    st = raw.stats.cpu().numpy()
    g0 = so.model_gradient_norms(np.zeros((3, raw.d)), np.zeros(3), p["X"], p["labels"], classes)[1]
    assert np.allclose(st[:, 1], g0, rtol=1e-13) and np.array_equal(st[:, 1], st[:, 2]) and (st[:, 3] == 0).all()
    assert np.allclose(st[:, 0], raw.n, rtol=1e-13)  # f(0) = C n


def test_main_fits_on_the_device_without_sklearn(tmp_path, monkeypatch, capsys):
    import joblib
    from video_analytics_amd import parameters
    D = parameters.VIDEO_DESCRIPTOR_DIM
    rng = np.random.RandomState(5)
    mu = rng.randn(2, 3, D)
    paths = {}
    for split, n in (("TRAIN", 36), ("TEST", 12)):
        lab = np.arange(n) % 3 + 1
        for s, stream in enumerate(("SPATIAL", "TEMPORAL")):
            x = np.maximum(0.0, mu[s][lab - 1] + 0.5 * rng.randn(n, D))
            path = tmp_path / ("%s_%s.csv" % (stream, split))
            with open(path, "w") as f:
                for i in range(n):
                    f.write("v_%s_%03d,%d,%s\n" % (split, i, lab[i], ",".join(repr(float(v)) for v in x[i])))
            monkeypatch.setattr(parameters, "%s_%s_CSV_LOC" % (stream, split), str(path))
    monkeypatch.setattr(parameters, "SVM_FILE", str(tmp_path / "svm.pkl"))
    monkeypatch.setitem(sys.modules, "sklearn", None)  # any ``import sklearn`` now raises ImportError
    combinedModel.main(fit="device")
    out = capsys.readouterr().out
    assert out.startswith("accuracy = ") and out.strip().endswith("percent") and float(out.split()[2]) == 100.0
    model = joblib.load(str(tmp_path / "svm.pkl"))
    assert sorted(model) == ["classes_", "coef_", "intercept_"]
    assert model["coef_"].shape == (3, 2 * D) and model["intercept_"].shape == (3,) and model["classes_"].tolist() == [1, 2, 3]
    trainX, trainY = combinedModel.combineDescriptors(parameters.SPATIAL_TRAIN_CSV_LOC, parameters.TEMPORAL_TRAIN_CSV_LOC)
    check_optimal(model["coef_"], model["intercept_"], trainX, trainY, model["classes_"])
