"""Kernel SVMs on the device (``video_analytics_amd.ksvm``) against the numpy restatement of
tests/ksvm_oracle.py: the chi-square distance bit for bit, the linear Gram matrix, the mean and the exponential at 16 x the
restatement's own deviation from a long-double witness, and the fit through the one tolerance strong convexity gives,
``|alpha - alpha*| <= 2C |pg(alpha)|``, with pg computed here in numpy float64 on the device's own Gram matrix."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import ksvm_oracle as ko
import svm_fit_oracle as so
from video_analytics_amd import _ffi, fusion, ksvm

pytestmark = pytest.mark.gpu

TOL = 1e-8
SIZES = (2, 63, 64, 65, 130)        # ragged last tile, exactly one tile, three tiles
DIMS = (1, 3, 16, 17, 67, 300)
DTYPES = (np.float32, np.float64)
LD = np.longdouble


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def cpu(t):
    return t.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- the chi-square distance: bit for bit ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("d", DIMS)
def test_chi2_distance_equals_the_written_order_bit_for_bit(d, dtype):
    for n in SIZES:
        x = ko.histograms(n, d, seed=n + d).astype(dtype)
        assert (n * d < 100 or (x == 0).mean() > 0.2) and np.array_equal(x[0], x[-1]) and (d == 1 or not x[:, d // 2].any())
        want = ko.chi2_distance(x)
        got = cpu(ksvm.chi2_distance(dev(x)))
        assert got.dtype == np.float64 and same_bits(got, want), (n, d, np.abs(got - want).max())
        assert same_bits(got, got.T.copy()) and not got.diagonal().any() and not np.signbit(got.diagonal()).any()
        assert same_bits(got, cpu(ksvm.chi2_distance(dev(x), dev(x.copy()))))  # the rectangular call on (x, x)
        assert same_bits(got, cpu(ksvm.chi2_distance(dev(x))))                 # two calls
        assert got[0, -1] == 0.0                                               # the two identical rows
    x, y = ko.histograms(130, d, seed=1).astype(dtype), ko.histograms(67, d, seed=2).astype(dtype)
    want = ko.chi2_distance(x, y)
    assert same_bits(cpu(ksvm.chi2_distance(dev(x), dev(y))), want)
    assert same_bits(cpu(ksvm.chi2_distance(dev(y), dev(x))), want.T.copy())


@pytest.mark.parametrize("chunk", (1, 5, 16, 31, 32))
def test_chi2_distance_has_the_same_bits_for_every_staging_length(chunk):
    x, y = ko.histograms(130, 67, seed=3), ko.histograms(67, 67, seed=4).astype(np.float32)
    assert same_bits(cpu(ksvm.chi2_distance(dev(x), chunk=chunk)), ko.chi2_distance(x))
    assert same_bits(cpu(ksvm.chi2_distance(dev(x.astype(np.float32)), dev(y), (16, 67), chunk=chunk)),
                     ko.chi2_distance(x.astype(np.float32), y, (16, 67)))


def test_chi2_channels_are_column_ranges():
    x = ko.histograms(130, 67, seed=5)
    chans = [(0, 16), (16, 67)]
    parts = [ksvm.chi2_distance(dev(x), columns=ch) for ch in chans]
    for ch, D in zip(chans, parts):
        assert same_bits(cpu(D), ko.chi2_distance(x, None, ch))
    K, scales = ksvm.chi2_kernel(dev(x), channels=chans)
    means = [float(ksvm.upper_mean(D).item()) for D in parts]
    assert np.array_equal(scales, [1.0 / a for a in means])
    assert same_bits(cpu(K), cpu(ksvm.combine(parts, scales)))
    K2, s2 = ksvm.chi2_kernel(dev(x[:40]), dev(x), channels=chans, scales=scales)  # test rows against the training rows
    assert same_bits(cpu(K2), cpu(K)[:40]) and np.array_equal(s2, scales)


def test_chi2_kernel_refusals_on_device_data():
    x = ko.histograms(10, 8, seed=6)
    bad = x.copy()
    bad[3, 2] = -0.5
    with pytest.raises(ValueError, match="negative"):
        ksvm.chi2_kernel(dev(bad))
    bad[3, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        ksvm.chi2_kernel(dev(bad))
    same = np.tile(x[:1], (5, 1))
    same[:, 4:] = ko.histograms(5, 4, seed=7) + 0.1
    with pytest.raises(ValueError, match="channel 0"):
        ksvm.chi2_kernel(dev(same), channels=[(0, 4), (4, 8)])
    with pytest.raises(ValueError, match="scales"):
        ksvm.chi2_kernel(dev(x), dev(x))
    with pytest.raises(ValueError, match="CUDA"):
        ksvm.chi2_distance(torch.as_tensor(x))
    with pytest.raises(ValueError, match="chunk"):
        ksvm.chi2_distance(dev(x), chunk=33)
    with pytest.raises(ValueError, match="start < stop"):
        ksvm.chi2_distance(dev(x), columns=(4, 4))


# ---- linear Gram, mean, exponential: 16 x the restatement's own deviation from long double ---------------------------------------

def within_16x(name, kern, rest):
    print("FIGURE %-12s kernel %.3e restatement %.3e" % (name, kern, rest))
    assert kern <= 16.0 * rest, (name, kern, rest)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_linear_gram_within_16x_of_the_restatement(dtype):
    kern = rest = 0.0
    for d in DIMS:
        for m, n in [(s, None) for s in SIZES] + [(130, 67)]:
            rng = np.random.RandomState(m + d)
            x = rng.randn(m, d).astype(dtype)
            y = None if n is None else rng.randn(n, d).astype(dtype)
            got = cpu(ksvm.linear_gram(dev(x), None if y is None else dev(y)))
            if y is None:
                assert same_bits(got, got.T.copy())
                assert same_bits(got, cpu(ksvm.linear_gram(dev(x), dev(x.copy())))) and same_bits(got, cpu(ksvm.linear_gram(dev(x))))
            want = ko.linear_gram_witness(x, y)
            scale = np.maximum(ko.linear_gram_witness(np.abs(x), None if y is None else np.abs(y)), LD(1e-300))
            kern = max(kern, float(np.max(np.abs(got.astype(LD) - want) / scale)))
            rest = max(rest, float(np.max(np.abs(ko.linear_gram(x, y).astype(LD) - want) / scale)))
    within_16x("linear_gram", kern, rest)


def test_linear_gram_operands_are_not_swapped():
    """An asymmetric pair: rows of x times rows of y, never the transpose."""
    x = np.arange(65 * 3, dtype=np.float64).reshape(65, 3)
    y = (np.arange(17 * 3, dtype=np.float64).reshape(17, 3) % 7) - 3.0
    assert np.array_equal(cpu(ksvm.linear_gram(dev(x), dev(y))), x @ y.T)  # small integers: exact


def test_upper_mean_within_16x_of_the_restatement():
    kern = rest = 0.0
    for n in SIZES + (300,):
        D = ko.chi2_distance(ko.histograms(n + 1, 17, seed=n)[:n])  # without the duplicated last row: n = 2 has a mean > 0
        want = ko.upper_mean_witness(D)
        got = ksvm.upper_mean(dev(D))
        assert same_bits(cpu(got), cpu(ksvm.upper_mean(dev(D))))
        kern = max(kern, float(abs(LD(got.item()) - want) / want))
        rest = max(rest, float(abs(LD(ko.upper_mean(D)) - want) / want))
    within_16x("upper_mean", kern, max(rest, float(np.finfo(np.float64).eps) / 2))  # one rounding of the result at the least


def test_exponential_combine_within_16x_of_numpy_exp():
    """The argument is restated bit for bit, so what is measured is the device's exp against numpy's (DESIGN.md S106 records
    the figure an MI355X gave)."""
    x = ko.histograms(130, 67, seed=8)
    chans = [(0, 16), (16, 67)]
    dists = [ko.chi2_distance(x, None, ch) for ch in chans]
    scales = [1.0 / ko.upper_mean(D) for D in dists]
    got = cpu(ksvm.combine([dev(D) for D in dists], scales))
    arg = ko.combine_argument(dists, scales)
    want = np.exp(-arg.astype(LD))
    kern = float(np.max(np.abs(got.astype(LD) - want) / want))
    rest = float(np.max(np.abs(np.exp(-arg).astype(LD) - want) / want))
    within_16x("exp", kern, rest)
    assert same_bits(got, got.T.copy()) and (got.diagonal() == 1.0).all()
    K, _ = ksvm.chi2_kernel(dev(x), channels=chans)
    assert same_bits(cpu(K), got) and same_bits(cpu(K), cpu(ksvm.chi2_kernel(dev(x), channels=chans)[0]))
    sk = pytest.importorskip("sklearn.metrics.pairwise")
    assert np.allclose(cpu(ksvm.chi2_kernel(dev(x), gamma=0.7)[0]), sk.chi2_kernel(x, gamma=0.7), rtol=1e-12, atol=0)


# ---- the fit ---------------------------------------------------------------------------------------------------------------------

_fits = {}


def fitted(name):
    """Every problem fitted once on the device's own Gram matrix, with the witness and the restatement on the same matrix."""
    if name not in _fits:
        X, labels, C, s, kernel = ko.solver_problem(name)
        Kd = ksvm.linear_gram(dev(X)) if kernel == "linear" else ksvm.chi2_kernel(dev(X))[0]
        K = cpu(Kd)
        kw = dict(C=C, tol=TOL, fit_intercept=s > 0, intercept_scaling=s if s > 0 else 1.0)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)  # a row that does not converge fails the test
            dual_coef, intercept, classes, info = ksvm.kernel_svm_fit(Kd, labels, return_info=True, **kw)
            again = ksvm.kernel_svm_fit(Kd, labels, **kw)
        Y = so.signs(labels, classes)
        _fits[name] = dict(X=X, labels=labels, C=C, s=s, K=K, Kd=Kd, Y=Y, beta=cpu(dual_coef), intercept=intercept, classes=classes,
                           info=info, again=(cpu(again[0]), again[1]), witness=ko.nnls_witness(K, Y, C, s),
                           restated=ko.dual_fit(K, labels, C, TOL, 100, s))
    return _fits[name]


@pytest.mark.parametrize("name", ko.PROBLEMS)
def test_fit_meets_the_stop_rule_and_the_witness(name):
    f = fitted(name)
    beta, Y, K, C, s, info = f["beta"], f["Y"], f["K"], f["C"], f["s"], f["info"]
    rows, n = Y.shape
    assert beta.shape == (rows, n) and beta.dtype == np.float64 and np.array_equal(f["classes"], np.unique(f["labels"]))
    alpha = Y * beta
    assert (alpha >= 0.0).all()                                            # feasible exactly
    pg = ko.pg_norms(beta, K, Y, C, s)
    pgw = ko.pg_norms(f["witness"], K, Y, C, s)
    zeros = (beta == 0.0).mean()
    print("%s: outer steps %d..%d, CG steps <= %d, max |pg| / (tol sqrt n) %.3g, zeros %.0f %%, witness |pg| %.2g"
          % (name, info["steps"].min(), info["steps"].max(), info["cg_steps"].max(), (pg / (TOL * np.sqrt(n))).max(), 100 * zeros, pgw.max()))
    assert (pg <= TOL * np.sqrt(n)).all(), (pg / (TOL * np.sqrt(n))).max()  # the stop rule, recomputed independently
    dist = np.linalg.norm(beta - f["witness"], axis=1)
    assert (dist <= 2.0 * C * (pg + pgw)).all(), (dist / (2.0 * C * (pg + pgw))).max()
    assert np.allclose(f["intercept"], s * s * beta.sum(1), rtol=1e-13, atol=0) and (s > 0 or not f["intercept"].any())
    assert info["converged"] is True and info["n_iter"] <= 100 and (info["rel_pg"] <= TOL).all()
    assert np.array_equal(info["n_sv"], (beta != 0.0).sum(1))
    if name != "tiny_C":
        assert ((beta == 0.0).sum(1) > 0).all()                           # zeros in every row: the face matters
    else:
        assert (alpha > 0.0).all()                                         # every point is a support vector
    # the restatement of the same method on the same matrix: it stops too, and lands within the bound
    rb, rint, _, rinfo = f["restated"]
    assert rinfo["converged"] and np.array_equal(rinfo["stopped"], np.ones(rows, dtype=bool))
    rpg = ko.pg_norms(rb, K, Y, C, s)
    assert (np.linalg.norm(beta - rb, axis=1) <= 2.0 * C * (pg + rpg)).all()
    print("%s: restatement outer steps %d..%d (device %d..%d)" % (name, rinfo["steps"].min(), rinfo["steps"].max(), info["steps"].min(),
                                                                  info["steps"].max()))
    # Step counts: both sides run the same method on the same matrix, but their products round differently, and a last-bit
    # difference can flip a discrete decision (the end of a CG, an accepted step length), after which that row's path differs.
    # A row's own count is therefore no property of the method: the restatement alone moves single rows by one or two steps
    # when K is perturbed by one part in 10^16 (and its products depend on the host's BLAS), while its count summed over the
    # rows moves by 0.2 % (640 against 639 on the 65-class problem).  So the sums are held to each other within a factor of
    # two, outer steps and CG steps alike: a guard against a regression of the method, not a tolerance on a result.
    for key in ("steps", "cg_steps"):
        ds, rs = int(info[key].sum()), int(rinfo[key].sum())
        print("%s: %s summed over the rows: device %d, restatement %d" % (name, key, ds, rs))
        assert ds <= 2 * rs + 2 * rows and rs <= 2 * ds + 2 * rows, (key, ds, rs)
    # two calls: the same bits
    assert same_bits(f["again"][0], beta) and same_bits(f["again"][1], f["intercept"])


def test_rows_finish_at_different_outer_steps_and_stay_frozen():
    """65 class rows: the 64-row tile and the single row of the second tile stop at different steps, so finished tiles are
    skipped while others go on; a finished row's coefficients never change again."""
    f = fitted("sixty_five_classes")
    steps = f["info"]["steps"]
    assert steps.max() - steps.min() >= 2, steps
    Kd, labels = f["Kd"], f["labels"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        early = ksvm.kernel_svm_fit(Kd, labels, C=f["C"], tol=TOL, max_iter=int(steps.min()) + 1, return_info=True)
    done = early[3]["rel_pg"] <= TOL
    assert done.any() and not done.all()
    assert same_bits(cpu(early[0])[done], f["beta"][done])


@pytest.mark.parametrize("name", ("three_classes", "two_classes", "wide", "no_intercept"))
def test_linear_kernel_gives_the_primal_solver_s_model(name):
    """W = beta [X, s] against fusion.linear_svm_fit within |grad f(W)| + |grad f(W_primal)|."""
    f = fitted(name)
    X, labels, C, s = f["X"], f["labels"], f["C"], f["s"]
    kw = dict(C=C, intercept_scaling=s if s > 0 else 1.0)
    coef, intercept, classes = fusion.linear_svm_fit(X, labels, tol=TOL, fit_intercept=s > 0, **kw)
    W = ko.primal_weights(f["beta"], X, s)
    Wp = so.pack(coef, intercept, s)
    Xa, Y = so.augmented(X, s), f["Y"]
    g = np.linalg.norm(so.gradient(W, Xa, Y, C), axis=1)
    gp = np.linalg.norm(so.gradient(Wp, Xa, Y, C), axis=1)
    dist = np.linalg.norm(W - Wp, axis=1)
    print("%s: max distance / bound %.3g" % (name, (dist / (g + gp)).max()))
    assert (dist <= g + gp).all(), (dist / (g + gp)).max()


@pytest.mark.parametrize("i", range(so.N_PROBLEMS))
def test_linear_kernel_on_the_golden_problems(i):
    p = so.load_golden()[i]
    X, labels = p["X"], p["labels"]
    dual_coef, intercept, classes = ksvm.kernel_svm_fit(ksvm.linear_gram(dev(X)), labels, tol=TOL)
    assert np.array_equal(classes, p["classes"])
    W = ko.primal_weights(cpu(dual_coef), X)
    Xa, Y = so.augmented(X), so.signs(labels, classes)
    g = np.linalg.norm(so.gradient(W, Xa, Y), axis=1)
    for ref in (so.pack(p["coef"], p["intercept"]), so.pack(*fusion.linear_svm_fit(X, labels, tol=TOL)[:2])):  # sklearn's, the primal fit's
        gr = np.linalg.norm(so.gradient(ref, Xa, Y), axis=1)
        assert (np.linalg.norm(W - ref, axis=1) <= g + gr).all()
    model = ksvm.KernelSvm("linear").fit(dev(X), labels)
    assert np.array_equal(model.coef, cpu(dual_coef @ dev(X))) and same_bits(model.intercept, intercept)
    assert np.array_equal(model.predict(dev(p["X_test"])), so.predict(p["X_test"], model.coef, model.intercept, classes))


def test_kernel_svm_predict_is_linear_svm_predict_on_the_test_kernel():
    f = fitted("three_classes")
    rng = np.random.RandomState(0)
    Xt = f["X"][rng.permutation(130)[:40]] + 0.1 * rng.randn(40, 17)
    Kt = ksvm.linear_gram(dev(Xt), dev(f["X"]))
    pred, scores = ksvm.kernel_svm_predict(Kt, dev(f["beta"]), f["intercept"], f["classes"], return_scores=True)
    want_pred, want = fusion.linear_svm_predict(cpu(Kt), f["beta"], f["intercept"], f["classes"], return_scores=True)
    assert same_bits(scores, want) and np.array_equal(pred, want_pred)
    assert np.allclose(scores, cpu(Kt) @ f["beta"].T + f["intercept"], rtol=1e-10, atol=1e-10)
    two = fitted("two_classes")
    Kt2 = ksvm.linear_gram(dev(two["X"][:9]), dev(two["X"]))
    p2, s2 = ksvm.kernel_svm_predict(Kt2, two["beta"], two["intercept"], two["classes"], return_scores=True)
    assert s2.shape == (9, 1) and np.array_equal(p2, two["classes"][(s2[:, 0] > 0).astype(int)])  # sklearn's one-row convention


def test_wide_predict_reads_rows_in_place_with_the_same_bits():
    """va_linear_svm_predict above 8192 columns (no LDS staging) against numpy in the written order on exact data."""
    rng = np.random.RandomState(1)
    x = rng.randint(-3, 4, (5, 9000)).astype(np.float64)
    w = rng.randint(-3, 4, (3, 9000)).astype(np.float64)
    b = np.array([0.5, -1.0, 2.0])
    pred, scores = fusion.linear_svm_predict(x, w, b, np.arange(3), return_scores=True)
    assert np.array_equal(scores, x @ w.T + b) and np.array_equal(pred, (x @ w.T + b).argmax(1))  # integers: every order is exact
    for dim in (8192, 8193):  # the last staged width and the first one read in place
        xs, ws_ = x[:, :1].repeat(dim, 1) * (np.arange(dim) % 3 - 1.0), w[:, :1].repeat(dim, 1) * (np.arange(dim) % 5 - 2.0)
        _, sc = fusion.linear_svm_predict(xs, ws_, b, np.arange(3), return_scores=True)
        assert np.array_equal(sc, xs @ ws_.T + b)
    with pytest.raises(ValueError, match="1 <= dim <= 65536"):
        fusion.linear_svm_predict(np.zeros((1, 65537)), np.zeros((3, 65537)), b, np.arange(3))


def test_fit_refusals_that_need_the_device():
    K = ksvm.linear_gram(dev(np.random.RandomState(0).randn(6, 3)))
    with pytest.raises(ValueError, match="CUDA"):
        ksvm.kernel_svm_fit(cpu(K), [0, 1] * 3)
    bad = K.clone()
    bad[1, 2] += 1.0
    with pytest.raises(ValueError, match="not symmetric"):
        ksvm.kernel_svm_fit(bad, [0, 1] * 3)
    bad = K.clone()
    bad[1, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        ksvm.kernel_svm_fit(bad, [0, 1] * 3)
    L = _ffi.lib()
    assert L.va_kernel_svm_fit_workspace_bytes(16385, 3) == 0 and "16384" in _ffi.last_error()
    assert L.va_kernel_svm_fit_workspace_bytes(10, 1025) == 0 and L.va_kernel_svm_fit_workspace_bytes(10, 2) == 0
    with pytest.warns(RuntimeWarning, match="not converged after max_iter = 1"):
        f = fitted("three_classes")
        ksvm.kernel_svm_fit(f["Kd"], f["labels"], C=f["C"], max_iter=1)


# ---- each phase alone ------------------------------------------------------------------------------------------------------------

class Stage(object):
    """The workspace of a three-class problem after two outer steps, read and advanced one phase at a time."""

    def __init__(self, name="three_classes"):
        f = fitted(name)
        self.f, self.n, self.rows = f, f["K"].shape[0], f["Y"].shape[0]
        self.H = ko.hessian(f["K"], f["C"], f["s"])
        L = _ffi.lib()
        off = (ctypes.c_size_t * len(_ffi.KSVM_FIT_FIELDS))()
        self.bytes = L.va_kernel_svm_fit_layout(self.n, self.rows, off, len(off))
        assert self.bytes == L.va_kernel_svm_fit_workspace_bytes(self.n, self.rows) > 0
        self.off = dict(zip(_ffi.KSVM_FIT_FIELDS, (int(o) for o in off)))
        assert sorted(self.off.values()) == list(self.off.values()) and all(o % 256 == 0 for o in self.off.values())
        self.work = torch.zeros((self.bytes,), dtype=torch.uint8, device="cuda")
        self.yd = dev(np.unique(f["labels"], return_inverse=True)[1].astype(np.int32))
        out = [torch.empty((self.rows, k), dtype=torch.float64, device="cuda") for k in (self.n, 1, 5)]
        _ffi.check(L.va_kernel_svm_fit(_ffi.ctx(0), _ffi.ptr(f["Kd"]), _ffi.ptr(self.yd), self.n, len(f["classes"]), f["C"], f["s"], TOL, 2, 1,
                                       _ffi.ptr(out[0]), _ffi.ptr(out[1]), _ffi.ptr(out[2]), _ffi.ptr(self.work), self.bytes,
                                       _ffi.stream_ptr(0)))

    def phase(self, name, count=0):
        f = self.f
        _ffi.check(_ffi.lib().va_kernel_svm_fit_phase(_ffi.ctx(0), _ffi.ptr(f["Kd"]), _ffi.ptr(self.yd), self.n, len(f["classes"]), f["C"],
                                                      f["s"], TOL, _ffi.KSVM_PHASES.index(name), count, _ffi.ptr(self.work), self.bytes,
                                                      _ffi.stream_ptr(0)))

    def read(self):
        out, vec = {}, self.rows * self.n
        for k in _ffi.KSVM_FIT_FIELDS:
            ints = k in ("free", "live", "notdone", "tight")
            count = vec if k in _ffi.KSVM_FIT_FIELDS[:10] else self.rows
            raw = self.work[self.off[k]:self.off[k] + count * (4 if ints else 8)]
            a = cpu(raw.view(torch.int32 if ints else torch.float64))
            out[k] = a.reshape(self.rows, self.n) if count == vec else a
        return out


def deviation(got, want, scale):
    return float(np.max(np.abs(np.asarray(got).astype(LD) - want) / np.maximum(scale, LD(1e-300))))


def test_phase_eval_face_candidate_and_stop_rule():
    st = Stage()
    s0 = st.read()
    Y, C = st.f["Y"], st.f["C"]
    fc = ko.face(st.H, s0["B"], Y, C, HB=s0["HB"])  # the face from the device's own product
    assert np.array_equal(s0["free"] != 0, fc["sv"]) and same_bits(np.where(fc["sv"] & (Y * s0["B"] > 0), s0["B"], 0.0), s0["BC"])
    HL = st.H.astype(LD)
    scale = np.abs(s0["B"]).astype(LD) @ np.abs(HL)
    within_16x("H B", deviation(s0["HB"], s0["B"].astype(LD) @ HL, scale),
               deviation(ko.masked_product(st.H, s0["B"]), s0["B"].astype(LD) @ HL, scale))
    scale = np.abs(s0["BC"]).astype(LD) @ np.abs(HL)
    gr = ko.grad(st.H, fc, Y, TOL)
    within_16x("H BC", deviation(s0["Z"], s0["BC"].astype(LD) @ HL, scale), deviation(gr["Z"], s0["BC"].astype(LD) @ HL, scale))
    # what follows the products, from the device's own Z: elementwise and short sums
    g = Y * s0["Z"] - 1.0
    pg = np.where(Y * s0["BC"] > 0, g, np.minimum(g, 0.0))
    assert np.allclose(s0["pgn"], np.sqrt((pg * pg).sum(1)), rtol=1e-13, atol=0)
    assert same_bits(s0["R"], np.where(fc["sv"], Y - s0["Z"], 0.0)) and same_bits(s0["P"], s0["R"]) and same_bits(s0["X"], s0["BC"])
    assert np.allclose(s0["ref"], fc["ref"], rtol=1e-12, atol=0) and np.array_equal(s0["nsv"], (s0["BC"] != 0).sum(1))
    assert np.array_equal(s0["notdone"] != 0, s0["pgn"] > TOL * np.sqrt(st.n)) and s0["notdone"].all()  # two steps in: still running
    assert np.array_equal(s0["live"] != 0, np.sqrt(s0["rr"]) > s0["cgtol"])


def test_phase_cg_masked_product_and_one_step():
    st = Stage()
    s0 = st.read()
    st.phase("cg", 1)
    s1 = st.read()
    HL, free = st.H.astype(LD), s0["free"] != 0
    want = np.where(free, s0["P"].astype(LD) @ HL, 0)
    scale = np.abs(s0["P"]).astype(LD) @ np.abs(HL)
    live = s0["live"] != 0
    assert live.any()
    within_16x("H P masked", deviation(s1["HP"], want, scale), deviation(ko.masked_product(st.H, s0["P"], free), want, scale))
    assert not s1["HP"][~free].any()
    # the step itself from the device's own HP, in long double and in float64
    for r in np.nonzero(live)[0]:
        res = {}
        for T in (LD, np.float64):
            P, R, X, HP = s0["P"][r].astype(T), s0["R"][r].astype(T), s0["X"][r].astype(T), s1["HP"][r].astype(T)
            alpha = T(s0["rr"][r]) / (P @ HP)
            Rn = R - alpha * HP
            res[T] = (X + alpha * P, Rn, Rn + ((Rn @ Rn) / T(s0["rr"][r])) * P, Rn @ Rn)
        for k, i in (("X", 0), ("R", 1)):
            scale = np.abs(s0[k][r]).astype(LD) + np.abs(res[LD][i] - s0[k][r])
            assert deviation(s1[k][r], res[LD][i], scale) <= 16.0 * max(deviation(res[np.float64][i], res[LD][i], scale), 2.0 ** -53), (k, r)
        assert s1["cgs"][r] == s0["cgs"][r] + 1
        if s1["live"][r]:
            assert np.isclose(s1["rr"][r], float(res[LD][3]), rtol=1e-10) and np.sqrt(s1["rr"][r]) > s0["cgtol"][r]
            assert np.allclose(s1["P"][r], res[np.float64][2], rtol=1e-9, atol=1e-9 * np.abs(res[np.float64][2]).max())
        else:
            assert np.sqrt(float(res[LD][3])) <= s0["cgtol"][r] * (1 + 1e-9)


def test_phase_line_search_takes_the_restatement_s_step():
    st = Stage()
    st.phase("cg", 100)
    s0 = st.read()
    st.phase("line_search")
    s1 = st.read()
    Y, C = st.f["Y"], st.f["C"]
    S = s0["X"] - s0["B"]
    assert same_bits(s1["X"], S)
    HL = st.H.astype(LD)
    scale = np.abs(S).astype(LD) @ np.abs(HL)
    within_16x("H S", deviation(s1["Q"], S.astype(LD) @ HL, scale), deviation(ko.masked_product(st.H, S), S.astype(LD) @ HL, scale))
    for r in range(st.rows):
        b, t = ko.line_search(st.H, s0["B"][r], s0["HB"][r], S[r], Y[r], C, Q=s1["Q"][r])
        assert t > 0 and s1["steps"][r] == s0["steps"][r] + 1 and s1["tight"][r] == 0
        assert same_bits(s1["B"][r], s0["B"][r] + t * S[r]), r  # the same step length: B + t S is one multiply and one add


def test_phase_refusals():
    st = Stage()
    for name, count, msg in (("cg", 0, "1 <= count <= 100"), ("cg", 101, "1 <= count <= 100")):
        with pytest.raises(ValueError, match=msg):
            st.phase(name, count)
    f = st.f
    rc = _ffi.lib().va_kernel_svm_fit_phase(_ffi.ctx(0), _ffi.ptr(f["Kd"]), _ffi.ptr(st.yd), st.n, len(f["classes"]), f["C"], f["s"], TOL, 4, 0,
                                            _ffi.ptr(st.work), st.bytes, _ffi.stream_ptr(0))
    assert rc == _ffi.VA_ERR_INVALID and "unknown phase" in _ffi.last_error()
    rc = _ffi.lib().va_kernel_svm_fit_phase(_ffi.ctx(0), _ffi.ptr(f["Kd"]), _ffi.ptr(st.yd), st.n, len(f["classes"]), f["C"], f["s"], TOL, 1, 0,
                                            _ffi.ptr(st.work), st.bytes - 1, _ffi.stream_ptr(0))
    assert rc == _ffi.VA_ERR_WORKSPACE


# ---- end to end ------------------------------------------------------------------------------------------------------------------

def trajectory_videos(n_videos, seed, width=80):
    """tests/test_fisher_gpu.py's planted videos, wide enough for Sheet02's PCA(64)."""
    rng, base = np.random.RandomState(seed), np.random.RandomState(77)
    basis = base.randn(6, width)
    centres = {0: base.randn(3, 6) * 4.0, 1: base.randn(3, 6) * 4.0}
    out, labels = [], []
    for v in range(n_videos):
        c = v % 2
        n = int(rng.randint(150, 250))
        z = rng.randint(0, 3, n)
        out.append(((centres[c][z] + rng.randn(n, 6)) @ basis + 0.05 * rng.randn(n, width)).astype(np.float32))
        labels.append(10 + c)
    return out, np.array(labels)


def test_trajectory_classifier_fits_sheet02_s_own_configuration(tmp_path):
    from video_analytics_amd import trajectories
    train, y = trajectory_videos(12, seed=0)
    tv = [dev(v) for v in train]
    with pytest.raises(ValueError, match="exceeds the 8192 columns"):
        trajectories.TrajectoryClassifier().fit(tv, y)  # the default route refuses as before
    with pytest.raises(ValueError, match="svm must be"):
        trajectories.TrajectoryClassifier().fit(tv, y, svm="kernel")
    clf = trajectories.TrajectoryClassifier().fit(tv, y, svm="dual", max_iter=5)  # PCA(64) x GaussianMixture(256)
    assert clf.coef.shape == (1, 33024) and clf.intercept.shape == (1,) and clf.classes.tolist() == [10, 11]
    assert clf.predict(tv).tolist() == y.tolist()
    clf.save(str(tmp_path / "model.npz"))
    back = trajectories.TrajectoryClassifier.load(str(tmp_path / "model.npz"))
    assert back.predict(tv).tolist() == y.tolist() and np.array_equal(back.coef, clf.coef)


def test_trajectory_classifier_dual_route_gives_the_primal_route_s_model():
    from video_analytics_amd import trajectories
    train, y = trajectory_videos(12, seed=0, width=30)
    tv = [dev(v) for v in train]
    kw = dict(n_components=6, n_gmm=4, power=0.5, max_iter=30)
    a = trajectories.TrajectoryClassifier().fit(tv, y, **kw)
    b = trajectories.TrajectoryClassifier().fit(tv, y, svm="dual", **kw)
    fv = cpu(a.encode(tv)).astype(np.float64)
    Xa, Y = so.augmented(fv), so.signs(y, a.classes)
    Wa, Wb = so.pack(a.coef, a.intercept), so.pack(b.coef, b.intercept)
    bound = np.linalg.norm(so.gradient(Wa, Xa, Y), axis=1) + np.linalg.norm(so.gradient(Wb, Xa, Y), axis=1)
    assert (np.linalg.norm(Wa - Wb, axis=1) <= bound).all()


def test_stip_classifier_with_the_chi_square_kernel(tmp_path):
    from video_analytics_amd import stip
    rng = np.random.RandomState(3)
    centres = rng.randn(2, 4, 12) * 3.0
    videos, labels = [], []
    for v in range(10):
        c = v % 2
        z = rng.randint(0, 4, 60)
        videos.append(dev((centres[c][z] + 0.3 * rng.randn(60, 12)).astype(np.float32)))
        labels.append(c + 5)
    clf = stip.StipClassifier().fit(videos, labels, n_words=8, norm="l1", svm="chi2", C=10.0)
    assert clf.coef is None and clf.kernel_svm.dual_coef.shape == (1, 10) and clf.kernel_svm.scales.shape == (1,)
    assert clf.predict(videos).tolist() == labels
    clf.save(str(tmp_path / "stip.npz"))
    back = stip.StipClassifier.load(str(tmp_path / "stip.npz"))
    assert back.predict(videos).tolist() == labels and back.norm == "l1"
    assert np.array_equal(back.kernel_svm.decision_function(back.encode(videos)), clf.kernel_svm.decision_function(clf.encode(videos)))
    plain = stip.StipClassifier().fit(videos, labels, n_words=8)  # the default route and its file are as before
    plain.save(str(tmp_path / "plain.npz"))
    assert stip.StipClassifier.load(str(tmp_path / "plain.npz")).kernel_svm is None and plain.coef.shape == (1, 8)
    with pytest.raises(ValueError, match="svm must be"):
        stip.StipClassifier().fit(videos, labels, n_words=8, svm="rbf")
