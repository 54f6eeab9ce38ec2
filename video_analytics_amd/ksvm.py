"""Kernel SVMs on the device: chi-square and linear Gram matrices, and a one-vs-rest fit over any positive
semi-definite Gram matrix.

The chi-square kernel ``exp(-sum_c D_c / A_c)`` over one channel per descriptor type is the classifier Laptev's interest points
(Sheet01's method) and Wang's dense trajectories are evaluated with; the linear kernel poses ``fusion.linear_svm_fit``'s problem
over ``n x n`` instead of ``n x d`` and so has no column limit (Sheet02's Fisher vectors have 33,024 columns).

The model is ``fusion.linear_svm_fit``'s: L2-regularised squared hinge, one-vs-rest, regularised bias ``s = intercept_scaling``.
For class row r with ``y_i = +-1`` and ``Kt = K + s^2`` the dual is ``min over alpha >= 0 of 1/2 alpha^T ((y y^T) o Kt + I/(2C))
alpha - e^T alpha``; ``dual_coef[r] = y alpha``, ``intercept[r] = s^2 sum(dual_coef[r])`` and the score of a row x is ``sum_i
dual_coef[r, i] K(x_i, x) + intercept[r]``.  Departures from the literature's libsvm: the squared hinge with a regularised bias
instead of the hinge with a free one, and no factor 1/2 in the chi-square distance (sklearn's ``chi2_kernel`` convention).
"""
import ctypes
import warnings

import numpy as np
import torch

from . import _features
from . import _ffi
from . import fusion

MAX_ROWS, MAX_CLASSES, MAX_DIM = 16384, 1024, 65536  # ksvm.hip: the fit's rows and labels, the Gram kernels' columns
FIT_OUTER_CHUNK = 4  # outer steps enqueued between two reads of the solver's statistics


# ---- Gram matrices ---------------------------------------------------------------------------------------------------------

def _rows(x, who, name="x"):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in (torch.float32, torch.float64) or x.dim() != 2:
        raise ValueError("%s: %s must be a CUDA float32 or float64 [n, d] tensor" % (who, name))
    if x.shape[0] < 1 or not 1 <= x.shape[1] <= MAX_DIM:
        raise ValueError("%s: %s must have at least one row and 1 .. %d columns, got %s" % (who, name, MAX_DIM, tuple(x.shape)))
    return x.contiguous()


def _pair(x, y, who):
    x = _rows(x, who)
    if y is not None:
        y = _rows(y, who, "y")
        if y.dtype != x.dtype or y.device != x.device or y.shape[1] != x.shape[1]:
            raise ValueError("%s: x %s %s and y %s %s must share dtype, device and columns"
                             % (who, x.dtype, tuple(x.shape), y.dtype, tuple(y.shape)))
    return x, y


def check_columns(columns, d, who="chi2_distance"):
    """A column range ``(start, stop)`` with ``0 <= start < stop <= d`` (None: all columns) -> ``(start, stop)`` as ints."""
    if columns is None:
        return 0, int(d)
    try:
        c0, c1 = columns
    except (TypeError, ValueError):
        raise ValueError("%s: a column range must be (start, stop), got %r" % (who, columns))
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (c0, c1)) or not 0 <= c0 < c1 <= d:
        raise ValueError("%s: need 0 <= start < stop <= %d, got %r" % (who, d, columns))
    return int(c0), int(c1)


def chi2_distance(x, y=None, columns=None, chunk=0):
    """``va_chi2_distance``: ``D[i, j] = sum_k (x_ik - y_jk)^2 / (x_ik + y_jk)`` over the columns ``columns = (start, stop)`` in
    ascending order, a term with a zero denominator counting 0 -> CUDA float64 ``[m, n]``.  ``y=None``: the symmetric form
    on ``(x, x)``, which computes one triangle of tiles and mirrors it (bitwise symmetric, the diagonal exactly 0, the bits of
    the call on ``(x, x)``).  ``chunk`` (1 .. 32, 0: the library's) is the staging length; no value changes a result."""
    who = "chi2_distance"
    x, y = _pair(x, y, who)
    c0, c1 = check_columns(columns, x.shape[1], who)
    m, n, dev = int(x.shape[0]), int(x.shape[0] if y is None else y.shape[0]), x.device
    out = torch.empty((m, n), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_chi2_distance(_ffi.ctx(dev.index), _ffi.ptr(x), _ffi.ptr(y), m, n, int(x.shape[1]), c0, c1,
                                               int(x.dtype == torch.float64), int(chunk), _ffi.ptr(out), _ffi.stream_ptr(dev)))
    return out


def linear_gram(x, y=None):
    """``va_linear_gram``: ``x y^T`` on the float64 MFMA -> CUDA float64 ``[m, n]``; ``y=None`` as ``chi2_distance``."""
    who = "linear_gram"
    x, y = _pair(x, y, who)
    m, n, dev = int(x.shape[0]), int(x.shape[0] if y is None else y.shape[0]), x.device
    out = torch.empty((m, n), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_linear_gram(_ffi.ctx(dev.index), _ffi.ptr(x), _ffi.ptr(y), m, n, int(x.shape[1]),
                                             int(x.dtype == torch.float64), _ffi.ptr(out), _ffi.stream_ptr(dev)))
    return out


def upper_mean(dist):
    """``va_upper_mean``: the mean of the strict upper triangle of a CUDA float64 ``[n, n]`` matrix, n >= 2 -> a CUDA float64
    tensor of one element (Laptev's and Wang's normaliser A)."""
    if not isinstance(dist, torch.Tensor) or not dist.is_cuda or dist.dtype != torch.float64 or dist.dim() != 2 \
            or dist.shape[0] != dist.shape[1] or dist.shape[0] < 2:
        raise ValueError("upper_mean: dist must be a CUDA float64 [n, n] tensor with n >= 2")
    dist = dist.contiguous()
    n, dev = int(dist.shape[0]), dist.device
    rowsum = torch.empty((n,), dtype=torch.float64, device=dev)
    mean = torch.empty((1,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_upper_mean(_ffi.ctx(dev.index), _ffi.ptr(dist), n, _ffi.ptr(rowsum), _ffi.ptr(mean), _ffi.stream_ptr(dev)))
    return mean


def combine(dists, weights):
    """``va_chi2_combine``: ``exp(-(w_0 D_0 + w_1 D_1 + ...))`` elementwise over 1 .. 16 CUDA float64 tensors of one shape."""
    who = "combine"
    if not isinstance(dists, (list, tuple)) or not 1 <= len(dists) <= _ffi.CHI2_MAX_CHANNELS:
        raise ValueError("%s: 1 .. %d distance matrices expected" % (who, _ffi.CHI2_MAX_CHANNELS))
    ws = check_scales(weights, len(dists), who)
    first = dists[0]
    for t in dists:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or t.shape != first.shape or t.device != first.device:
            raise ValueError("%s: the distances must be CUDA float64 tensors of one shape on one device" % who)
    dists = [t.contiguous() for t in dists]
    dev = first.device
    out = torch.empty(first.shape, dtype=torch.float64, device=dev)
    if out.numel() == 0:
        return out
    ptrs = (ctypes.c_void_p * len(dists))(*[t.data_ptr() for t in dists])
    cw = (ctypes.c_double * len(dists))(*ws)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_chi2_combine(_ffi.ctx(dev.index), ptrs, cw, len(dists), out.numel(), _ffi.ptr(out), _ffi.stream_ptr(dev)))
    return out


def check_scales(scales, n_channels, who="chi2_kernel"):
    """``n_channels`` finite numbers >= 0 -> a list of floats."""
    try:
        ws = [float(w) for w in np.asarray(scales, dtype=np.float64).reshape(-1)]
    except (TypeError, ValueError):
        raise ValueError("%s: scales must be %d numbers, got %r" % (who, n_channels, scales))
    if len(ws) != n_channels:
        raise ValueError("%s: %d scales for %d channels" % (who, len(ws), n_channels))
    if not all(np.isfinite(w) and w >= 0 for w in ws):
        raise ValueError("%s: scales must be finite and >= 0, got %r" % (who, ws))
    return ws


def check_channels(channels, d, who="chi2_kernel"):
    """``channels``: a list of 1 .. 16 ``(start, stop)`` column ranges (None: one channel of all columns) -> a list of tuples."""
    if channels is None:
        return [(0, int(d))]
    if not isinstance(channels, (list, tuple)) or not 1 <= len(channels) <= _ffi.CHI2_MAX_CHANNELS:
        raise ValueError("%s: channels must be a list of 1 .. %d (start, stop) column ranges" % (who, _ffi.CHI2_MAX_CHANNELS))
    return [check_columns(ch, d, who) for ch in channels]


def check_gamma(gamma, who="chi2_kernel"):
    if gamma is None:
        return None
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.integer, np.floating)) or not np.isfinite(gamma) or gamma <= 0:
        raise ValueError("%s: gamma must be a finite number > 0, got %r" % (who, gamma))
    return float(gamma)


def scales_from_means(means, who="chi2_kernel"):
    """``1 / A_c`` for every channel; ``A_c = 0`` (all rows equal on the channel) or a non-finite mean raises ValueError naming
    the channel."""
    out = []
    for c, a in enumerate(means):
        a = float(a)
        if not np.isfinite(a) or a <= 0.0:
            raise ValueError("%s: the mean chi-square distance A of channel %d is %r: the channel cannot be normalised "
                             "(pass gamma or scales)" % (who, c, a))
        out.append(1.0 / a)
    return out


def check_histograms(x, who="chi2_kernel", name="x"):
    """Histogram rows are finite and >= 0 (one device reduction each)."""
    if not bool(torch.isfinite(x).all()):
        raise ValueError("%s: %s holds non-finite entries" % (who, name))
    if bool((x < 0).any()):
        raise ValueError("%s: %s holds negative entries; the chi-square kernel is defined on histograms" % (who, name))


def chi2_kernel(x, y=None, gamma=None, channels=None, scales=None):
    """The multi-channel chi-square kernel ``K = exp(-sum_c scales[c] D_c)`` with ``D_c = chi2_distance`` over channel c
    -> ``(K CUDA float64 [m, n], scales float64 numpy [n_channels])``.

    ``channels``: a list of ``(start, stop)`` column ranges, one per descriptor type (default: one channel of all columns).
    ``y=None``: the training kernel (symmetric, diagonal exactly 1); without ``gamma`` and ``scales`` it takes ``scales[c] =
    1 / A_c``, ``A_c`` the mean of ``D_c`` over the pairs i < j (Laptev's and Wang's normaliser).  ``gamma``: ``scales[c] =
    gamma`` for every channel (sklearn's ``chi2_kernel``).  With ``y`` given (rows x against the training rows y), ``scales`` or
    ``gamma`` must be passed: the training set's.  Negative or non-finite entries and ``A_c = 0`` raise ValueError."""
    who = "chi2_kernel"
    x, y = _pair(x, y, who)
    chans = check_channels(channels, x.shape[1], who)
    gamma = check_gamma(gamma, who)
    if gamma is not None and scales is not None:
        raise ValueError("%s: pass gamma or scales, not both" % who)
    if y is not None and gamma is None and scales is None:
        raise ValueError("%s: with y given, pass the training set's scales (or gamma)" % who)
    if y is None and x.shape[0] < 2 and gamma is None and scales is None:
        raise ValueError("%s: the normaliser A needs at least two rows" % who)
    check_histograms(x, who)
    if y is not None:
        check_histograms(y, who, "y")
    dists = [chi2_distance(x, y, ch) for ch in chans]
    if scales is not None:
        ws = check_scales(scales, len(chans), who)
    elif gamma is not None:
        ws = [gamma] * len(chans)
    else:
        ws = scales_from_means(torch.cat([upper_mean(D) for D in dists]).cpu().numpy(), who)  # the one read of the host
    return combine(dists, ws), np.asarray(ws, dtype=np.float64)


# ---- the fit ---------------------------------------------------------------------------------------------------------------

def check_kernel_svm_fit_args(K, labels, C=1.0, tol=1e-8, max_iter=100, fit_intercept=True, intercept_scaling=1.0):
    """The argument check of ``kernel_svm_fit``, on the host alone when K is a numpy array or a CPU tensor (a CUDA K is judged
    by device reductions): ValueError for a K that is not a square float64 ``[n, n]`` with ``2 <= n <= 16384``, holds non-finite
    values or is not symmetric, labels of another length, fewer than 2 or more than 1024 distinct labels, and C, tol, max_iter
    or intercept_scaling out of range.  -> ``(classes, y)`` as ``fusion.check_svm_fit_args``."""
    who = "kernel_svm_fit"
    for name, v, positive in (("C", C, True), ("tol", tol, True), ("intercept_scaling", intercept_scaling, bool(fit_intercept))):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) \
                or (v <= 0 if positive else v < 0):
            raise ValueError("%s: %s must be a finite number %s 0, got %r" % (who, name, ">" if positive else ">=", v))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError("%s: max_iter must be an integer >= 1 (outer steps), got %r" % (who, max_iter))
    if not isinstance(K, torch.Tensor):
        try:
            K = torch.as_tensor(np.asarray(K, dtype=np.float64))
        except (TypeError, ValueError):
            raise ValueError("%s: K must be numbers [n, n]" % who)
    if K.dtype != torch.float64:
        raise ValueError("%s: K must be float64, got %s" % (who, K.dtype))
    if K.dim() != 2 or K.shape[0] != K.shape[1]:
        raise ValueError("%s: K must be square [n, n], got shape %s" % (who, tuple(K.shape)))
    n = int(K.shape[0])
    if n < 2 or n > MAX_ROWS:
        raise ValueError("%s: need 2 <= n <= %d training rows, got %d" % (who, MAX_ROWS, n))
    if not bool(torch.isfinite(K).all()):
        raise ValueError("%s: K holds non-finite values" % who)
    if not bool(torch.equal(K, K.t())):
        raise ValueError("%s: K is not symmetric" % who)
    labels = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
    if labels.ndim != 1 or labels.shape[0] != n:
        raise ValueError("%s: K has %d rows but labels of shape %s" % (who, n, tuple(labels.shape)))
    if labels.dtype.kind == "f" and not np.isfinite(labels).all():
        raise ValueError("%s: labels hold non-finite values" % who)
    classes, y = np.unique(labels, return_inverse=True)
    if len(classes) < 2 or len(classes) > MAX_CLASSES:
        raise ValueError("%s: need 2 .. %d distinct labels, got %d" % (who, MAX_CLASSES, len(classes)))
    return classes, np.ascontiguousarray(y.reshape(-1), dtype=np.int32)


def kernel_svm_fit(K, labels, C=1.0, tol=1e-8, max_iter=100, fit_intercept=True, intercept_scaling=1.0, return_info=False):
    """The one-vs-rest kernel SVM over a CUDA float64 Gram matrix ``K [n, n]`` (symmetric positive semi-definite, 2 <= n <=
    16384): ``va_kernel_svm_fit``, DESIGN.md S104-S108.  -> ``(dual_coef [rows, n] CUDA float64, intercept [rows] float64 numpy,
    classes)``; ``classes = np.unique(labels)``, and two classes give ONE row, for ``classes[1]``.  ``alpha = y dual_coef`` is
    >= 0 exactly and its zeros are exact (the rows with a nonzero are the support vectors).

    A row stops when the dual's projected gradient has ``|pg|_2 <= tol sqrt(n)`` (``sqrt(n)`` is the norm at ``alpha = 0``);
    then ``|alpha - alpha*|_2 <= 2C |pg|_2``.  ``max_iter`` counts outer steps; reaching it with a row not converged is a
    ``RuntimeWarning`` and the iterate is returned.  With ``K = linear_gram(X)`` the model ``dual_coef [X, s]`` is
    ``fusion.linear_svm_fit``'s.  ``return_info=True`` adds ``{"n_iter", "rel_pg" [rows] (|pg| / sqrt(n)), "objective" [rows]
    (the dual's), "converged", "steps" [rows], "cg_steps" [rows], "n_sv" [rows]}``.  Two calls give the same bits."""
    who = "kernel_svm_fit"
    if not isinstance(K, torch.Tensor) or not K.is_cuda:
        raise ValueError("%s: K must be a CUDA float64 [n, n] tensor (ksvm.chi2_kernel, ksvm.linear_gram)" % who)
    classes, y = check_kernel_svm_fit_args(K, labels, C, tol, max_iter, fit_intercept, intercept_scaling)
    K = K.contiguous()
    n, dev = int(K.shape[0]), K.device
    rows = 1 if len(classes) == 2 else len(classes)
    scale = float(intercept_scaling) if fit_intercept else 0.0
    L = _ffi.lib()
    work = _features.workspace(L.va_kernel_svm_fit_workspace_bytes(n, rows), dev)
    yd = torch.as_tensor(y).to(dev)
    dual_coef = torch.empty((rows, n), dtype=torch.float64, device=dev)
    intercept = torch.empty((rows,), dtype=torch.float64, device=dev)
    stats = torch.empty((rows, 5), dtype=torch.float64, device=dev)
    bound = float(tol) * np.sqrt(n)
    enqueued, restart = 0, 1
    with torch.cuda.device(dev):
        while True:
            steps = min(int(FIT_OUTER_CHUNK), int(max_iter) - enqueued)
            _ffi.check(L.va_kernel_svm_fit(_ffi.ctx(dev.index), _ffi.ptr(K), _ffi.ptr(yd), n, len(classes), float(C), scale, float(tol),
                                           steps, restart, _ffi.ptr(dual_coef), _ffi.ptr(intercept), _ffi.ptr(stats), _ffi.ptr(work),
                                           work.numel(), _ffi.stream_ptr(dev)))
            enqueued, restart = enqueued + steps, 0
            st = stats.cpu().numpy()  # the one synchronisation of a round
            converged = bool((st[:, 1] <= bound).all())
            if converged or enqueued >= int(max_iter):
                break
    if not converged:
        warnings.warn("%s: %d of %d class rows not converged after max_iter = %d outer steps"
                      % (who, int((st[:, 1] > bound).sum()), rows, int(max_iter)), RuntimeWarning)
    out = (dual_coef, intercept.cpu().numpy(), classes)
    if not return_info:
        return out
    info = {"n_iter": int(st[:, 3].max()), "rel_pg": st[:, 1] / np.sqrt(n), "objective": st[:, 0].copy(), "converged": converged,
            "steps": st[:, 3].astype(np.int64), "cg_steps": st[:, 4].astype(np.int64), "n_sv": st[:, 2].astype(np.int64)}
    return out + (info,)


def kernel_svm_predict(K_test, dual_coef, intercept, classes, return_scores=False):
    """``scores = K_test dual_coef^T + intercept`` and the labels: ``va_linear_svm_predict`` with ``dim = n`` on ``K_test [m,
    n]``, the kernel of every test row against the n training rows -- ``fusion.linear_svm_predict``'s bits.  A CUDA float64
    ``K_test`` stays on the device, and so does a CUDA ``dual_coef``; anything else goes through
    ``fusion.linear_svm_predict``.  The binary case keeps sklearn's one-row convention.  -> labels, or ``(labels, scores
    float64 numpy [m, rows])``."""
    who = "kernel_svm_predict"
    if not (isinstance(K_test, torch.Tensor) and K_test.is_cuda and K_test.dtype == torch.float64):
        dc = dual_coef.detach().cpu().numpy() if isinstance(dual_coef, torch.Tensor) else dual_coef
        return fusion.linear_svm_predict(K_test, dc, intercept, classes, return_scores=return_scores)
    dev = K_test.device
    x = K_test.contiguous()
    w = dual_coef.to(device=dev, dtype=torch.float64) if isinstance(dual_coef, torch.Tensor) else _features.dev64(np.atleast_2d(dual_coef), dev)
    w = w.reshape(1, -1).contiguous() if w.dim() == 1 else w.contiguous()
    b = _features.dev64(np.atleast_1d(np.asarray(intercept, dtype=np.float64)), dev)
    classes = np.asarray(classes)
    if x.dim() != 2 or w.dim() != 2 or x.shape[0] < 1 or x.shape[1] != w.shape[1] or b.shape[0] != w.shape[0]:
        raise ValueError("%s: shapes K_test[m,n], dual_coef[rows,n], intercept[rows] expected, got %s %s %s"
                         % (who, tuple(x.shape), tuple(w.shape), tuple(b.shape)))
    if len(classes) != (2 if w.shape[0] == 1 else w.shape[0]):
        raise ValueError("%s: %d classes for %d coefficient rows" % (who, len(classes), w.shape[0]))
    m, rows = int(x.shape[0]), int(w.shape[0])
    scores = torch.empty((m, rows), dtype=torch.float64, device=dev)
    pred = torch.empty((m,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_linear_svm_predict(_ffi.ctx(dev.index), _ffi.ptr(x), m, int(x.shape[1]), _ffi.ptr(w), _ffi.ptr(b), rows,
                                                    _ffi.ptr(scores), _ffi.ptr(pred), _ffi.stream_ptr(dev)))
    out = classes[pred.cpu().numpy()]
    return (out, scores.cpu().numpy()) if return_scores else out


# ---- the classifier --------------------------------------------------------------------------------------------------------

KERNELS = ("chi2", "linear")


class KernelSvm(object):
    """``fit(x, labels)``, ``predict(x)``, ``decision_function(x)``, ``save`` and ``load`` over CUDA float32 or float64 rows.

    ``kernel="chi2"``: the multi-channel chi-square kernel (``channels``: ``(start, stop)`` column ranges; ``gamma=None``
    normalises every channel by its mean distance); the model keeps the training rows and ``dual_coef`` on the device, and
    the scales.
    ``kernel="linear"``: the fit runs over ``linear_gram(x)`` and the model collapses to ``coef = dual_coef x`` and
    ``intercept``, predicted through ``fusion.linear_svm_predict``."""

    def __init__(self, kernel="chi2", C=1.0, channels=None, gamma=None, tol=1e-8, max_iter=100, fit_intercept=True, intercept_scaling=1.0):
        if kernel not in KERNELS:
            raise ValueError("KernelSvm: kernel must be 'chi2' or 'linear', got %r" % (kernel,))
        self.kernel, self.C, self.channels, self.gamma = kernel, C, channels, check_gamma(gamma, "KernelSvm")
        self.tol, self.max_iter, self.fit_intercept, self.intercept_scaling = tol, max_iter, fit_intercept, intercept_scaling
        self.train = self.scales = self.dual_coef = self.coef = self.intercept = self.classes = self.info = None

    def fit(self, x, labels):
        x = _rows(x, "KernelSvm.fit")
        kw = dict(C=self.C, tol=self.tol, max_iter=self.max_iter, fit_intercept=self.fit_intercept,
                  intercept_scaling=self.intercept_scaling, return_info=True)
        if self.kernel == "chi2":
            K, self.scales = chi2_kernel(x, None, self.gamma, self.channels)
            dual_coef, self.intercept, self.classes, self.info = kernel_svm_fit(K, labels, **kw)
            self.train, self.dual_coef = x, dual_coef
        else:
            dual_coef, self.intercept, self.classes, self.info = kernel_svm_fit(linear_gram(x), labels, **kw)
            self.coef = (dual_coef @ x.to(torch.float64)).cpu().numpy()
        return self

    def _scores(self, x, who):
        if self.classes is None:
            raise ValueError("%s: the model is not fitted" % who)
        x = _rows(x, who)
        if self.kernel == "chi2":
            K_test, _ = chi2_kernel(x.to(self.train.dtype), self.train.to(x.device), channels=self.channels, scales=self.scales)
            return kernel_svm_predict(K_test, self.dual_coef.to(x.device), self.intercept, self.classes, return_scores=True)
        return fusion.linear_svm_predict(x.double().cpu().numpy(), self.coef, self.intercept, self.classes, device=x.device.index,
                                         return_scores=True)

    def predict(self, x):
        return self._scores(x, "KernelSvm.predict")[0]

    def decision_function(self, x):
        """-> float64 numpy ``[m, rows]`` (one column for two classes)."""
        return self._scores(x, "KernelSvm.decision_function")[1]

    def state(self):
        """The arrays ``save`` writes (``StipClassifier`` stores them beside its codebook)."""
        if self.classes is None:
            raise ValueError("KernelSvm.save: the model is not fitted")
        out = {"kernel": np.str_(self.kernel), "C": np.float64(self.C), "intercept": self.intercept, "classes": self.classes,
               "intercept_scaling": np.float64(self.intercept_scaling if self.fit_intercept else 0.0)}
        if self.kernel == "chi2":
            chans = check_channels(self.channels, self.train.shape[1], "KernelSvm")
            out.update(train=self.train.cpu().numpy(), scales=self.scales, dual_coef=self.dual_coef.cpu().numpy(),
                       channels=np.asarray(chans, dtype=np.int64).reshape(-1, 2))
        else:
            out.update(coef=self.coef)
        return out

    @classmethod
    def from_state(cls, z, device=None, prefix=""):
        kernel = str(z[prefix + "kernel"])
        m = cls(kernel, float(z[prefix + "C"]))
        m.intercept, m.classes = np.asarray(z[prefix + "intercept"]), np.asarray(z[prefix + "classes"])
        s = float(z[prefix + "intercept_scaling"])
        m.fit_intercept, m.intercept_scaling = s > 0.0, s if s > 0.0 else 1.0
        if kernel == "chi2":
            dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
            m.train = torch.as_tensor(np.asarray(z[prefix + "train"])).to(dev)
            m.scales, m.dual_coef = np.asarray(z[prefix + "scales"]), torch.as_tensor(np.asarray(z[prefix + "dual_coef"])).to(dev)
            m.channels = [tuple(int(v) for v in ch) for ch in np.asarray(z[prefix + "channels"])]
        else:
            m.coef = np.asarray(z[prefix + "coef"])
        return m

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, **self.state())

    @classmethod
    def load(cls, path, device=None):
        with np.load(path) as z:
            return cls.from_state(z, device)
