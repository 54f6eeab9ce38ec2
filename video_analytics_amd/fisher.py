"""Fisher vectors on MI355X (``csrc/fisher.hip``): the part of the modelled project's Sheet02 between the
trajectory descriptors and the linear SVM (Sheet02.py:568-617) -- PCA to 64 dimensions (Sheet02.py:40, 574), a 256-component
diagonal-covariance Gaussian mixture (Sheet02.py:41, 582) and one Fisher vector of length ``K + 2 K D`` per video
(Sheet02.py:588-617).

The descriptors are CUDA float32 tensors (what ``trajectories.dense_trajectories`` returns as ``desc``); every sum is float64
in a fixed order, so two calls give the same bits.  The dense work -- ``X^T X``, the projection, the log-densities and the
``gamma^T [1, x, x^2]`` statistics -- is HIP on the float64 MFMA; the 426 x 426 eigen-decomposition of the PCA is a host job
(``torch.linalg.eigh`` on the CPU).  No part of this module needs scikit-learn.

Where it departs from Sheet02, deliberately: ``getFisherVector`` multiplies ``predict_proba``'s output, which already is the
posterior, by the mixture weights again and renormalises (Sheet02.py:599-602).  Here gamma is the posterior.
"""
import ctypes

import numpy as np
import torch

from . import _ffi
from ._features import check_rows, check_segments, dev64, workspace

EPSILON = 1e-6  # Sheet02.py:39: a Fisher vector whose norm is below it is stored as it is
MAX_PCA_DIM, MAX_GMM_DIM, MAX_GMM_COMPONENTS, MAX_POSTERIOR_ROWS = 2048, 512, 256, 65536


# ---- PCA -----------------------------------------------------------------------------------------------------------------

def pca_moments(descs):
    """``va_pca_moments`` over a CUDA float32 ``[N,d]`` tensor or a list of them (empty ones are skipped): the first call
    stores, the others add.  -> ``(count, column sums [d], upper triangle of X^T X [d,d])`` as float64 numpy."""
    who = "pca_moments"
    parts = [descs] if isinstance(descs, torch.Tensor) else list(descs)
    parts = [check_rows(p, who, MAX_PCA_DIM, "descs") for p in parts]
    parts = [p for p in parts if p.shape[0] > 0]
    if not parts:
        raise ValueError("%s: descs holds no rows" % who)
    d, dev = int(parts[0].shape[1]), parts[0].device
    for p in parts:
        if p.shape[1] != d or p.device != dev:
            raise ValueError("%s: descs must share one width and one device" % who)
    L = _ffi.lib()
    sums = torch.empty((1 + d + d * d,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        for i, p in enumerate(parts):
            n = int(p.shape[0])
            ws = workspace(L.va_pca_workspace_bytes(n, d), dev)
            _ffi.check(L.va_pca_moments(_ffi.ctx(dev.index), _ffi.ptr(p), n, d, int(i == 0), _ffi.ptr(sums), _ffi.ptr(ws), ws.numel(),
                                        _ffi.stream_ptr(dev)))
        s = sums.cpu().numpy()
    return float(s[0]), s[1:1 + d].copy(), s[1 + d:].reshape(d, d).copy()


class PCAModel(object):
    """What ``pca_fit`` returns: ``mean [d]``, ``components [m,d]``, ``explained_variance [m]`` (float64 numpy) and
    ``n_samples``."""

    def __init__(self, mean, components, explained_variance, n_samples):
        self.mean = np.ascontiguousarray(mean, dtype=np.float64)
        self.components = np.ascontiguousarray(components, dtype=np.float64)
        self.explained_variance = np.ascontiguousarray(explained_variance, dtype=np.float64)
        self.n_samples = int(n_samples)

    def transform(self, x):
        """``(x - mean) components^T`` for a CUDA float32 ``[n,d]`` tensor -> CUDA float32 ``[n,m]`` (``va_pca_transform``:
        float64 accumulation, no whitening)."""
        x = check_rows(x, "PCAModel.transform", MAX_PCA_DIM)
        m, d = self.components.shape
        if x.shape[1] != d:
            raise ValueError("PCAModel.transform: x has %d columns, the model %d" % (x.shape[1], d))
        dev, n = x.device, int(x.shape[0])
        out = torch.empty((n, m), dtype=torch.float32, device=dev)
        if n == 0:
            return out
        mean, comp = dev64(self.mean, dev), dev64(self.components, dev)
        with torch.cuda.device(dev):
            _ffi.check(_ffi.lib().va_pca_transform(_ffi.ctx(dev.index), _ffi.ptr(x), n, d, _ffi.ptr(mean), _ffi.ptr(comp), m, _ffi.ptr(out),
                                                   _ffi.stream_ptr(dev)))
        return out

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, mean=self.mean, components=self.components, explained_variance=self.explained_variance,
                     n_samples=np.int64(self.n_samples))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["mean"], z["components"], z["explained_variance"], int(z["n_samples"]))


def pca_from_moments(count, colsum, xtx_upper, n_components):
    """The host half of ``pca_fit``: covariance with ``ddof = 1`` in float64, ``torch.linalg.eigh`` on the CPU, the largest
    ``n_components`` eigenvalues in descending order, each component flipped so that its entry of largest magnitude is
    positive (sklearn's ``svd_flip``)."""
    n, d = int(round(count)), len(colsum)
    if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) or n_components < 1:
        raise ValueError("pca_fit: n_components must be an integer >= 1, got %r" % (n_components,))
    if n_components > min(n - 1, d):
        raise ValueError("pca_fit: n_components = %d exceeds min(N - 1, d) = %d" % (n_components, min(n - 1, d)))
    mean = colsum / n
    up = np.triu(xtx_upper)
    xtx = up + np.triu(up, 1).T
    cov = (xtx - n * np.outer(mean, mean)) / (n - 1)
    vals, vecs = torch.linalg.eigh(torch.from_numpy(cov))
    vals, vecs = vals.numpy()[::-1][:n_components], vecs.numpy()[:, ::-1][:, :n_components].T
    vecs = np.ascontiguousarray(vecs)
    big = np.argmax(np.abs(vecs), axis=1)
    vecs *= np.sign(vecs[np.arange(len(vecs)), big])[:, None]
    return PCAModel(mean, vecs, np.maximum(vals, 0.0), n)


def pca_fit(descs, n_components=64):
    """PCA of a CUDA float32 ``[N,d]`` tensor or a list of them, ``d <= 2048`` (Sheet02.py:568-575 with 64 components,
    Sheet02.py:40): the moments on the device (one call per tensor, so a training set need not sit in one tensor), the
    eigen-decomposition on the host.  -> ``PCAModel``.  ``n_components > min(N - 1, d)`` raises ValueError."""
    return pca_from_moments(*pca_moments(descs), n_components=n_components)


# ---- the mixture ---------------------------------------------------------------------------------------------------------

def _gmm_params(chunk_rows, batch_rows):
    over = {}
    if chunk_rows is not None:
        over["chunk_rows"] = int(chunk_rows)
    if batch_rows is not None:
        over["batch_rows"] = int(batch_rows)
    return _ffi.default_gmm_params(**over)


def gmm_stats(x, segments, weights, means, variances, mode="soft", chunk_rows=None, batch_rows=None):
    """``va_gmm_stats``: x CUDA float32 ``[n,d]`` (n >= 1, d <= 512), segments ``[n_segments + 1]`` ascending from 0 to n,
    the parameters float64 ``[k]``, ``[k,d]``, ``[k,d]`` (k <= 256) as arrays or tensors on x's device.  ``mode``: "soft"
    (posteriors) or "hard" (one-hot of the arg-max, lowest component on ties).  -> ``(stats, loglik)``: CUDA float64
    ``[n_segments, k, 1 + 2d]`` = ``[S0 | S1 | S2]`` and ``[n_segments]``."""
    who = "gmm_stats"
    x = check_rows(x, who, MAX_GMM_DIM)
    if mode not in ("soft", "hard"):
        raise ValueError("%s: mode must be 'soft' or 'hard', got %r" % (who, mode))
    n, d, dev = int(x.shape[0]), int(x.shape[1]), x.device
    if n < 1:
        raise ValueError("%s: x holds no rows" % who)
    seg = check_segments(segments, n, who)
    w, mu, var = (t.to(device=dev, dtype=torch.float64).contiguous() if isinstance(t, torch.Tensor) else dev64(t, dev)
                  for t in (weights, means, variances))
    k = int(w.shape[0])
    if w.dim() != 1 or tuple(mu.shape) != (k, d) or tuple(var.shape) != (k, d):
        raise ValueError("%s: weights [k], means [k,%d], variances [k,%d] expected, got %s %s %s"
                         % (who, d, d, tuple(w.shape), tuple(mu.shape), tuple(var.shape)))
    L, p, ns = _ffi.lib(), _gmm_params(chunk_rows, batch_rows), len(seg) - 1
    ws = workspace(L.va_gmm_workspace_bytes(n, d, k, ns, ctypes.byref(p)), dev)
    segd = torch.as_tensor(seg).to(dev)
    stats = torch.empty((ns, k, 1 + 2 * d), dtype=torch.float64, device=dev)
    loglik = torch.empty((ns,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(L.va_gmm_stats(_ffi.ctx(dev.index), _ffi.ptr(x), n, d, _ffi.ptr(segd), ns, _ffi.ptr(w), _ffi.ptr(mu), _ffi.ptr(var), k,
                                  _ffi.VA_GMM_HARD if mode == "hard" else _ffi.VA_GMM_SOFT, ctypes.byref(p), _ffi.ptr(stats),
                                  _ffi.ptr(loglik), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(dev)))
    return stats, loglik


def gmm_mstep(stats, reg_covar=1e-6):
    """``va_gmm_mstep`` on CUDA float64 stats ``[n_segments, k, 1 + 2d]`` (summed over the segments in ascending order):
    sklearn's diagonal M-step.  -> ``(weights [k], means [k,d], variances [k,d])`` CUDA float64."""
    who = "gmm_mstep"
    if not isinstance(stats, torch.Tensor) or not stats.is_cuda or stats.dtype != torch.float64 or stats.dim() != 3 \
            or stats.shape[2] % 2 != 1 or stats.shape[2] < 3:
        raise ValueError("%s: stats must be a CUDA float64 [n_segments, k, 1 + 2d] tensor" % who)
    if isinstance(reg_covar, bool) or not isinstance(reg_covar, (int, float, np.integer, np.floating)) or not np.isfinite(reg_covar) \
            or reg_covar < 0:
        raise ValueError("%s: reg_covar must be a finite number >= 0, got %r" % (who, reg_covar))
    stats = stats.contiguous()
    ns, k, d, dev = int(stats.shape[0]), int(stats.shape[1]), (int(stats.shape[2]) - 1) // 2, stats.device
    w = torch.empty((k,), dtype=torch.float64, device=dev)
    mu = torch.empty((k, d), dtype=torch.float64, device=dev)
    var = torch.empty((k, d), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_gmm_mstep(_ffi.ctx(dev.index), _ffi.ptr(stats), ns, k, d, float(reg_covar), _ffi.ptr(w), _ffi.ptr(mu),
                                           _ffi.ptr(var), _ffi.stream_ptr(dev)))
    return w, mu, var


class GMMModel(object):
    """What ``gmm_fit`` returns: ``weights [K]``, ``means [K,D]``, ``variances [K,D]`` (float64 numpy), ``converged``,
    ``n_iter``, ``lower_bound`` (the last per-row mean log-likelihood) and ``history`` (one per iteration)."""

    def __init__(self, weights, means, variances, converged=False, n_iter=0, lower_bound=float("-inf"), history=()):
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        self.means = np.ascontiguousarray(means, dtype=np.float64)
        self.variances = np.ascontiguousarray(variances, dtype=np.float64)
        if self.weights.ndim != 1 or self.means.ndim != 2 or self.means.shape != self.variances.shape \
                or self.means.shape[0] != self.weights.shape[0]:
            raise ValueError("GMMModel: weights [K], means [K,D], variances [K,D] expected")
        self.converged, self.n_iter, self.lower_bound = bool(converged), int(n_iter), float(lower_bound)
        self.history = [float(h) for h in history]

    def posteriors(self, x, mode="soft"):
        """The responsibilities ``[n,K]`` float64 (numpy) of a CUDA float32 ``[n,D]`` tensor: for tests and small inputs
        only, at most 65536 rows -- the library itself never holds them for more than one batch of rows."""
        who = "GMMModel.posteriors"
        x = check_rows(x, who, MAX_GMM_DIM)
        n, d, dev, k = int(x.shape[0]), int(x.shape[1]), x.device, len(self.weights)
        if d != self.means.shape[1]:
            raise ValueError("%s: x has %d columns, the model %d" % (who, d, self.means.shape[1]))
        if n < 1 or n > MAX_POSTERIOR_ROWS:
            raise ValueError("%s: x must hold 1 .. %d rows, got %d" % (who, MAX_POSTERIOR_ROWS, n))
        if mode not in ("soft", "hard"):
            raise ValueError("%s: mode must be 'soft' or 'hard', got %r" % (who, mode))
        L = _ffi.lib()
        ws = workspace(L.va_gmm_workspace_bytes(n, d, k, 1, None), dev)
        w, mu, var = dev64(self.weights, dev), dev64(self.means, dev), dev64(self.variances, dev)
        g = torch.empty((n, k), dtype=torch.float64, device=dev)
        lse = torch.empty((n,), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _ffi.check(L.va_gmm_posteriors(_ffi.ctx(dev.index), _ffi.ptr(x), n, d, _ffi.ptr(w), _ffi.ptr(mu), _ffi.ptr(var), k,
                                           _ffi.VA_GMM_HARD if mode == "hard" else _ffi.VA_GMM_SOFT, _ffi.ptr(g), _ffi.ptr(lse),
                                           _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(dev)))
        return g.cpu().numpy()

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, weights=self.weights, means=self.means, variances=self.variances, converged=np.bool_(self.converged),
                     n_iter=np.int64(self.n_iter), lower_bound=np.float64(self.lower_bound), history=np.asarray(self.history, dtype=np.float64))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["weights"], z["means"], z["variances"], bool(z["converged"]), int(z["n_iter"]), float(z["lower_bound"]),
                       z["history"].tolist())


def check_gmm_fit_args(n_components, tol, max_iter, reg_covar, seed, kmeans_iters):
    """The scalar argument checks of ``gmm_fit``, on the host alone: ValueError naming the argument."""
    who = "gmm_fit"
    for name, v, lo in (("n_components", n_components, 1), ("max_iter", max_iter, 1), ("kmeans_iters", kmeans_iters, 0), ("seed", seed, 0)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError("%s: %s must be an integer >= %d, got %r" % (who, name, lo, v))
    if n_components > MAX_GMM_COMPONENTS:
        raise ValueError("%s: n_components must be <= %d, got %d" % (who, MAX_GMM_COMPONENTS, n_components))
    for name, v in (("tol", tol), ("reg_covar", reg_covar)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
            raise ValueError("%s: %s must be a finite number >= 0, got %r" % (who, name, v))


def gmm_fit(x, n_components=256, *, tol=1e-3, max_iter=100, reg_covar=1e-6, seed=0, kmeans_iters=10, init=None, chunk_rows=None,
            batch_rows=None):
    """A diagonal-covariance Gaussian mixture fitted by EM on the device (Sheet02.py:578-584 with 256 components,
    Sheet02.py:41): x CUDA float32 ``[N,D]``, D <= 512, n_components <= min(N, 256).

    ``init=(weights, means, variances)`` starts EM from exactly those parameters.  Otherwise the means start as the rows
    ``numpy.random.RandomState(seed).permutation(N)[:K]``, with equal weights and unit variances ``kmeans_iters`` hard passes
    (Lloyd steps) refine them -- an empty cluster keeps its mean --, one more hard pass gives one-hot statistics and the
    M-step turns those into the initial parameters (sklearn's initialisation from responsibilities, with this library's own
    k-means).  EM alternates ``va_gmm_stats`` and ``va_gmm_mstep`` and stops when the per-row mean log-likelihood moves by
    less than ``tol`` (sklearn's rule) or after ``max_iter`` iterations; the host reads one float64 per iteration.  A
    non-finite log-likelihood raises RuntimeError naming the iteration.  -> ``GMMModel``."""
    who = "gmm_fit"
    x = check_rows(x, who, MAX_GMM_DIM)
    check_gmm_fit_args(n_components, tol, max_iter, reg_covar, seed, kmeans_iters)
    n, d, dev, k = int(x.shape[0]), int(x.shape[1]), x.device, int(n_components)
    if n < k:
        raise ValueError("%s: n_components = %d exceeds the %d rows of x" % (who, k, n))
    seg = np.array([0, n], dtype=np.int64)
    kw = dict(chunk_rows=chunk_rows, batch_rows=batch_rows)
    if init is not None:
        if not isinstance(init, (tuple, list)) or len(init) != 3:
            raise ValueError("%s: init must be (weights, means, variances)" % who)
        w, mu, var = (dev64(a, dev) for a in init)
        if tuple(w.shape) != (k,) or tuple(mu.shape) != (k, d) or tuple(var.shape) != (k, d):
            raise ValueError("%s: init must hold weights [%d], means [%d,%d], variances [%d,%d]" % (who, k, k, d, k, d))
    else:
        rows = np.random.RandomState(int(seed)).permutation(n)[:k]
        mu = x[torch.as_tensor(rows, device=dev)].to(torch.float64)
        w = torch.full((k,), 1.0 / k, dtype=torch.float64, device=dev)
        var = torch.ones((k, d), dtype=torch.float64, device=dev)
        for _ in range(int(kmeans_iters)):
            st, _ll = gmm_stats(x, seg, w, mu, var, "hard", **kw)
            s0 = st[0, :, :1]
            mu = torch.where(s0 > 0, st[0, :, 1:1 + d] / torch.where(s0 > 0, s0, torch.ones_like(s0)), mu)
        st, _ll = gmm_stats(x, seg, w, mu, var, "hard", **kw)
        w, mu, var = gmm_mstep(st, reg_covar)
    history, converged, prev = [], False, float("-inf")
    for it in range(1, int(max_iter) + 1):
        st, ll = gmm_stats(x, seg, w, mu, var, "soft", **kw)
        w, mu, var = gmm_mstep(st, reg_covar)
        lb = float(ll.item()) / n  # the one value the host reads per iteration
        if not np.isfinite(lb):
            raise RuntimeError("%s: the log-likelihood is not finite (%r) at iteration %d" % (who, lb, it))
        history.append(lb)
        if abs(lb - prev) < tol:
            converged = True
            break
        prev = lb
    return GMMModel(w.cpu().numpy(), mu.cpu().numpy(), var.cpu().numpy(), converged, len(history), history[-1], history)


# ---- Fisher vectors ------------------------------------------------------------------------------------------------------

def fisher_encode(stats, counts, weights, means, variances, power=0.0):
    """``va_fisher_encode``: CUDA float64 stats ``[n_segments, k, 1 + 2d]`` and the segments' row counts ``[n_segments]`` ->
    CUDA float32 ``[n_segments, k + 2 k d]``."""
    who = "fisher_encode"
    if not isinstance(stats, torch.Tensor) or not stats.is_cuda or stats.dtype != torch.float64 or stats.dim() != 3:
        raise ValueError("%s: stats must be a CUDA float64 [n_segments, k, 1 + 2d] tensor" % who)
    if isinstance(power, bool) or not isinstance(power, (int, float, np.integer, np.floating)) or not 0.0 <= power <= 1.0:
        raise ValueError("%s: power must be a number in [0, 1], got %r" % (who, power))
    stats = stats.contiguous()
    ns, k, d, dev = int(stats.shape[0]), int(stats.shape[1]), (int(stats.shape[2]) - 1) // 2, stats.device
    cnt = np.asarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts).astype(np.int64)
    if cnt.shape != (ns,) or (cnt < 0).any():
        raise ValueError("%s: counts must be %d non-negative integers" % (who, ns))
    w, mu, var = (t.to(device=dev, dtype=torch.float64).contiguous() if isinstance(t, torch.Tensor) else dev64(t, dev)
                  for t in (weights, means, variances))
    if tuple(w.shape) != (k,) or tuple(mu.shape) != (k, d) or tuple(var.shape) != (k, d):
        raise ValueError("%s: weights [%d], means [%d,%d], variances [%d,%d] expected" % (who, k, k, d, k, d))
    cntd = torch.as_tensor(cnt).to(dev)
    out = torch.empty((ns, k + 2 * k * d), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_fisher_encode(_ffi.ctx(dev.index), _ffi.ptr(stats), _ffi.ptr(cntd), ns, k, d, _ffi.ptr(w), _ffi.ptr(mu),
                                               _ffi.ptr(var), float(power), _ffi.ptr(out), _ffi.stream_ptr(dev)))
    return out


def fisher_vectors(x, segments, gmm, power=0.0, chunk_rows=None, batch_rows=None):
    """One Fisher vector per segment (video): x CUDA float32 ``[n,D]``, ``segments [n_segments + 1]`` ascending row offsets
    from 0 to n (an empty segment gives a zero vector), ``gmm`` a ``GMMModel``.  -> CUDA float32 ``[n_segments, K + 2KD]``
    in Sheet02's order (alpha | mu block, row-major [K,D] | sigma block; Sheet02.py:611-615), divided by the segment's row
    count, signed-power normalised when ``power > 0`` (0: none, as Sheet02; 0.5: the improved Fisher vector), then divided by
    its L2 norm unless that is below ``EPSILON``.  One ``va_gmm_stats`` call and one ``va_fisher_encode`` call cover all
    segments."""
    who = "fisher_vectors"
    x = check_rows(x, who, MAX_GMM_DIM)
    if not isinstance(gmm, GMMModel):
        raise ValueError("%s: gmm must be a GMMModel" % who)
    if isinstance(power, bool) or not isinstance(power, (int, float, np.integer, np.floating)) or not 0.0 <= power <= 1.0:
        raise ValueError("%s: power must be a number in [0, 1], got %r" % (who, power))
    n, d, k = int(x.shape[0]), int(x.shape[1]), len(gmm.weights)
    if d != gmm.means.shape[1]:
        raise ValueError("%s: x has %d columns, the mixture %d" % (who, d, gmm.means.shape[1]))
    seg = check_segments(segments, n, who)
    if n == 0:
        return torch.zeros((len(seg) - 1, k + 2 * k * d), dtype=torch.float32, device=x.device)
    stats, _ll = gmm_stats(x, seg, gmm.weights, gmm.means, gmm.variances, "soft", chunk_rows, batch_rows)
    return fisher_encode(stats, np.diff(seg), gmm.weights, gmm.means, gmm.variances, power)
