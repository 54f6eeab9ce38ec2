"""Bag of words on MI355X (``csrc/codebook.hip``): the part of the modelled project's Sheet01 between the
interest-point descriptors and the linear SVM -- ``makeCodebook`` (Sheet01.py:259-264, ``KMeans(n_clusters=256,
random_state=0)``) and ``makeVideoHistogram`` (Sheet01.py:267-277).

The descriptors are CUDA float32 tensors (what ``stip.space_time_interest_points`` returns as ``desc``); the centres are
float64 and every sum is float64 in a fixed order, so two calls give the same bits.  Seeding, assignment, update and
histograms are HIP; nothing of size ``n x K`` exists.  No part of this module needs scikit-learn.

Where it departs from scikit-learn, deliberately: the seeding is plain k-means++ with one trial per centre (sklearn's is the
greedy variant with ``2 + log K`` trials), an empty cluster keeps its centre (sklearn moves it to the row farthest from its
centre) and ``n_init`` defaults to 1 (Sheet01's era of sklearn ran 10).  A fit from a given ``init`` on which no cluster
empties follows sklearn's Lloyd iterations to rounding.
"""
import ctypes

import numpy as np
import torch

from . import _ffi
from . import fisher
from ._features import check_rows, check_segments, dev64, workspace

MAX_DIM, MAX_CLUSTERS, MAX_SEGMENTS = 512, 4096, 65536
NORMS = {"none": _ffi.VA_BOW_NONE, "l1": _ffi.VA_BOW_L1, "l2": _ffi.VA_BOW_L2}


def _centres(centres, d, dev, who):
    c = centres.to(device=dev, dtype=torch.float64).contiguous() if isinstance(centres, torch.Tensor) else dev64(centres, dev)
    if c.dim() != 2 or c.shape[1] != d or not 1 <= c.shape[0] <= MAX_CLUSTERS:
        raise ValueError("%s: centres must be [K, %d] with 1 <= K <= %d, got %s" % (who, d, MAX_CLUSTERS, tuple(c.shape)))
    return c


def _workspace(n, d, k, n_segments, dev, params=None):
    ws = workspace(_ffi.lib().va_kmeans_workspace_bytes(n, d, k, n_segments, None if params is None else ctypes.byref(params)), dev)
    return ws, ws.numel()


def _norm(norm, who):
    if norm not in NORMS:
        raise ValueError("%s: norm must be 'l2', 'l1' or 'none', got %r" % (who, norm))
    return NORMS[norm]


def assign(x, centres, prev_labels=None, want_d2=True):
    """``va_kmeans_assign``: x CUDA float32 ``[n,d]`` (n >= 1, d <= 512), centres float64 ``[K,d]`` (K <= 4096).  ->
    ``(labels int32 [n], d2 float64 [n] or None, inertia float64 [1], changed int64 [1])``, all CUDA: the lowest nearest
    centre of each row, its squared distance, their sum, and the rows whose label differs from ``prev_labels`` (all rows when
    that is None)."""
    who = "assign"
    x = check_rows(x, who, MAX_DIM)
    n, d, dev = int(x.shape[0]), int(x.shape[1]), x.device
    if n < 1:
        raise ValueError("%s: x holds no rows" % who)
    c = _centres(centres, d, dev, who)
    k = int(c.shape[0])
    if prev_labels is not None and (not isinstance(prev_labels, torch.Tensor) or prev_labels.device != dev
                                    or prev_labels.dtype != torch.int32 or tuple(prev_labels.shape) != (n,)):
        raise ValueError("%s: prev_labels must be an int32 [%d] tensor on x's device" % (who, n))
    ws, need = _workspace(n, d, k, 1, dev)
    labels = torch.empty((n,), dtype=torch.int32, device=dev)
    d2 = torch.empty((n,), dtype=torch.float64, device=dev) if want_d2 else None
    inertia = torch.empty((1,), dtype=torch.float64, device=dev)
    changed = torch.empty((1,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_kmeans_assign(_ffi.ctx(dev.index), _ffi.ptr(x), n, d, _ffi.ptr(c), k,
                                               _ffi.ptr(None if prev_labels is None else prev_labels.contiguous()), _ffi.ptr(labels),
                                               _ffi.ptr(d2), _ffi.ptr(inertia), _ffi.ptr(changed), _ffi.ptr(ws), need, _ffi.stream_ptr(dev)))
    return labels, d2, inertia, changed


def update(x, labels, centres, chunk_rows=None):
    """``va_kmeans_update``: -> ``(counts int64 [K], new centres float64 [K,d], shift2 float64 [1])``, all CUDA.  A cluster's
    centre is the mean of its rows, added in a fixed tree over the rows in ascending order; an empty cluster keeps its centre;
    ``shift2 = sum_j |new_j - old_j|^2``.  ``chunk_rows`` sizes the counting sort's chunks and reaches no result."""
    who = "update"
    x = check_rows(x, who, MAX_DIM)
    n, d, dev = int(x.shape[0]), int(x.shape[1]), x.device
    if n < 1:
        raise ValueError("%s: x holds no rows" % who)
    c = _centres(centres, d, dev, who)
    k = int(c.shape[0])
    if not isinstance(labels, torch.Tensor) or labels.device != dev or labels.dtype != torch.int32 or tuple(labels.shape) != (n,):
        raise ValueError("%s: labels must be an int32 [%d] tensor on x's device" % (who, n))
    p = _ffi.default_kmeans_params(**({} if chunk_rows is None else {"chunk_rows": int(chunk_rows)}))
    ws, need = _workspace(n, d, k, 1, dev, p)
    counts = torch.empty((k,), dtype=torch.int64, device=dev)
    new = torch.empty((k, d), dtype=torch.float64, device=dev)
    shift2 = torch.empty((1,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_kmeans_update(_ffi.ctx(dev.index), _ffi.ptr(x), n, d, _ffi.ptr(labels.contiguous()), _ffi.ptr(c), k,
                                               ctypes.byref(p), _ffi.ptr(counts), _ffi.ptr(new), _ffi.ptr(shift2), _ffi.ptr(ws), need,
                                               _ffi.stream_ptr(dev)))
    return counts, new, shift2


def seed(x, n_clusters, u):
    """``va_kmeans_seed``: plain k-means++ from ``u`` float64 ``[K]`` in [0, 1).  -> ``(centres float64 [K,d], rows int32 [K],
    m float64 [n])``, all CUDA: the chosen rows widened, their indices and each row's squared distance to the nearest of the
    centres chosen before the last."""
    who = "seed"
    x = check_rows(x, who, MAX_DIM)
    n, d, dev, k = int(x.shape[0]), int(x.shape[1]), x.device, int(n_clusters)
    if n < 1:
        raise ValueError("%s: x holds no rows" % who)
    u = np.ascontiguousarray(np.asarray(u, dtype=np.float64))
    if u.shape != (k,) or not ((u >= 0) & (u < 1)).all():
        raise ValueError("%s: u must hold %d numbers in [0, 1)" % (who, k))
    ws, need = _workspace(n, d, k, 1, dev)
    ud = torch.as_tensor(u).to(dev)
    centres = torch.empty((k, d), dtype=torch.float64, device=dev)
    rows = torch.empty((k,), dtype=torch.int32, device=dev)
    m = torch.empty((n,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_kmeans_seed(_ffi.ctx(dev.index), _ffi.ptr(x), n, d, _ffi.ptr(ud), k, _ffi.ptr(centres), _ffi.ptr(rows),
                                             _ffi.ptr(m), _ffi.ptr(ws), need, _ffi.stream_ptr(dev)))
    return centres, rows, m


def bow_histograms(labels, segments, n_words, norm="l2"):
    """``va_bow_histograms``: labels CUDA int32 ``[n]``, ``segments [S + 1]`` ascending from 0 to n.  -> CUDA float32
    ``[S, n_words]``; an empty segment gives zeros."""
    who = "bow_histograms"
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda or labels.dtype != torch.int32 or labels.dim() != 1:
        raise ValueError("%s: labels must be a CUDA int32 [n] tensor" % who)
    mode, n, dev, k = _norm(norm, who), int(labels.shape[0]), labels.device, int(n_words)
    seg = check_segments(segments, n, who)
    ns = len(seg) - 1
    if not 1 <= k <= MAX_CLUSTERS or ns > MAX_SEGMENTS:
        raise ValueError("%s: need 1 <= n_words <= %d and at most %d segments, got %d and %d" % (who, MAX_CLUSTERS, MAX_SEGMENTS, k, ns))
    if n == 0:
        return torch.zeros((ns, k), dtype=torch.float32, device=dev)
    segd = torch.as_tensor(seg).to(dev)
    out = torch.empty((ns, k), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_bow_histograms(_ffi.ctx(dev.index), _ffi.ptr(labels.contiguous()), n, _ffi.ptr(segd), ns, k, mode,
                                                _ffi.ptr(out), _ffi.stream_ptr(dev)))
    return out


def bow_encode(x, segments, centres, norm="l2"):
    """``va_bow_encode``: assignment and histograms in one call; the labels live in the workspace and no ``d2`` exists."""
    who = "bow_encode"
    x = check_rows(x, who, MAX_DIM)
    mode, n, d, dev = _norm(norm, who), int(x.shape[0]), int(x.shape[1]), x.device
    c = _centres(centres, d, dev, who)
    k = int(c.shape[0])
    seg = check_segments(segments, n, who)
    ns = len(seg) - 1
    if ns > MAX_SEGMENTS:
        raise ValueError("%s: at most %d segments, got %d" % (who, MAX_SEGMENTS, ns))
    if n == 0:
        return torch.zeros((ns, k), dtype=torch.float32, device=dev)
    ws, need = _workspace(n, d, k, ns, dev)
    segd = torch.as_tensor(seg).to(dev)
    out = torch.empty((ns, k), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_bow_encode(_ffi.ctx(dev.index), _ffi.ptr(x), n, d, _ffi.ptr(c), k, _ffi.ptr(segd), ns, mode, _ffi.ptr(out),
                                            _ffi.ptr(ws), need, _ffi.stream_ptr(dev)))
    return out


class Codebook(object):
    """What ``kmeans_fit`` returns: ``centres [K,d]`` (float64 numpy), ``inertia`` (the sum of the squared distances of the
    final assignment), ``n_iter``, ``converged`` and ``counts [K]`` (int64; a zero is a cluster that emptied and kept its
    centre)."""

    def __init__(self, centres, inertia=float("nan"), n_iter=0, converged=False, counts=None):
        self.centres = np.ascontiguousarray(centres, dtype=np.float64)
        if self.centres.ndim != 2 or not 1 <= self.centres.shape[0] <= MAX_CLUSTERS or not 1 <= self.centres.shape[1] <= MAX_DIM:
            raise ValueError("Codebook: centres must be [K, d] with K <= %d and d <= %d, got %s"
                             % (MAX_CLUSTERS, MAX_DIM, self.centres.shape))
        self.inertia, self.n_iter, self.converged = float(inertia), int(n_iter), bool(converged)
        self.counts = np.zeros(len(self.centres), dtype=np.int64) if counts is None else np.ascontiguousarray(counts, dtype=np.int64)
        if self.counts.shape != (len(self.centres),):
            raise ValueError("Codebook: counts must be [K]")

    @property
    def n_words(self):
        return int(self.centres.shape[0])

    def assign(self, x):
        """-> the int32 CUDA labels of a CUDA float32 ``[n,d]`` tensor (an empty tensor gives an empty one)."""
        x = check_rows(x, "Codebook.assign", MAX_DIM)
        if x.shape[1] != self.centres.shape[1]:
            raise ValueError("Codebook.assign: x has %d columns, the codebook %d" % (x.shape[1], self.centres.shape[1]))
        if x.shape[0] == 0:
            return torch.empty((0,), dtype=torch.int32, device=x.device)
        return assign(x, self.centres, want_d2=False)[0]

    def histograms(self, x, segments, norm="l2"):
        """One histogram of words per segment (video): x CUDA float32 ``[n,d]``, ``segments [S + 1]`` ascending row offsets
        from 0 to n.  -> CUDA float32 ``[S, K]``: the counts divided by their L2 norm (``"l2"``, Sheet01's ``normalize``), their
        sum (``"l1"``) or nothing (``"none"``).  An empty segment gives zeros (Sheet01 would give NaN there)."""
        x = check_rows(x, "Codebook.histograms", MAX_DIM)
        if x.shape[1] != self.centres.shape[1]:
            raise ValueError("Codebook.histograms: x has %d columns, the codebook %d" % (x.shape[1], self.centres.shape[1]))
        return bow_encode(x, segments, self.centres, norm)

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, centres=self.centres, inertia=np.float64(self.inertia), n_iter=np.int64(self.n_iter),
                     converged=np.bool_(self.converged), counts=self.counts)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["centres"], float(z["inertia"]), int(z["n_iter"]), bool(z["converged"]), z["counts"])


def check_kmeans_fit_args(n, d, n_clusters, init, n_init, max_iter, tol, seed):
    """The argument checks of ``kmeans_fit`` that need no device: ValueError naming the argument."""
    who = "kmeans_fit"
    for name, v, lo in (("n_clusters", n_clusters, 1), ("n_init", n_init, 1), ("max_iter", max_iter, 1), ("seed", seed, 0)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError("%s: %s must be an integer >= %d, got %r" % (who, name, lo, v))
    if n_clusters > MAX_CLUSTERS:
        raise ValueError("%s: n_clusters must be <= %d, got %d" % (who, MAX_CLUSTERS, n_clusters))
    if seed + n_init - 1 > 2 ** 32 - 1:
        raise ValueError("%s: seed + n_init - 1 must fit numpy's RandomState (< 2^32), got seed %d" % (who, seed))
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not np.isfinite(tol) or tol < 0:
        raise ValueError("%s: tol must be a finite number >= 0, got %r" % (who, tol))
    if not 1 <= d <= MAX_DIM:
        raise ValueError("%s: x must have 1 .. %d columns, got %d" % (who, MAX_DIM, d))
    if n < n_clusters:
        raise ValueError("%s: n_clusters = %d exceeds the %d rows of x" % (who, n_clusters, n))
    if isinstance(init, str):
        if init not in ("k-means++", "random"):
            raise ValueError("%s: init must be 'k-means++', 'random' or a [K, d] array, got %r" % (who, init))
    else:
        try:
            a = np.asarray(init.cpu() if isinstance(init, torch.Tensor) else init, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("%s: init must be 'k-means++', 'random' or a [K, d] array, got %r" % (who, type(init)))
        if a.shape != (n_clusters, d) or not np.isfinite(a).all():
            raise ValueError("%s: init must be a finite [%d, %d] array, got shape %s" % (who, n_clusters, d, a.shape))


def tolerance(count, colsum, xtx, tol):
    """sklearn's scale of ``tol``: ``tol`` times the mean over the columns of their variance (``np.var``, ddof 0), from
    ``fisher.pca_moments``' count, column sums and ``X^T X``."""
    mean = np.asarray(colsum, dtype=np.float64) / count
    var = np.diag(np.asarray(xtx, dtype=np.float64)) / count - mean * mean
    return float(tol) * float(np.mean(np.maximum(var, 0.0)))


def lloyd_stop(it, changed, shift2, tol_scaled, max_iter):
    """The stopping rule after Lloyd step ``it`` (1-based): -> ``(stop, converged)``.  ``changed``: the rows whose label
    differs from the step before (None at the first step); ``shift2``: the summed squared movement of the centres."""
    if changed is not None and changed == 0:
        return True, True
    if shift2 <= tol_scaled:
        return True, True
    return it >= max_iter, False


def best_run(inertias):
    """The index of the lowest inertia, the first on ties (``n_init`` selection)."""
    best = 0
    for i, v in enumerate(inertias):
        if v < inertias[best]:
            best = i
    return best


def _one_fit(x, k, init, max_iter, tol_scaled, seed_value):
    n, dev = int(x.shape[0]), x.device
    if isinstance(init, str) and init == "k-means++":
        centres = seed(x, k, np.random.RandomState(seed_value).random_sample(k))[0]
    elif isinstance(init, str):
        rows = np.random.RandomState(seed_value).permutation(n)[:k]
        centres = x[torch.as_tensor(rows, device=dev)].to(torch.float64)
    else:
        centres = dev64(init.cpu().numpy() if isinstance(init, torch.Tensor) else init, dev)
    prev, n_iter, converged = None, 0, False
    for it in range(1, max_iter + 1):
        labels, _d2, _inertia, changed = assign(x, centres, prev, want_d2=False)
        n_iter = it
        moved = None if prev is None else int(changed.item())  # the first of the two values the host reads per iteration
        if moved == 0:  # the update would return these centres again, bit for bit
            converged = True
            break
        _counts, centres, shift2 = update(x, labels, centres)
        stop, converged = lloyd_stop(it, moved, float(shift2.item()), tol_scaled, max_iter)  # the second
        prev = labels
        if stop:
            break
    labels, _d2, inertia, _changed = assign(x, centres, None, want_d2=False)
    counts, _new, _shift2 = update(x, labels, centres)
    return Codebook(centres.cpu().numpy(), float(inertia.item()), n_iter, converged, counts.cpu().numpy())


def kmeans_fit(x, n_clusters=256, *, init="k-means++", n_init=1, max_iter=300, tol=1e-4, seed=0):
    """Lloyd's k-means on the device (Sheet01.py:259-264 with 256 clusters): x a CUDA float32 ``[n,d]`` tensor or a list of
    per-video tensors (empty ones are skipped), d <= 512, n_clusters <= min(n, 4096).  -> ``Codebook``.

    ``init``: ``"k-means++"`` (plain k-means++, one trial per centre, from ``RandomState(seed).random_sample(K)``; not
    sklearn's greedy variant), ``"random"`` (the rows ``RandomState(seed).permutation(n)[:K]``, as ``gmm_fit``) or a ``[K,d]``
    array.  A Lloyd step is one assignment and one update; the steps stop at the first of: no label changed since the step
    before; ``shift2 <= tol * mean_c Var(x_c)`` (sklearn's rule; the variance from ``fisher.pca_moments``); ``max_iter``
    steps.  A final assignment on the last centres gives ``inertia`` and ``counts``, as sklearn does.  The host reads two
    scalars per iteration.  ``n_init > 1`` repeats with seeds ``seed, seed + 1, ...`` and keeps the lowest inertia, the first
    on ties (with an array ``init`` every run is the same).

    An empty cluster keeps its centre (as ``gmm_fit``'s k-means does); sklearn relocates it instead.  ``counts`` shows
    empties to the caller."""
    who = "kmeans_fit"
    if isinstance(x, (list, tuple)):
        parts = [check_rows(p, who, MAX_DIM) for p in x]
        parts = [p for p in parts if p.shape[0] > 0]
        if not parts:
            raise ValueError("%s: x holds no rows" % who)
        if len(set((int(p.shape[1]), p.device) for p in parts)) != 1:
            raise ValueError("%s: x must share one width and one device" % who)
        x = torch.cat(parts, 0) if len(parts) > 1 else parts[0]
    x = check_rows(x, who, MAX_DIM)
    n, d = int(x.shape[0]), int(x.shape[1])
    check_kmeans_fit_args(n, d, n_clusters, init, n_init, max_iter, tol, seed)
    tol_scaled = tolerance(*fisher.pca_moments(x), tol=tol)
    runs = [_one_fit(x, int(n_clusters), init, int(max_iter), tol_scaled, int(seed) + r) for r in range(int(n_init))]
    return runs[best_run([r.inertia for r in runs])]
