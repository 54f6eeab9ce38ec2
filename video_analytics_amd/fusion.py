"""Video-level aggregation and two-stream fusion on the device.

``DescriptorMeters`` is the bank of per-video ``AverageMeter`` objects that ``validate()`` fills
(Sheet03/utils.py:154-171, Sheet03/spatialModel.py:223-228), kept in HBM so that the batch loop
needs no device-to-host copy; ``linear_svm_predict`` is ``LinearSVC.predict`` of the fusion step
(Sheet03/combinedModel.py:38) on the joined descriptors.  ``score_consensus`` and ``fuse_scores`` are the video-level
half of the papers' test protocol (Sheet03/notes.txt:113-116, 121-124, 225-230): the class scores of a
video's snippets and views averaged, then the two streams' scores fused by a weighted average (``fuse_scores_n``: any
number of streams up to eight).  ``linear_svm_fit`` is ``LinearSVC().fit`` of the same step
(Sheet03/combinedModel.py:34-35) as a float64 Newton-CG on the device.
"""
import ctypes
import warnings

import numpy as np
import torch

from . import _features
from . import _ffi


class _MeterView(object):
    """What ``saveVideoDescriptors`` and the reference code read from an AverageMeter: avg/sum/count/val."""

    def __init__(self, avg, total, count):
        self.avg = avg
        self.sum = total
        self.count = count
        self.val = None


class DescriptorMeters(object):
    """``update(desc, names, labels)`` per batch; ``as_dict()`` -> {videoName: (meter, label)} in first-seen
    order, the shape of the reference's ``testDict`` (Sheet03/spatialModel.py:131-132,223-228)."""

    def __init__(self, dim, device, capacity=1024):
        self.dim = int(dim)
        self.device = torch.device(device)
        self.slots = {}   # videoName -> slot
        self.labels = []  # slot -> label
        self._alloc(capacity)

    def _alloc(self, capacity):
        sums = torch.zeros((capacity, self.dim), dtype=torch.float32, device=self.device)
        counts = torch.zeros((capacity,), dtype=torch.int32, device=self.device)
        if getattr(self, "sums", None) is not None:
            n = self.sums.shape[0]
            sums[:n] = self.sums
            counts[:n] = self.counts
        self.sums, self.counts = sums, counts

    def __len__(self):
        return len(self.slots)

    def update(self, desc, names, labels):
        if not isinstance(desc, torch.Tensor) or not desc.is_cuda or desc.dtype != torch.float32:
            raise ValueError("DescriptorMeters.update: desc must be a CUDA float32 tensor")
        if desc.device != self.device:
            raise ValueError("DescriptorMeters.update: desc is on %s, the meters on %s" % (desc.device, self.device))
        if desc.dim() != 2 or desc.shape[1] != self.dim or desc.shape[0] != len(names):
            raise ValueError("DescriptorMeters.update: desc must be [len(names), %d]" % self.dim)
        idx = []
        for i, name in enumerate(names):
            s = self.slots.get(name)
            if s is None:
                s = self.slots[name] = len(self.labels)
                self.labels.append(labels[i])
            idx.append(s)
        if len(self.labels) > self.sums.shape[0]:
            self._alloc(max(2 * self.sums.shape[0], len(self.labels)))
        slot = torch.tensor(idx, dtype=torch.int32).to(self.device, non_blocking=True)
        desc = desc.contiguous()
        _ffi.check(_ffi.lib().va_meter_update(_ffi.ctx(self.device.index), _ffi.ptr(desc), _ffi.ptr(slot), desc.shape[0], self.dim,
                                              _ffi.ptr(self.sums), _ffi.ptr(self.counts), self.sums.shape[0], _ffi.stream_ptr(self.device)))

    def average(self):
        """-> float32 [n_videos, dim] on the device (AverageMeter.avg of every video, first-seen order)."""
        n = len(self.labels)
        avg = torch.empty((max(n, 1), self.dim), dtype=torch.float32, device=self.device)
        if n:
            _ffi.check(_ffi.lib().va_meter_average(_ffi.ctx(self.device.index), _ffi.ptr(self.sums), _ffi.ptr(self.counts), n, self.dim,
                                                   _ffi.ptr(avg), _ffi.stream_ptr(self.device)))
        return avg[:n]

    def as_dict(self):
        n = len(self.labels)
        avg = self.average().cpu()
        sums = self.sums[:n].cpu()
        counts = self.counts[:n].cpu().tolist()
        out = {}
        for name, s in self.slots.items():
            out[name] = (_MeterView(avg[s], sums[s], counts[s]), self.labels[s])
        return out


CONSENSUS_MODES = ("softmax", "logits")


def check_consensus(mode, who):
    if not isinstance(mode, str) or mode not in CONSENSUS_MODES:
        raise ValueError("%s: consensus must be one of %s, got %r" % (who, ", ".join(CONSENSUS_MODES), mode))
    return CONSENSUS_MODES.index(mode)


def check_fusion_weights(weights, who):
    """-> (wa, wb) as floats; ValueError unless both are finite, >= 0 and their sum is > 0."""
    try:
        wa, wb = (float(w) for w in weights)
    except (TypeError, ValueError):
        raise ValueError("%s: fusion weights must be two numbers (spatial, temporal), got %r" % (who, weights))
    if not (np.isfinite(wa) and np.isfinite(wb)) or wa < 0 or wb < 0 or wa + wb <= 0:
        raise ValueError("%s: fusion weights must be >= 0 with a positive sum, got (%g, %g)" % (who, wa, wb))
    return wa, wb


def score_consensus(logits, mode="softmax"):
    """The video score from the class logits of its items (``va_score_consensus``): logits CUDA float32
    ``[N,k,C]`` -- or ``[N,n,V,C]``, snippets x views, read snippet-major -- -> ``[N,C]`` float32.

    ``"softmax"`` (Simonyan and Zisserman's testing): the softmax of every item, then their mean in item order;
    ``"logits"`` (TSN's consensus, then the prediction function): the mean of the logits in item order, then one softmax."""
    m = check_consensus(mode, "score_consensus")
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() not in (3, 4):
        raise ValueError("score_consensus: logits must be a CUDA float32 [N,k,C] or [N,n,V,C] tensor")
    N, C = int(logits.shape[0]), int(logits.shape[-1])
    k = logits.numel() // max(1, N * C)
    if N < 1 or k < 1 or C < 1:
        raise ValueError("score_consensus: empty logits %s" % (tuple(logits.shape),))
    logits = logits.contiguous()
    scores = torch.empty((N, C), dtype=torch.float32, device=logits.device)
    _ffi.check(_ffi.lib().va_score_consensus(_ffi.ctx(logits.device.index), _ffi.ptr(logits), N, k, C, m, _ffi.ptr(scores),
                                             _ffi.stream_ptr(logits.device)))
    return scores


def fuse_scores(a, b, weights=(1.0, 1.0)):
    """Two-stream fusion by weighted averaging (``va_fuse_scores``): a, b CUDA float32 ``[N,C]`` ->
    ``(fused [N,C] float32, pred [N] int32)``, ``fused = (wa*a + wb*b) / (wa + wb)`` and ``pred`` its arg-max with the
    first maximum winning.  ``(1, 1)`` is the two-stream paper's averaging, ``(1, 1.5)`` TSN's spatial : temporal weights."""
    wa, wb = check_fusion_weights(weights, "fuse_scores")
    for t in (a, b):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError("fuse_scores: a and b must be CUDA float32 [N,C] tensors")
    if a.shape != b.shape or a.device != b.device or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("fuse_scores: a %s and b %s must have one non-empty shape on one device" % (tuple(a.shape), tuple(b.shape)))
    a, b = a.contiguous(), b.contiguous()
    N, C = int(a.shape[0]), int(a.shape[1])
    fused = torch.empty((N, C), dtype=torch.float32, device=a.device)
    pred = torch.empty((N,), dtype=torch.int32, device=a.device)
    _ffi.check(_ffi.lib().va_fuse_scores(_ffi.ctx(a.device.index), _ffi.ptr(a), _ffi.ptr(b), N, C, wa, wb, _ffi.ptr(fused),
                                         _ffi.ptr(pred), _ffi.stream_ptr(a.device)))
    return fused, pred


def check_fusion_weights_n(weights, m, who):
    """-> the m weights as a tuple of floats; ValueError unless there are exactly ``m`` (2..8) of them, each finite (as a
    float32 too) and >= 0, with a positive sum."""
    m = int(m)
    if m < 2 or m > 8:
        raise ValueError("%s: fusion takes 2..8 streams, got %d" % (who, m))
    try:
        ws = tuple(float(w) for w in weights)
    except (TypeError, ValueError):
        raise ValueError("%s: fusion weights must be %d numbers, got %r" % (who, m, weights))
    if len(ws) != m:
        raise ValueError("%s: %d fusion weights for %d streams" % (who, len(ws), m))
    with np.errstate(over="ignore"):
        w32 = np.asarray(ws, dtype=np.float32)
        total = np.float32(0.0)
        for w in w32:
            total = np.float32(total + w)
    if not np.isfinite(w32).all() or (w32 < 0).any() or not np.isfinite(total) or not sum(ws) > 0 or not total > 0:
        raise ValueError("%s: fusion weights must be finite and >= 0 with a positive sum, got %r" % (who, ws))
    return ws


def fuse_scores_n(scores, weights=None):
    """Fusion of m streams by weighted averaging (``va_fuse_scores_n``): scores a list of m (2..8) CUDA
    float32 ``[N,C]`` tensors, ``weights`` m numbers (None: all ones) -> ``(fused [N,C] float32, pred [N] int32)``,
    ``fused = (((w0*a0 + w1*a1) + w2*a2) + ...) / (((w0 + w1) + w2) + ...)`` with every operation rounded to float32 in
    stream order, and ``pred`` its arg-max with the first maximum winning.  m = 2 gives ``fuse_scores``' bits."""
    if not isinstance(scores, (tuple, list)):
        raise ValueError("fuse_scores_n: scores must be a list of CUDA float32 [N,C] tensors")
    m = len(scores)
    ws = check_fusion_weights_n((1.0,) * m if weights is None else weights, m, "fuse_scores_n")
    for t in scores:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError("fuse_scores_n: scores must be CUDA float32 [N,C] tensors")
    a = scores[0]
    if any(t.shape != a.shape or t.device != a.device for t in scores) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("fuse_scores_n: the scores must have one non-empty shape on one device")
    scores = [t.contiguous() for t in scores]
    N, C = int(a.shape[0]), int(a.shape[1])
    fused = torch.empty((N, C), dtype=torch.float32, device=a.device)
    pred = torch.empty((N,), dtype=torch.int32, device=a.device)
    ptrs = (ctypes.c_void_p * m)(*[t.data_ptr() for t in scores])
    cw = (ctypes.c_float * m)(*ws)
    _ffi.check(_ffi.lib().va_fuse_scores_n(_ffi.ctx(a.device.index), ptrs, cw, m, N, C, _ffi.ptr(fused), _ffi.ptr(pred),
                                           _ffi.stream_ptr(a.device)))
    return fused, pred


def linear_svm_predict(descriptors, coef, intercept, classes, device=None, return_scores=False):
    """``LinearSVC.predict`` (Sheet03/combinedModel.py:38): classes[argmax(X coef^T + intercept)]; a single
    coefficient row is sklearn's binary problem (classes[score > 0]).  Inputs: array-likes (float64).

    Any ``dim``: the reference's use is the joined descriptors ``[N,512]`` of ``combineDescriptors``
    (``video.evaluateVideos`` returns them for whole videos); fusion by an SVM on the streams' scores
    (Sheet03/notes.txt:124) is the same call on the stacked scores ``[N,2C]``, ``concatenate([scores_s, scores_t], 1)``."""
    if not torch.cuda.is_available():
        raise RuntimeError("linear_svm_predict: no GPU visible; the hot path has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    x = torch.as_tensor(np.ascontiguousarray(np.asarray(descriptors, dtype=np.float64))).to(dev)
    w = torch.as_tensor(np.ascontiguousarray(np.atleast_2d(np.asarray(coef, dtype=np.float64)))).to(dev)
    b = torch.as_tensor(np.ascontiguousarray(np.atleast_1d(np.asarray(intercept, dtype=np.float64)))).to(dev)
    classes = np.asarray(classes)
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1] or b.shape[0] != w.shape[0]:
        raise ValueError("linear_svm_predict: shapes X[n,d], coef[c,d], intercept[c] expected, got %s %s %s"
                         % (tuple(x.shape), tuple(w.shape), tuple(b.shape)))
    if len(classes) != (2 if w.shape[0] == 1 else w.shape[0]):
        raise ValueError("linear_svm_predict: %d classes for %d coefficient rows" % (len(classes), w.shape[0]))
    n, c = x.shape[0], w.shape[0]
    scores = torch.empty((n, c), dtype=torch.float64, device=dev)
    pred = torch.empty((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(_ffi.lib().va_linear_svm_predict(_ffi.ctx(dev.index), _ffi.ptr(x), n, x.shape[1], _ffi.ptr(w), _ffi.ptr(b), c,
                                                    _ffi.ptr(scores), _ffi.ptr(pred), _ffi.stream_ptr(dev)))
    out = classes[pred.cpu().numpy()]
    return (out, scores.cpu().numpy()) if return_scores else out


SVM_FIT_NEWTON_CHUNK = 4  # Newton steps enqueued between two reads of the solver's statistics


def check_svm_fit_args(descriptors, labels, C=1.0, tol=1e-8, max_iter=100, fit_intercept=True, intercept_scaling=1.0):
    """The argument check of ``linear_svm_fit``, on the host alone (no GPU needed): ValueError for descriptors that are not
    2-D ``[n >= 2, 1 <= d <= 8192]`` or hold non-finite values, labels of another length, fewer than two (or more than 4096)
    distinct labels, and C, tol, max_iter or intercept_scaling out of range.  -> ``(classes, y)``: ``np.unique(labels)`` and
    every label's index into it as int32."""
    who = "linear_svm_fit"
    for name, v, positive in (("C", C, True), ("tol", tol, True), ("intercept_scaling", intercept_scaling, bool(fit_intercept))):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) \
                or (v <= 0 if positive else v < 0):
            raise ValueError("%s: %s must be a finite number %s 0, got %r" % (who, name, ">" if positive else ">=", v))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError("%s: max_iter must be an integer >= 1 (Newton steps), got %r" % (who, max_iter))
    if isinstance(descriptors, torch.Tensor):
        if descriptors.dtype not in (torch.float32, torch.float64):
            raise ValueError("%s: a descriptor tensor must be float32 or float64, got %s" % (who, descriptors.dtype))
        shape = tuple(descriptors.shape)
    else:
        try:
            descriptors = np.asarray(descriptors, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("%s: descriptors must be numbers [n, d]" % who)
        shape = descriptors.shape
    if len(shape) != 2:
        raise ValueError("%s: descriptors must be 2-D [n, d], got shape %s" % (who, tuple(shape)))
    n, d = int(shape[0]), int(shape[1])
    if n < 2 or d < 1 or d > 8192:
        raise ValueError("%s: need n >= 2 rows and 1 <= d <= 8192 columns, got [%d, %d]" % (who, n, d))
    finite = bool(torch.isfinite(descriptors).all()) if isinstance(descriptors, torch.Tensor) else bool(np.isfinite(descriptors).all())
    if not finite:
        raise ValueError("%s: descriptors hold non-finite values" % who)
    labels = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
    if labels.ndim != 1 or labels.shape[0] != n:
        raise ValueError("%s: %d descriptors but labels of shape %s" % (who, n, tuple(labels.shape)))
    if labels.dtype.kind == "f" and not np.isfinite(labels).all():
        raise ValueError("%s: labels hold non-finite values" % who)
    classes, y = np.unique(labels, return_inverse=True)
    if len(classes) < 2 or len(classes) > 4096:
        raise ValueError("%s: need 2 .. 4096 distinct labels, got %d" % (who, len(classes)))
    return classes, np.ascontiguousarray(y.reshape(-1), dtype=np.int32)


def linear_svm_fit(descriptors, labels, C=1.0, tol=1e-8, max_iter=100, fit_intercept=True, intercept_scaling=1.0, device=None,
                   return_info=False):
    """``LinearSVC().fit`` (Sheet03/combinedModel.py:34-35) on the device: ``va_linear_svm_fit``, DESIGN.md S27 and S28.

    The problem is ``LinearSVC``'s with its defaults, liblinear's L2R_L2LOSS_SVC one-vs-rest: row r minimises
    ``1/2 |w|^2 + C sum_i max(0, 1 - y_i w.[x_i, s])^2`` with ``y_i = +1`` where ``labels[i] == classes[r]``, else ``-1``,
    and ``s = intercept_scaling`` (the bias is regularised, as in liblinear); ``coef[r] = w[:d]``, ``intercept[r] = s w[d]``.
    The objective is strongly convex, so the optimum is liblinear's; the solver is a float64 Newton-CG over all rows at once
    and a row stops when ``|grad f_r(w)| <= tol |grad f_r(0)|``.  Two calls give the same bits.

    ``descriptors``: an array-like ``[n, d]``, or a CUDA float32 / float64 tensor (float32 is widened on the device: what
    ``video.evaluateVideos`` returns never visits the host); ``labels``: ``[n]``.  -> ``(coef [rows, d] f64, intercept [rows]
    f64, classes)`` as numpy, ready for ``linear_svm_predict``; ``classes = np.unique(labels)``, and two classes give ONE
    row, for ``classes[1]`` (sklearn's convention).  ``return_info=True`` adds ``{"n_iter", "rel_grad" [rows], "objective"
    [rows], "converged", "steps" [rows], "cg_steps" [rows]}`` (Newton and CG steps of every row).  ``max_iter`` counts Newton steps; reaching it with a row not converged is a
    ``RuntimeWarning`` and the iterate is returned.  ``fit_intercept=False``: no bias, ``intercept == 0``.

    Fusion by an SVM on the streams' scores (Sheet03/notes.txt:124) is the same call on the stacked scores ``[N, 2C]``,
    as for ``linear_svm_predict``.  Not offered: the hinge (L1) loss, the L1 penalty, Crammer-Singer, class or sample
    weights, sparse input."""
    classes, y = check_svm_fit_args(descriptors, labels, C, tol, max_iter, fit_intercept, intercept_scaling)
    if not torch.cuda.is_available():
        raise RuntimeError("linear_svm_fit: no GPU visible; the hot path has no CPU fallback")
    if isinstance(descriptors, torch.Tensor) and descriptors.is_cuda:
        dev = descriptors.device if device is None else torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        x = descriptors.to(device=dev, dtype=torch.float64).contiguous()
    else:
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        src = descriptors.to(torch.float64).numpy() if isinstance(descriptors, torch.Tensor) else np.asarray(descriptors, dtype=np.float64)
        x = torch.as_tensor(np.ascontiguousarray(src)).to(dev)
    n, d = int(x.shape[0]), int(x.shape[1])
    rows = 1 if len(classes) == 2 else len(classes)
    scale = float(intercept_scaling) if fit_intercept else 0.0
    L = _ffi.lib()
    work = _features.workspace(L.va_linear_svm_fit_workspace_bytes(n, d, rows), dev)
    need = work.numel()
    yd = torch.as_tensor(y).to(dev)
    coef = torch.empty((rows, d), dtype=torch.float64, device=dev)
    intercept = torch.empty((rows,), dtype=torch.float64, device=dev)
    stats = torch.empty((rows, 4), dtype=torch.float64, device=dev)
    enqueued, restart = 0, 1
    with torch.cuda.device(dev):
        while True:
            steps = min(int(SVM_FIT_NEWTON_CHUNK), int(max_iter) - enqueued)
            _ffi.check(L.va_linear_svm_fit(_ffi.ctx(dev.index), _ffi.ptr(x), _ffi.ptr(yd), n, d, len(classes), float(C), scale, float(tol),
                                           steps, restart, _ffi.ptr(coef), _ffi.ptr(intercept), _ffi.ptr(stats), _ffi.ptr(work), need,
                                           _ffi.stream_ptr(dev)))
            enqueued, restart = enqueued + steps, 0
            st = stats.cpu().numpy()  # the one synchronisation of a round
            converged = bool((st[:, 1] <= float(tol) * st[:, 2]).all())
            if converged or enqueued >= int(max_iter):
                break
    if not converged:
        warnings.warn("linear_svm_fit: %d of %d class rows not converged after max_iter = %d Newton steps"
                      % (int((st[:, 1] > float(tol) * st[:, 2]).sum()), rows, int(max_iter)), RuntimeWarning)
    out = (coef.cpu().numpy(), intercept.cpu().numpy(), classes)
    if not return_info:
        return out
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(st[:, 2] > 0, st[:, 1] / st[:, 2], 0.0)
    cg = torch.empty((rows,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _ffi.check(L.va_linear_svm_fit_cg_steps(_ffi.ctx(dev.index), n, d, rows, _ffi.ptr(work), need, _ffi.ptr(cg), _ffi.stream_ptr(dev)))
    info = {"n_iter": int(st[:, 3].max()), "rel_grad": rel, "objective": st[:, 0].copy(), "converged": converged,
            "steps": st[:, 3].astype(np.int64), "cg_steps": cg.cpu().numpy().astype(np.int64)}
    return out + (info,)
