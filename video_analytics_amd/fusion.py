"""Video-level aggregation and two-stream fusion on the device.

``DescriptorMeters`` is the bank of per-video ``AverageMeter`` objects that ``validate()`` fills
(Sheet03/utils.py:154-171, Sheet03/spatialModel.py:223-228), kept in HBM so that the batch loop
needs no device-to-host copy; ``linear_svm_predict`` is ``LinearSVC.predict`` of the fusion step
(Sheet03/combinedModel.py:38) on the joined descriptors.  ``score_consensus`` and ``fuse_scores`` are the video-level
half of the papers' test protocol (Sheet03/notes.txt:113-116, 121-124, 225-230): the class scores of a
video's snippets and views averaged, then the two streams' scores fused by a weighted average (``fuse_scores_n``: any
number of streams up to eight).
"""
import ctypes

import numpy as np
import torch

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
