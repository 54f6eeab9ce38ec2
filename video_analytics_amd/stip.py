"""Space-time interest points on MI355X (``va_stip_extract``): the detector and descriptors of the
modelled project's Sheet01 -- Laptev's Harris3D response at every pair of a spatial and a temporal scale, its strict local
maxima, and around each a cuboid of HOG / HOF histograms -- ending at the per-point descriptors ``[n, 144]``.

The flow comes from this library (Farneback with Sheet01's arguments by default, Sheet01.py:79) or from the caller.  It is
computed once on the input frames and shared by all scales.  ``StipClassifier`` carries the descriptors on to a class label:
the k-means codebook and the bag-of-words histograms of ``codebook`` (Sheet01.py:259-277) and a linear SVM (Sheet01.py:379-390).
"""
import ctypes

import numpy as np
import torch

from . import _features
from . import _ffi
from . import codebook as vcodebook
from . import fusion
from . import ksvm

# what the outputs sized for the proven bound may take when max_points is None
MEMORY_BUDGET_BYTES = 8 << 30


def descriptor_length(params):
    """HOG then HOF, ``bins`` values in each of the nx * ny * nt cells: 144 at the defaults"""
    return 2 * params.nx * params.ny * params.nt * params.bins


def point_bound(w, h, n_frames, params):
    """No video yields more: strict maxima along x cannot be adjacent and the faces never qualify, so a row holds at most
    ceil((w - 2) / 2) of them, and only the (h - 2)(T - 2) inner rows hold any, at each scale pair (S87)."""
    per_row = max((w - 2 + 1) // 2, 0)
    return per_row * max(h - 2, 0) * max(n_frames - 2, 0) * params.n_sigmas * params.n_taus


def space_time_interest_points(gray, flow=None, params=None, flow_params=None, max_points=None, **over):
    """gray: CUDA uint8 or float32 ``[T,H,W]`` in [0,255], T >= 2, H and W in [1,16384].

    ``flow``: None computes ``farneback_flow(gray, flow_params)`` (an ``_ffi.Tvl1Params`` or ``_ffi.BroxParams`` in
    ``flow_params`` selects those methods, as ``flow.tvl1_flow`` does everywhere); a CUDA float32 ``[T-1,2,H,W]`` tensor is
    used as it is.  ``params``: an ``_ffi.StipParams`` or keyword overrides (sigmas, taus, integration, k, min_response,
    cuboid, neighbours, nx, ny, nt, bins), not both.

    Returns a dict: ``desc`` float32 ``[n, 144]`` (HOG 72 | HOF 72 at the defaults), ``points`` int32 ``[n, 5]`` (x, y, t,
    sigma index, tau index), ``response`` float32 ``[n]``, all CUDA and in the order scale pair (sigma outer, tau inner), t,
    y, x; ``count``: n.  More than ``max_points`` raises ValueError stating the count found; nothing is cut short.  With
    ``max_points=None`` the outputs are sized for ``point_bound`` and the call raises ValueError when that does not fit
    ``MEMORY_BUDGET_BYTES``.  The inputs are left untouched.
    """
    who = "space_time_interest_points"
    gray, flow, p = _features.extraction_inputs(who, gray, flow, flow_params, params, over, _ffi.StipParams, _ffi.default_stip_params)
    T, H, W = gray.shape
    L = _ffi.lib()
    dim = descriptor_length(p)
    cap = _features.extraction_capacity(who, lambda: point_bound(W, H, T, p), (dim + 5 + 1) * 4, max_points, MEMORY_BUDGET_BYTES,
                                        "points", "max_points")
    dev = gray.device
    ws = _features.workspace(L.va_stip_workspace_bytes(W, H, T, cap, ctypes.byref(p)), dev)
    desc = torch.empty((cap, dim), dtype=torch.float32, device=dev)
    points = torch.empty((cap, 5), dtype=torch.int32, device=dev)
    response = torch.empty((cap,), dtype=torch.float32, device=dev)
    count = ctypes.c_int(0)
    _ffi.check(L.va_stip_extract(_ffi.ctx(dev.index), _ffi.ptr(gray), int(gray.dtype == torch.uint8), _ffi.ptr(flow), T, W, H,
                                 ctypes.byref(p), _ffi.ptr(points), _ffi.ptr(response), _ffi.ptr(desc), cap, ctypes.byref(count),
                                 _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(dev)))
    n = int(count.value)
    if n > cap:
        raise ValueError("%s: found %d points, more than max_points = %d" % (who, n, cap))
    return {"desc": desc[:n], "points": points[:n], "response": response[:n], "count": n}


class StipClassifier(object):
    """Sheet01's ``main()`` after the extraction (Sheet01.py:259-277, 379-390): a k-means codebook of all training
    descriptors, one histogram of words per video, a linear SVM on those -- or, with ``svm="chi2"``, the chi-square kernel SVM
    that Laptev's interest points are evaluated with (``ksvm``; ``norm="l1"`` is its usual companion).

    ``descs_per_video``: a list of CUDA float32 ``[n_i, d]`` tensors, one per video
    (``space_time_interest_points(...)["desc"]``); a video without points (``n_i = 0``) is legal and gets a zero histogram."""

    def __init__(self):
        self.codebook = self.coef = self.intercept = self.classes = self.kernel_svm = None
        self.norm = "l2"

    def fit(self, descs_per_video, labels, n_words=256, norm="l2", svm="linear", C=1.0, **kmeans_kw):
        """``codebook.kmeans_fit`` with ``n_words`` clusters (Sheet01.py:262) and ``kmeans_kw``, histograms with ``norm``
        (``"l2"``: Sheet01's ``normalize``), then ``svm="linear"``: ``fusion.linear_svm_fit`` (Sheet01's classifier), or
        ``svm="chi2"``: ``ksvm.KernelSvm("chi2", C)`` on the histograms as one channel normalised by its mean distance, which
        keeps the training histograms, the scale and ``dual_coef`` (``C`` is read by this route only; ``norm="l1"`` is the
        usual companion of the chi-square kernel).  -> self."""
        who = "StipClassifier.fit"
        if svm not in ("linear", "chi2"):
            raise ValueError("%s: svm must be 'linear' or 'chi2', got %r" % (who, svm))
        videos, segments = _features.check_videos(descs_per_video, who)
        if len(labels) != len(videos):
            raise ValueError("%s: %d videos but %d labels" % (who, len(videos), len(labels)))
        if norm not in vcodebook.NORMS:
            raise ValueError("%s: norm must be 'l2', 'l1' or 'none', got %r" % (who, norm))
        rows = torch.cat(videos, 0)
        self.codebook = vcodebook.kmeans_fit(rows, n_words, **kmeans_kw)
        self.norm = norm
        hist = self.codebook.histograms(rows, segments, norm)
        if svm == "linear":
            self.kernel_svm = None
            self.coef, self.intercept, self.classes = fusion.linear_svm_fit(hist, labels)
        else:
            self.kernel_svm = ksvm.KernelSvm("chi2", C).fit(hist, labels)
            self.coef, self.intercept, self.classes = None, self.kernel_svm.intercept, self.kernel_svm.classes
        return self

    def encode(self, descs_per_video):
        """The histograms CUDA float32 ``[n_videos, n_words]`` of the fitted codebook, for callers who fuse them elsewhere."""
        who = "StipClassifier.encode"
        if self.codebook is None:
            raise ValueError("%s: the model is not fitted" % who)
        videos, segments = _features.check_videos(descs_per_video, who)
        return self.codebook.histograms(torch.cat(videos, 0), segments, self.norm)

    def predict(self, descs_per_video):
        """-> the predicted labels, one per video (``fusion.linear_svm_predict`` on the histograms, or on their chi-square
        kernel against the training histograms)."""
        if self.classes is None:
            raise ValueError("StipClassifier.predict: the model is not fitted")
        h = self.encode(descs_per_video)
        if self.kernel_svm is not None:
            return self.kernel_svm.predict(h)
        return fusion.linear_svm_predict(h.double().cpu().numpy(), self.coef, self.intercept, self.classes, device=h.device.index)

    def save(self, path):
        if self.classes is None:
            raise ValueError("StipClassifier.save: the model is not fitted")
        cb = self.codebook
        if self.kernel_svm is None:
            model = dict(coef=self.coef, intercept=self.intercept, classes=self.classes)
        else:  # the kernel model's arrays under a ksvm_ prefix, beside the keys every file has
            model = dict(intercept=self.intercept, classes=self.classes)
            model.update(("ksvm_" + k, v) for k, v in self.kernel_svm.state().items())
        with open(path, "wb") as f:
            np.savez(f, centres=cb.centres, inertia=np.float64(cb.inertia), n_iter=np.int64(cb.n_iter), converged=np.bool_(cb.converged),
                     counts=cb.counts, norm=np.str_(self.norm), **model)

    @classmethod
    def load(cls, path):
        m = cls()
        with np.load(path) as z:
            m.codebook = vcodebook.Codebook(z["centres"], float(z["inertia"]), int(z["n_iter"]), bool(z["converged"]), z["counts"])
            m.norm = str(z["norm"])
            m.intercept, m.classes = z["intercept"], z["classes"]
            if "ksvm_kernel" in z.files:
                m.kernel_svm = ksvm.KernelSvm.from_state(z, prefix="ksvm_")
            else:
                m.coef = z["coef"]
        return m
