"""Dense trajectories on MI355X (``va_dtraj_extract``): the extraction stage of the modelled project's
Sheet02 -- sampling points, following them through the median-filtered flow, HOG / HOF / MBHx / MBHy histograms and the
trajectory shape in a tube around each track -- ending at the per-trajectory descriptors ``[n, 426]``.

The flow comes from this library (Farneback with Sheet02's arguments by default, Sheet02.py:191) or from the caller; the 3x3
median Sheet02 applies before tracking (Sheet02.py:293-299) is ``flow.median_filter``.

``TrajectoryClassifier`` is the rest of Sheet02's ``main()`` (Sheet02.py:568-617, 710-763) on top of ``desc``: PCA, the
diagonal Gaussian mixture and the Fisher vectors of ``fisher``, then ``fusion.linear_svm_fit``.
"""
import ctypes

import numpy as np
import torch

from . import _features
from . import _ffi
from . import fisher
from . import flow as vflow
from . import fusion
from . import ksvm

REJECTED = ("left_frame", "static", "erratic", "jump", "unfinished")
# what the outputs sized for the proven bound cells * (T - length) may take when max_trajectories is None
MEMORY_BUDGET_BYTES = 8 << 30


def descriptor_length(params):
    """2 * length values of shape, then 8 + 9 + 8 + 8 bins in each of the nt * nxy * nxy cells: 426 at the defaults"""
    return 2 * params.length + 33 * params.nt * params.nxy * params.nxy


def trajectory_bound(w, h, n_frames, params):
    """No video yields more: every grid cell can start one track at every frame t <= T - 1 - length (S74)."""
    return (w // params.step) * (h // params.step) * max(n_frames - params.length, 0)


def dense_trajectories(gray, flow=None, params=None, flow_params=None, max_trajectories=None, **over):
    """gray: CUDA uint8 or float32 ``[T,H,W]`` in [0,255], T >= 2, H and W in [16,16384].

    ``flow``: None computes ``farneback_flow(gray, flow_params)`` (an ``_ffi.Tvl1Params`` or ``_ffi.BroxParams`` in
    ``flow_params`` selects those methods, as ``flow.tvl1_flow`` does everywhere); a CUDA float32 ``[T-1,2,H,W]`` tensor is
    used as it is (a stored flow of ``extract_flow`` in float32 is one).  ``params``: an ``_ffi.DenseTrajParams`` or keyword
    overrides (step, length, patch, nxy, nt, quality, min_flow, min_std, max_std, max_dis, max_dis_share), not both.

    Returns a dict: ``desc`` float32 ``[n, 426]`` (shape 30 | HOG 96 | HOF 108 | MBHx 96 | MBHy 96 at the defaults),
    ``points`` float32 ``[n, length+1, 2]`` (x, y), ``start`` int32 ``[n]`` (first frame), all CUDA and in order of the last
    frame, then of the track; ``rejected``: a dict of the five counts ``REJECTED``; ``count``: n.  More than
    ``max_trajectories`` raises ValueError stating the count found; nothing is cut short.  With ``max_trajectories=None``
    the outputs are sized for ``trajectory_bound`` and the call raises ValueError when that does not fit
    ``MEMORY_BUDGET_BYTES``.  The inputs are left untouched.
    """
    who = "dense_trajectories"
    gray, flow, p = _features.extraction_inputs(who, gray, flow, flow_params, params, over, _ffi.DenseTrajParams,
                                                _ffi.default_dense_traj_params)
    T, H, W = gray.shape
    L = _ffi.lib()
    dim, npts = descriptor_length(p), p.length + 1
    cap = _features.extraction_capacity(who, lambda: trajectory_bound(W, H, T, p), (dim + 2 * npts + 1) * 4, max_trajectories,
                                        MEMORY_BUDGET_BYTES, "trajectories", "max_trajectories")
    dev = gray.device
    ws = _features.workspace(L.va_dtraj_workspace_bytes(W, H, T, cap, ctypes.byref(p)), dev)
    median = vflow.median_filter(flow, 3)
    desc = torch.empty((cap, dim), dtype=torch.float32, device=dev)
    points = torch.empty((cap, npts, 2), dtype=torch.float32, device=dev)
    start = torch.empty((cap,), dtype=torch.int32, device=dev)
    count = ctypes.c_int(0)
    rejected = (ctypes.c_int * 5)()
    _ffi.check(L.va_dtraj_extract(_ffi.ctx(dev.index), _ffi.ptr(gray), int(gray.dtype == torch.uint8), _ffi.ptr(flow), _ffi.ptr(median),
                                  T, W, H, ctypes.byref(p), _ffi.ptr(desc), _ffi.ptr(points), _ffi.ptr(start), cap, ctypes.byref(count),
                                  rejected, _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(dev)))
    n = int(count.value)
    if n > cap:
        raise ValueError("%s: found %d trajectories, more than max_trajectories = %d" % (who, n, cap))
    return {"desc": desc[:n], "points": points[:n], "start": start[:n], "rejected": dict(zip(REJECTED, (int(r) for r in rejected))),
            "count": n}


class TrajectoryClassifier(object):
    """Sheet02's ``main()`` after the extraction (Sheet02.py:710-763): PCA of all training descriptors, a diagonal Gaussian
    mixture fitted to the reduced rows, one Fisher vector per video, a linear SVM on those.

    ``descs_per_video``: a list of CUDA float32 ``[n_i, d]`` tensors, one per video (``dense_trajectories(...)["desc"]``); a
    video with no trajectories (``n_i = 0``) is legal and gets a zero vector.  With the default ``svm="primal"`` the Fisher
    vector's length ``n_gmm (1 + 2 n_components)`` must not exceed 8192, the widest problem ``fusion.linear_svm_fit`` takes;
    ``svm="dual"`` fits the same model over the videos' linear Gram matrix (``ksvm``) and has no such limit, and neither has
    ``encode`` (Sheet02's 64 x 256 gives 33,024)."""

    SVM_MAX_DIM = 8192

    def __init__(self):
        self.pca = self.gmm = self.coef = self.intercept = self.classes = None
        self.power = 0.0

    def fit(self, descs_per_video, labels, n_components=64, n_gmm=256, power=0.0, svm="primal", **gmm_kw):
        """PCA to ``n_components`` (Sheet02.py:40), ``gmm_fit`` with ``n_gmm`` components (Sheet02.py:41) and ``gmm_kw``,
        Fisher vectors with ``power``, then the linear SVM: ``svm="primal"`` is ``fusion.linear_svm_fit`` (at most 8192
        columns), ``svm="dual"`` is ``ksvm.kernel_svm_fit`` on ``ksvm.linear_gram`` of the Fisher vectors (2 .. 16384 videos,
        any length), collapsed to the same ``coef`` and ``intercept``.  -> self."""
        who = "TrajectoryClassifier.fit"
        if svm not in ("primal", "dual"):
            raise ValueError("%s: svm must be 'primal' or 'dual', got %r" % (who, svm))
        videos, segments = _features.check_videos(descs_per_video, who)
        if len(labels) != len(videos):
            raise ValueError("%s: %d videos but %d labels" % (who, len(videos), len(labels)))
        if isinstance(n_gmm, bool) or not isinstance(n_gmm, (int, np.integer)) or n_gmm < 1:
            raise ValueError("%s: n_gmm must be an integer >= 1, got %r" % (who, n_gmm))
        if svm == "primal" and isinstance(n_components, (int, np.integer)) and n_gmm * (1 + 2 * n_components) > self.SVM_MAX_DIM:
            raise ValueError("%s: the Fisher vector's length n_gmm (1 + 2 n_components) = %d exceeds the %d columns linear_svm_fit takes"
                             % (who, n_gmm * (1 + 2 * n_components), self.SVM_MAX_DIM))
        self.pca = fisher.pca_fit(videos, n_components)
        reduced = self.pca.transform(torch.cat(videos, 0))
        self.gmm = fisher.gmm_fit(reduced, n_gmm, **gmm_kw)
        self.power = float(power)
        fv = fisher.fisher_vectors(reduced, segments, self.gmm, self.power)
        if svm == "primal":
            self.coef, self.intercept, self.classes = fusion.linear_svm_fit(fv, labels)
        else:
            dual_coef, self.intercept, self.classes = ksvm.kernel_svm_fit(ksvm.linear_gram(fv), labels)
            self.coef = (dual_coef @ fv.to(torch.float64)).cpu().numpy()
        return self

    def encode(self, descs_per_video):
        """The Fisher vectors CUDA float32 ``[n_videos, K + 2KD]`` of the fitted PCA and mixture, for callers who fuse them
        elsewhere."""
        who = "TrajectoryClassifier.encode"
        if self.pca is None or self.gmm is None:
            raise ValueError("%s: the model is not fitted" % who)
        videos, segments = _features.check_videos(descs_per_video, who)
        return fisher.fisher_vectors(self.pca.transform(torch.cat(videos, 0)), segments, self.gmm, self.power)

    def predict(self, descs_per_video):
        """-> the predicted labels, one per video (``fusion.linear_svm_predict`` on the Fisher vectors)."""
        if self.coef is None:
            raise ValueError("TrajectoryClassifier.predict: the model is not fitted")
        fv = self.encode(descs_per_video)
        return fusion.linear_svm_predict(fv.double().cpu().numpy(), self.coef, self.intercept, self.classes, device=fv.device.index)

    def save(self, path):
        if self.coef is None:
            raise ValueError("TrajectoryClassifier.save: the model is not fitted")
        with open(path, "wb") as f:
            np.savez(f, pca_mean=self.pca.mean, pca_components=self.pca.components, pca_explained_variance=self.pca.explained_variance,
                     pca_n_samples=np.int64(self.pca.n_samples), gmm_weights=self.gmm.weights, gmm_means=self.gmm.means,
                     gmm_variances=self.gmm.variances, gmm_converged=np.bool_(self.gmm.converged), gmm_n_iter=np.int64(self.gmm.n_iter),
                     gmm_lower_bound=np.float64(self.gmm.lower_bound), gmm_history=np.asarray(self.gmm.history, dtype=np.float64),
                     power=np.float64(self.power), coef=self.coef, intercept=self.intercept, classes=self.classes)

    @classmethod
    def load(cls, path):
        m = cls()
        with np.load(path) as z:
            m.pca = fisher.PCAModel(z["pca_mean"], z["pca_components"], z["pca_explained_variance"], int(z["pca_n_samples"]))
            m.gmm = fisher.GMMModel(z["gmm_weights"], z["gmm_means"], z["gmm_variances"], bool(z["gmm_converged"]), int(z["gmm_n_iter"]),
                                    float(z["gmm_lower_bound"]), z["gmm_history"].tolist())
            m.power = float(z["power"])
            m.coef, m.intercept, m.classes = z["coef"], z["intercept"], z["classes"]
        return m
