"""What the classical feature chains share on the host (``fisher``, ``codebook``, ``stip``, ``trajectories`` and
``fusion.linear_svm_fit``): the argument checks that several of them make in the same words, and the workspace step.  ``who``
heads every message, so each caller's errors read as before."""
import numpy as np
import torch

from . import _ffi
from . import flow as vflow


def check_rows(x, who, max_dim, name="x"):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("%s: %s must be a CUDA tensor" % (who, name))
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("%s: %s must be float32 [n, d], got %s %s" % (who, name, x.dtype, tuple(x.shape)))
    if x.shape[1] < 1 or x.shape[1] > max_dim:
        raise ValueError("%s: %s must have 1 .. %d columns, got %d" % (who, name, max_dim, x.shape[1]))
    return x.contiguous()


def dev64(a, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(dev)


def check_segments(segments, n, who):
    seg = np.asarray(segments.cpu() if isinstance(segments, torch.Tensor) else segments)
    if seg.ndim != 1 or len(seg) < 2 or seg.dtype.kind not in "iu":
        raise ValueError("%s: segments must be integers [n_segments + 1]" % who)
    seg = seg.astype(np.int64)
    if seg[0] != 0 or seg[-1] != n or (np.diff(seg) < 0).any():
        raise ValueError("%s: segments must ascend from 0 to the number of rows (%d)" % (who, n))
    return seg


def check_videos(descs_per_video, who):
    """A classifier's per-video descriptors -> ``(the list, segments int64 [n_videos + 1])``."""
    if isinstance(descs_per_video, torch.Tensor) or not isinstance(descs_per_video, (list, tuple)) or len(descs_per_video) == 0:
        raise ValueError("%s: descs_per_video must be a non-empty list of CUDA float32 [n_i, d] tensors" % who)
    for v in descs_per_video:
        if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.float32 or v.dim() != 2:
            raise ValueError("%s: descs_per_video must be a non-empty list of CUDA float32 [n_i, d] tensors" % who)
    if len(set(int(v.shape[1]) for v in descs_per_video)) != 1:
        raise ValueError("%s: descs_per_video must share one descriptor length" % who)
    segments = np.concatenate([[0], np.cumsum([int(v.shape[0]) for v in descs_per_video])]).astype(np.int64)
    return list(descs_per_video), segments


def workspace(nbytes, dev):
    """The uint8 workspace of ``nbytes``, what a ``va_*_workspace_bytes`` call returned: 0 means that call refused its
    arguments, and ``va_last_error`` says why."""
    if nbytes == 0:
        raise ValueError(_ffi.last_error())
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev)


def extraction_inputs(who, gray, flow, flow_params, params, over, params_type, default_params):
    """The front end of ``space_time_interest_points`` and ``dense_trajectories``: the checks on ``gray``, the parameters
    from ``params`` or the overrides, and the flow, computed or checked.  -> ``(gray, flow, params)``, the tensors contiguous."""
    if not isinstance(gray, torch.Tensor) or not gray.is_cuda:
        raise ValueError("%s: gray must be a CUDA tensor" % who)
    if gray.dim() != 3 or gray.dtype not in (torch.uint8, torch.float32):
        raise ValueError("%s: gray must be uint8 or float32 [T,H,W]" % who)
    if gray.shape[0] < 2:
        raise ValueError("%s: gray must hold at least 2 frames, got %d" % (who, gray.shape[0]))
    if params is not None and over:
        raise ValueError("%s: pass an _ffi.%s or keyword overrides, not both" % (who, params_type.__name__))
    p = params if params is not None else default_params(**over)
    if not isinstance(p, params_type):
        raise ValueError("%s: params must be an _ffi.%s" % (who, params_type.__name__))
    gray = gray.contiguous()
    T, H, W = gray.shape
    if flow is None:
        if flow_params is None:
            flow = vflow.farneback_flow(gray)
        else:
            flow = vflow.tvl1_flow(gray, flow_params)
    else:
        if flow_params is not None:
            raise ValueError("%s: flow_params describes the flow this call computes; with a given flow it must be None" % who)
        if (not isinstance(flow, torch.Tensor) or flow.device != gray.device or flow.dtype != torch.float32
                or tuple(flow.shape) != (T - 1, 2, H, W)):
            raise ValueError("%s: flow must be a float32 [%d,2,%d,%d] tensor on gray's device" % (who, T - 1, H, W))
        flow = flow.contiguous()
    return gray, flow, p


def extraction_capacity(who, bound, row_bytes, max_items, budget, noun, max_name):
    """The rows the outputs hold: ``max_items``, or with None the proven ``bound()`` (not called otherwise: the library has
    not seen the parameters yet) when ``row_bytes`` each fit ``budget``."""
    if max_items is None:
        cap = max(bound(), 1)
        need = cap * row_bytes
        if need > budget:
            raise ValueError("%s: the bound of %d %s needs %d bytes of output, more than MEMORY_BUDGET_BYTES (%d): pass %s"
                             % (who, cap, noun, need, budget, max_name))
    else:
        cap = int(max_items)
        if cap < 1:
            raise ValueError("%s: %s must be >= 1, got %d" % (who, max_name, cap))
    return cap
