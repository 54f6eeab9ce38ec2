"""RGB difference, the third input modality of temporal segment networks (Sheet03/notes.txt:187-191): the
differences of ``D + 1`` consecutive RGB frames, stacked as a ``3D``-channel volume for a VGG-16 stream of its own whose
first layer is the cross-modality copy of the RGB one (``vgg.copy_first_layer``).  The reference has no code for it.

Every frame of a window goes through the same crop, resampling and flip (one S17 table row per item, ``src`` = the window's
first frame), is normalised, and neighbours are subtracted: plane ``3j + c`` is ``(r[j+1,c] - r[j,c]) / (255 * std[c])`` on
the u8 values ``r`` that ``augment.resize_images`` gives, so the mean cancels and the integer difference is exact
(``va_rgbdiff_to_stack``).  ``window_table`` and ``view_table`` build the tables of ``TwoStreamPipeline.train_videos`` and
``submit_video``.
"""
import ctypes

import numpy as np
import torch

from . import _ffi, augment
from .parameters import NORM_STDS_TF

RGB_DIFF_COUNT = 5  # TSN's number of stacked differences (six consecutive frames)
MAX_CHANNELS = 64   # va_vgg16_create's largest c_in


def check_diff_count(D, L, who):
    """-> D as an int; ValueError unless ``1 <= D <= L`` (the window of D + 1 frames lies inside a snippet's L + 1) and
    ``3*D <= 64`` (the first layer's channels)."""
    if isinstance(D, bool) or not isinstance(D, (int, np.integer)):
        raise ValueError("%s: the number of RGB differences must be an integer, got %r" % (who, D))
    D, L = int(D), int(L)
    if D < 1 or D > L or 3 * D > MAX_CHANNELS:
        raise ValueError("%s: %d RGB differences out of range (1..%d, at most %d channels)" % (who, D, L, MAX_CHANNELS))
    return D


def _starts_column(starts, n, who):
    try:
        st = [int(s) for s in starts]
    except (TypeError, ValueError):
        raise ValueError("%s: starts must be a list of frame indices" % who)
    if len(st) != n or n < 1:
        raise ValueError("%s: %d starts for %d items" % (who, len(st), n))
    return torch.tensor(st, dtype=torch.int32).view(n, 1)


def window_table(starts, crops):
    """One S17 crop per item -> the S23 table.  crops: CPU int32 ``[n,5]`` rows ``{top, left, ch, cw, flip}``
    (``augment.draw_scale_jitter_crops``); ``starts[i]``: the first frame of item i's window among the frames handed to
    ``rgb_diff_stack``.  Returns CPU int32 ``[n,6]`` rows ``{src, top, left, ch, cw, flip}``."""
    if not isinstance(crops, torch.Tensor) or crops.is_cuda or crops.dim() != 2 or crops.shape[1] != 5 or crops.dtype != torch.int32:
        raise ValueError("window_table: crops must be a CPU int32 [n,5] tensor")
    n = int(crops.shape[0])
    return torch.cat([_starts_column(starts, n, "window_table"), crops], dim=1).contiguous()


def view_table(starts, views):
    """Every window through every view -> the S23 table.  views: CPU int32 ``[V,3]`` rows ``{top, left, flip}``
    (``augment.ten_crop_views``), each a 224x224 rectangle; ``starts[s]``: the first frame of snippet s's window.  Returns
    CPU int32 ``[n*V,6]``, snippet-major: row ``s*V + v`` is ``{starts[s], top_v, left_v, 224, 224, flip_v}``."""
    if not isinstance(views, torch.Tensor) or views.is_cuda or views.dim() != 2 or views.shape[1] != 3 or views.dtype != torch.int32 \
            or views.shape[0] < 1:
        raise ValueError("view_table: views must be a CPU int32 [V,3] tensor with V >= 1")
    V = int(views.shape[0])
    n = len(starts) if hasattr(starts, "__len__") else 0
    src = _starts_column(starts, n, "view_table").repeat_interleave(V, dim=0)
    size = torch.full((V, 2), augment.CROP_SIZE, dtype=torch.int32)
    rows = torch.cat([views[:, :2], size, views[:, 2:]], dim=1).repeat(n, 1)
    return torch.cat([src, rows], dim=1).contiguous()


def denominators(stds):
    """``den[c] = 255.0f * std[c]``, rounded to float32 once -> numpy float32 ``[3]``; ValueError unless every entry is
    finite and positive."""
    try:
        s = np.asarray([float(v) for v in stds], dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("rgb_diff_stack: stds must be three numbers, got %r" % (stds,))
    if s.shape != (3,):
        raise ValueError("rgb_diff_stack: stds must be three numbers, got %r" % (stds,))
    den = np.float32(255.0) * s
    if not np.isfinite(den).all() or not (den > 0).all():
        raise ValueError("rgb_diff_stack: every std must be finite and > 0, got %r" % (stds,))
    return den.astype(np.float32)


def check_rgb_diff(frames_u8, table, n_diff, stds, layout, out):
    """The host-side checks of ``rgb_diff_stack`` (ValueError; nothing touches the device) -> (n_frames, h, w, D, den).
    Where the frames live is looked at last, so that every other rule can be exercised with host tensors."""
    who = "rgb_diff_stack"
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4:
        raise ValueError("%s: frames must be a 4-d CUDA uint8 tensor" % who)
    if layout == "NCHW":
        n, c, h, w = frames_u8.shape
    elif layout == "NHWC":
        n, h, w, c = frames_u8.shape
    else:
        raise ValueError("%s: layout must be 'NCHW' or 'NHWC', got %r" % (who, layout))
    if c != 3:
        raise ValueError("%s: frames must have 3 channels, got %d" % (who, c))
    if isinstance(n_diff, bool) or not isinstance(n_diff, (int, np.integer)) or n_diff < 1 or 3 * n_diff > MAX_CHANNELS:
        raise ValueError("%s: n_diff must be an integer in 1..%d, got %r" % (who, MAX_CHANNELS // 3, n_diff))
    D = int(n_diff)
    if n - D < 1:
        raise ValueError("%s: %d frames do not hold a window of %d differences" % (who, n, D))
    if 3 * h * w > 0x7fffffff:
        raise ValueError("%s: a %dx%d frame is too large" % (who, w, h))
    den = denominators(stds)
    augment.check_resize_table(table, n - D, h, w, who)
    n_out = int(table.shape[0])
    if n_out > 65535:
        raise ValueError("%s: %d output items exceed 65535 per call" % (who, n_out))
    numel = n_out * 3 * D * augment.CROP_SIZE * augment.CROP_SIZE
    if out is not None and (not isinstance(out, torch.Tensor) or out.numel() != numel or out.dtype != torch.float32
                            or not out.is_contiguous() or out.device != frames_u8.device):
        raise ValueError("%s: out must be a contiguous float32 tensor of %d elements on the frames' device" % (who, numel))
    if not frames_u8.is_cuda:
        raise ValueError("%s: frames must be a 4-d CUDA uint8 tensor, got one on %s" % (who, frames_u8.device))
    return int(n), int(h), int(w), D, den


def rgb_diff_stack(frames_u8, table, n_diff=RGB_DIFF_COUNT, stds=NORM_STDS_TF, layout="NCHW", out=None):
    """frames_u8: CUDA uint8 ``[n_frames,3,h,w]`` (``layout="NCHW"``) or ``[n_frames,h,w,3]`` (``"NHWC"``); table: CPU int32
    ``[n_out,6]`` rows ``{src, top, left, ch, cw, flip}`` with ``src`` the first of the item's ``n_diff + 1`` frames
    (``window_table``, ``view_table``) -> CUDA float32 ``[n_out, 3*n_diff, 224, 224]`` (DESIGN.md S23;
    ``va_rgbdiff_to_stack``), into ``out`` when given: plane ``3j + c`` is the difference of frames ``src + j + 1`` and
    ``src + j`` of channel c, both resampled as ``augment.resize_images`` does, divided by ``255 * stds[c]``.

    The table is validated with ``augment.check_resize_table`` over the ``n_frames - n_diff`` possible first frames; every
    bad argument raises ValueError on the host before any device call."""
    n, h, w, D, den = check_rgb_diff(frames_u8, table, n_diff, stds, layout, out)
    n_out = int(table.shape[0])
    frames_u8 = frames_u8.contiguous()
    dev = frames_u8.device
    if out is None:
        out = torch.empty((n_out, 3 * D, augment.CROP_SIZE, augment.CROP_SIZE), dtype=torch.float32, device=dev)
    dtable = augment.crops_to_device(table, dev)
    cden = (ctypes.c_float * 3)(*[float(v) for v in den])
    _ffi.check(_ffi.lib().va_rgbdiff_to_stack(_ffi.ctx(dev.index), _ffi.ptr(frames_u8), n, w, h, int(layout == "NHWC"), D, cden,
                                              _ffi.ptr(dtable), n_out, _ffi.ptr(out), _ffi.stream_ptr(dev)))
    return out.view(n_out, 3 * D, augment.CROP_SIZE, augment.CROP_SIZE)
