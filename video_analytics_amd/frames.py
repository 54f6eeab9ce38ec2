"""Decoded frames -> the pipeline's inputs, on the device: the whole-frame rescale both papers apply before
flow is computed ("the smallest side of the frame equals 256", Sheet03/notes.txt:104; TSN's 340x256) and the gray frames
TV-L1 reads, from ``uint8`` RGB frames of any size.

``prepare_frames(rgb, size)`` gives what ``Image.resize((ow, oh), Image.BILINEAR)`` and ``convert('L')`` of every frame give,
bit for bit: the gray level is ``utils.grayLevel``; the resize is PIL's 8-bit two-pass resample, whose taps the host builds in
float64 (``resample_table``) and whose sums the device forms in int32 (``va_frames_prepare``).  ``resizeBilinear`` and
``prepareFrames`` restate both in numpy, in the style of ``utils.grayLevel``; tests hold the kernels to them and to PIL.
"""
import math
import numbers

import numpy as np

from . import utils

PRECISION_BITS = 22  # PIL's 8-bit resample: taps are fixed point with 32 - 8 - 2 fractional bits
MAX_KSIZE = 33       # taps per output sample the device accepts: a downscale factor of at most 16


def short_side_size(h, w, s):
    """torchvision's ``Resize(s)`` of an ``h x w`` image -> ``(oh, ow)``: the short side becomes ``s``, the long side
    ``int(s * long / short)`` (240x320 at 256: 256x341)."""
    h, w, s = int(h), int(w), int(s)
    if h < 1 or w < 1 or s < 1:
        raise ValueError("short_side_size: sizes must be >= 1, got %dx%d -> %d" % (h, w, s))
    if w <= h:
        return int(s * h / w), s
    return s, int(s * w / h)


def kernel_size(n_in, n_out):
    """Taps per output sample of one axis: ``2 ceil(max(in / out, 1)) + 1``."""
    return 2 * int(math.ceil(max(float(n_in) / float(n_out), 1.0))) + 1


def resample_table(n_in, n_out):
    """The bilinear taps of one axis, ``n_in`` samples to ``n_out`` -> ``(bounds int32 [n_out,2], taps int32
    [n_out,ksize])``: row i of ``bounds`` is ``{xmin, n}``, the first input sample and the number of samples output i reads;
    ``taps[i,:n]`` are their weights in units of ``2**-22`` (zeros behind them).  PIL's ``precompute_coeffs`` and
    ``normalize_coeffs_8bpc`` operation for operation in float64: the triangle of half-width ``max(in / out, 1)`` around
    ``(i + 0.5) in / out``, normalised by its sum, each weight rounded half up."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("resample_table: lengths must be >= 1, got %d -> %d" % (n_in, n_out))
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = fs  # the bilinear filter's support, 1, times fs
    ss = 1.0 / fs
    ksize = kernel_size(n_in, n_out)
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    taps = np.zeros((n_out, ksize), dtype=np.int32)
    for i in range(n_out):
        c = (i + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), n_in) - xmin
        w = [max(0.0, 1.0 - abs((j + xmin - c + 0.5) * ss)) for j in range(n)]
        ww = 0.0
        for v in w:  # PIL adds them in tap order
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[i] = (xmin, n)
        taps[i, :n] = [int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    return bounds, taps


def _resample_axis(a, n_out, axis):
    """One pass of the 8-bit resample along ``axis`` of a uint8 array -> uint8."""
    a = np.moveaxis(np.asarray(a), axis, -1)
    bounds, taps = resample_table(a.shape[-1], n_out)
    src = a.astype(np.int64)
    out = np.empty(a.shape[:-1] + (n_out,), dtype=np.uint8)
    for i in range(n_out):
        lo, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (1 << (PRECISION_BITS - 1)) + (src[..., lo:lo + n] * taps[i, :n].astype(np.int64)).sum(axis=-1)
        out[..., i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, -1, axis)


def resizeBilinear(a, oh, ow):
    """PIL's ``Image.resize((ow, oh), Image.BILINEAR)`` of a uint8 array ``[..., h, w, c]`` (HWC, any leading axes) ->
    ``[..., oh, ow, c]``: the horizontal pass into a uint8 intermediate, then the vertical pass; a pass whose length does not
    change is skipped.  ``out = clamp((2**21 + sum_j p[xmin + j] k_j) >> 22, 0, 255)`` with ``resample_table``'s taps."""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim < 3:
        raise ValueError("resizeBilinear: need a uint8 [...,h,w,c] array")
    oh, ow = int(oh), int(ow)
    if oh < 1 or ow < 1 or a.shape[-3] < 1 or a.shape[-2] < 1:
        raise ValueError("resizeBilinear: sizes must be >= 1")
    if ow != a.shape[-2]:
        a = _resample_axis(a, ow, -2)
    if oh != a.shape[-3]:
        a = _resample_axis(a, oh, -3)
    return a


def prepareFrames(a, size=None):
    """The host statement of ``prepare_frames``: uint8 RGB frames ``[..., h, w, 3]`` -> ``(rgb [..., oh, ow, 3], gray
    [..., oh, ow])``, ``resizeBilinear`` then ``utils.grayLevel``.  ``size`` as there."""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim < 3 or a.shape[-1] != 3:
        raise ValueError("prepareFrames: need a uint8 [...,h,w,3] array")
    oh, ow = output_size(a.shape[-3], a.shape[-2], size, "prepareFrames")
    out = resizeBilinear(a, oh, ow)
    return out, utils.grayLevel(out)


def output_size(h, w, size, who="prepare_frames"):
    """``size`` of ``prepare_frames`` for ``h x w`` frames -> ``(oh, ow)``: None keeps the size, an int is
    ``short_side_size``'s rule, a pair is ``(oh, ow)`` itself.  ValueError for anything else, for an empty frame, an output
    side below 1 and a downscale factor above 16 on either axis (more than ``MAX_KSIZE`` taps)."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError("%s: empty %dx%d frames" % (who, w, h))

    def integer(v):
        return isinstance(v, numbers.Integral) and not isinstance(v, bool)
    if size is None:
        return h, w
    if integer(size):
        if size < 1:
            raise ValueError("%s: size must be >= 1, got %d" % (who, size))
        oh, ow = short_side_size(h, w, size)
    elif isinstance(size, (tuple, list)) and len(size) == 2 and integer(size[0]) and integer(size[1]):
        oh, ow = int(size[0]), int(size[1])
    else:
        raise ValueError("%s: size must be None, an int (the short side) or (height, width), got %r" % (who, size))
    if oh < 1 or ow < 1:
        raise ValueError("%s: the output would be %dx%d" % (who, ow, oh))
    if kernel_size(h, oh) > MAX_KSIZE or kernel_size(w, ow) > MAX_KSIZE:
        raise ValueError("%s: %dx%d -> %dx%d shrinks an axis by more than 16" % (who, w, h, ow, oh))
    return oh, ow


def check_frames(rgb, size=None, layout="NCHW", who="prepare_frames"):
    """The host-side checks of ``prepare_frames`` short of the device (ValueError; nothing is enqueued) ->
    ``(n, h, w, oh, ow)``: ``rgb`` a uint8 tensor ``[n,3,h,w]`` (``"NCHW"``) or ``[n,h,w,3]`` (``"NHWC"``) with n >= 1."""
    import torch
    if layout not in ("NCHW", "NHWC"):
        raise ValueError("%s: layout must be 'NCHW' or 'NHWC', got %r" % (who, layout))
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8 or rgb.dim() != 4:
        raise ValueError("%s: rgb must be a 4-d uint8 tensor" % who)
    if layout == "NCHW":
        n, c, h, w = rgb.shape
    else:
        n, h, w, c = rgb.shape
    if c != 3:
        raise ValueError("%s: rgb must hold 3 channels (%s), got %s" % (who, layout, tuple(rgb.shape)))
    if n < 1:
        raise ValueError("%s: no frames" % who)
    oh, ow = output_size(h, w, size, who)
    return int(n), int(h), int(w), oh, ow


_tables = {}


def device_table(n_in, n_out, device):
    """``resample_table`` on ``device``, built and copied once per ``(n_in, n_out, device)``; the copy is complete when this
    returns, so every stream may read it."""
    import torch
    key = (int(n_in), int(n_out), str(device))
    if key not in _tables:
        bounds, taps = resample_table(n_in, n_out)
        _tables[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(taps).to(device))
    return _tables[key]


def _check_out(t, shape, dev, name):
    import torch
    numel = 1
    for d in shape:
        numel *= d
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.numel() != numel or not t.is_contiguous()
            or t.device != dev):
        raise ValueError("prepare_frames: %s must be a contiguous uint8 tensor of %d elements on rgb's device" % (name, numel))


def prepare_frames(rgb, size=None, layout="NCHW", out_rgb=None, out_gray=None):
    """rgb: CUDA uint8 ``[n,3,h,w]`` (``layout="NCHW"``) or ``[n,h,w,3]`` (``"NHWC"``, the decode order of PIL / JPEG) ->
    ``(rgb_out u8 [n,3,oh,ow], gray u8 [n,oh,ow])``: every frame through PIL's bilinear resize and ``convert('L')``, bit for
    bit (``va_frames_prepare``), ordered on the current stream.

    ``size``: None keeps the size (gray only; planar frames come back as they are unless ``out_rgb`` asks for a copy), an
    int is torchvision's ``Resize(size)`` rule (``short_side_size``), a pair is ``(oh, ow)``.  ``out_rgb`` / ``out_gray``:
    contiguous uint8 tensors to write into.  ValueError for a wrong dtype, rank, layout or device, no frames, an output side
    below 1 and a downscale factor above 16, before anything is enqueued."""
    import torch
    from . import _ffi
    n, h, w, oh, ow = check_frames(rgb, size, layout)
    if not rgb.is_cuda:
        raise ValueError("prepare_frames: rgb must be on a CUDA device")
    dev = rgb.device
    nhwc = layout == "NHWC"
    same = (oh, ow) == (h, w)
    if out_rgb is not None:
        _check_out(out_rgb, (n, 3, oh, ow), dev, "out_rgb")
    if out_gray is not None:
        _check_out(out_gray, (n, oh, ow), dev, "out_gray")
    rgb = rgb.contiguous()
    if out_rgb is None and not (same and not nhwc):
        out_rgb = torch.empty((n, 3, oh, ow), dtype=torch.uint8, device=dev)
    if out_gray is None:
        out_gray = torch.empty((n, oh, ow), dtype=torch.uint8, device=dev)
    xb, xt = device_table(w, ow, dev) if ow != w else (None, None)
    yb, yt = device_table(h, oh, dev) if oh != h else (None, None)
    L = _ffi.lib()
    nbytes = int(L.va_frames_prepare_workspace_bytes(n, w, h, ow, oh))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None  # stream-ordered, this call's own
    _ffi.check(L.va_frames_prepare(_ffi.ctx(dev.index), _ffi.ptr(rgb), n, w, h, int(nhwc), ow, oh, _ffi.ptr(xb), _ffi.ptr(xt),
                                   _ffi.ptr(yb), _ffi.ptr(yt), _ffi.ptr(out_rgb), _ffi.ptr(out_gray), _ffi.ptr(work), nbytes,
                                   _ffi.stream_ptr(dev)))
    return (rgb if out_rgb is None else out_rgb.view(n, 3, oh, ow)), out_gray.view(n, oh, ow)
