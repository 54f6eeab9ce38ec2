"""Crop and horizontal flip of full-size frames on the device: ``getTransforms()``'s ``RandomCrop(224)`` and
``RandomHorizontalFlip()`` (Sheet03/utils.py:143,145) for clips of any size >= 224, e.g. UCF-101's 320x240.

The random numbers are drawn on the host with Python's ``random`` (the global generator by default, as the reference's
transforms use it), in exactly the order the reference draws them, so that a seeded run replays the reference's data path
crop for crop.  A crop is one row ``{top, left, flip}`` of a CPU int32 ``[n,3]`` tensor; the kernels
(``va_crop_images_u8``, ``va_flow_to_stack_crop``: DESIGN.md S10) receive the rows as a device copy.

Ten-crop evaluation (``ten_crop_views``) uses the same rows: a CPU int32 ``[V,3]`` view table that every clip, and every
flow image of a clip, is seen through (``crop_image_views``, ``flow.crop_flow_to_stack_views``).
"""
import random

import torch

from . import _ffi

CROP_SIZE = 224  # the literal RandomCrop(224) of Sheet03/utils.py:143


def _draw(rng, h, w, size):
    """One ``RandomCrop(size)`` + ``RandomHorizontalFlip()`` of an ``h x w`` image, draw for draw
    (utils.RandomCrop, utils.RandomHorizontalFlip): no crop numbers when the image already has the crop's size."""
    top = left = 0
    if not (h == size and w == size):
        top = rng.randint(0, h - size)
        left = rng.randint(0, w - size)
    return top, left, int(rng.random() < 0.5)


def _center(h, w, size):
    """torchvision's ``CenterCrop`` offsets; no flip."""
    return int(round((h - size) / 2.0)), int(round((w - size) / 2.0)), 0


def _check_frame(h, w, size, who):
    if size < 1 or h < size or w < size:
        raise ValueError("%s: a %dx%d frame is smaller than the %dx%d crop" % (who, w, h, size, size))


def draw_image_crops(n, h, w, size=CROP_SIZE, mode="random", rng=None):
    """Crops of ``n`` images of ``h x w`` pixels -> CPU int32 ``[n,3]`` rows ``{top, left, flip}``.

    ``mode="random"``: the reference's transform per image (``randint(0, h-size)``, ``randint(0, w-size)``,
    ``random() < 0.5``); ``"center"``: CenterCrop offsets, no flip, nothing drawn."""
    _check_frame(h, w, size, "draw_image_crops")
    rng = random if rng is None else rng
    if mode == "random":
        rows = [_draw(rng, h, w, size) for _ in range(int(n))]
    elif mode == "center":
        rows = [_center(h, w, size)] * int(n)
    else:
        raise ValueError("draw_image_crops: mode must be 'random' or 'center', got %r" % (mode,))
    return torch.tensor(rows, dtype=torch.int32).view(int(n), 3)


def draw_flow_crops(B, L, h, w, size=CROP_SIZE, mode="per_image", rng=None):
    """Crops of the 2L flow images of ``B`` clips -> CPU int32 ``[B*2L,3]``, row ``b*2L + c`` for channel c of clip b
    (channel 2k = x flow of pair k, 2k+1 its y flow).

    ``mode="per_image"``: the reference, which applies the transform to each flow image independently
    (Sheet03/temporalModel.py:86), drawing in the interleave order x_s, y_s, x_{s+1}, ...; ``"shared"``: one draw per
    clip for all its channels (the corrected mode of SURVEY.md section 8f); ``"center"``: CenterCrop offsets, no flip."""
    _check_frame(h, w, size, "draw_flow_crops")
    rng = random if rng is None else rng
    B, C = int(B), 2 * int(L)
    if mode == "per_image":
        rows = [_draw(rng, h, w, size) for _ in range(B * C)]
    elif mode == "shared":
        rows = [r for _ in range(B) for r in [_draw(rng, h, w, size)] * C]
    elif mode == "center":
        rows = [_center(h, w, size)] * (B * C)
    else:
        raise ValueError("draw_flow_crops: mode must be 'per_image', 'shared' or 'center', got %r" % (mode,))
    return torch.tensor(rows, dtype=torch.int32).view(B * C, 3)


def draw_clip_crops(B, L, rgb_hw, gray_hw, size=CROP_SIZE, rgb_mode="random", flow_mode="per_image", rng=None):
    """The crops of one batch for ``TwoStreamPipeline.submit(..., crops=)``: ``(rgb_crops [B,3], flow_crops [B*2L,3])``.
    ``rgb_hw`` / ``gray_hw``: (height, width) of the RGB and gray frames.  The RGB crops are drawn first."""
    rgb = draw_image_crops(B, rgb_hw[0], rgb_hw[1], size, rgb_mode, rng)
    fl = draw_flow_crops(B, L, gray_hw[0], gray_hw[1], size, flow_mode, rng)
    return rgb, fl


def check_crops(crops, n, h, w, size, who):
    """Host-side validation (ValueError) of a crop table for ``n`` images of ``h x w`` pixels, before anything reaches the
    GPU: CPU int32 ``[n,3]``, every ``top`` in [0, h-size], ``left`` in [0, w-size], ``flip`` 0 or 1."""
    _check_frame(h, w, size, who)
    if not isinstance(crops, torch.Tensor) or crops.is_cuda or crops.dtype != torch.int32:
        raise ValueError("%s: crops must be a CPU int32 tensor (augment.draw_*_crops)" % who)
    if crops.dim() != 2 or tuple(crops.shape) != (n, 3):
        raise ValueError("%s: crops must be [%d,3], got %s" % (who, n, tuple(crops.shape)))
    top, left, flip = crops[:, 0], crops[:, 1], crops[:, 2]
    if bool((top < 0).any()) or bool((top > h - size).any()) or bool((left < 0).any()) or bool((left > w - size).any()):
        raise ValueError("%s: a crop offset lies outside the %dx%d frame (top <= %d, left <= %d)"
                         % (who, w, h, h - size, w - size))
    if bool(((flip != 0) & (flip != 1)).any()):
        raise ValueError("%s: flip must be 0 or 1" % who)


def crops_to_device(crops, device):
    """Non-blocking copy of a (validated) crop table from pinned memory, ordered on the current stream.  The returned
    tensor belongs to that stream's pool of the caching allocator, so it stays valid for every kernel enqueued on the
    same stream after the copy; the pinned staging block is held by the allocator until the copy has run."""
    return crops.contiguous().pin_memory().to(device, non_blocking=True)


def crop_images(x_u8, crops, size=CROP_SIZE, layout="NCHW"):
    """x_u8: CUDA uint8 ``[n,c,h,w]`` (``layout="NCHW"``) or ``[n,h,w,c]`` (``"NHWC"``, the decode order of PIL / JPEG);
    crops: CPU int32 ``[n,3]`` -> CUDA uint8 ``[n,c,size,size]`` NCHW, the u8 input of ``Vgg16Stream.forward`` (which
    applies ToTensor + Normalize itself)."""
    if not isinstance(x_u8, torch.Tensor) or not x_u8.is_cuda or x_u8.dtype != torch.uint8 or x_u8.dim() != 4:
        raise ValueError("crop_images: x must be a 4-d CUDA uint8 tensor")
    if layout == "NCHW":
        n, c, h, w = x_u8.shape
    elif layout == "NHWC":
        n, h, w, c = x_u8.shape
    else:
        raise ValueError("crop_images: layout must be 'NCHW' or 'NHWC', got %r" % (layout,))
    check_crops(crops, n, h, w, size, "crop_images")
    x_u8 = x_u8.contiguous()
    dev = x_u8.device
    out = torch.empty((n, c, size, size), dtype=torch.uint8, device=dev)
    dcrops = crops_to_device(crops, dev)
    _ffi.check(_ffi.lib().va_crop_images_u8(_ffi.ctx(dev.index), _ffi.ptr(x_u8), n, c, w, h, int(layout == "NHWC"),
                                            _ffi.ptr(dcrops), size, size, _ffi.ptr(out), _ffi.stream_ptr(dev)))
    return out


def ten_crop_views(h, w, size=CROP_SIZE):
    """torchvision's ``TenCrop(size)`` of an ``h x w`` image as a CPU int32 ``[10,3]`` view table ``{top, left, flip}``:
    ``five_crop`` of the image (top-left, top-right, bottom-left, bottom-right, centre), then ``five_crop`` of its
    mirror, with every row in the original frame's coordinates.  View 4 is ``draw_image_crops(mode="center")``; view 9,
    the mirror's centre, has ``left = (w-size) - cl``, which differs from view 4's ``cl`` when ``w - size`` is odd.
    Draws no random numbers."""
    _check_frame(h, w, size, "ten_crop_views")
    ct, cl, _ = _center(h, w, size)
    b, r = h - size, w - size
    five = [(0, 0), (0, r), (b, 0), (b, r), (ct, cl)]
    mirrored = [(0, r), (0, 0), (b, r), (b, 0), (ct, r - cl)]  # five_crop of the mirror: its left is r - left
    rows = [(t, l, 0) for t, l in five] + [(t, l, 1) for t, l in mirrored]
    return torch.tensor(rows, dtype=torch.int32)


def check_views(views, h, w, size, who):
    """Host-side validation (ValueError) of a view table for ``h x w`` frames: CPU int32 ``[V,3]`` with V >= 1 and the
    rules of ``check_crops`` for every row."""
    if not isinstance(views, torch.Tensor) or views.dim() != 2 or views.shape[0] < 1 or views.shape[1] != 3:
        raise ValueError("%s: views must be a CPU int32 [V,3] tensor with V >= 1 (augment.ten_crop_views)" % who)
    check_crops(views, views.shape[0], h, w, size, who)


def expand_views(views, n, per=1):
    """A ``[V,3]`` view table -> the crop table of ``n`` items with ``per`` planes each seen through every view: row
    ``(i*V + v)*per + c`` is view v (``per = 2L``: one row per output plane of a flow volume; ``per = 1``: one per
    output image)."""
    return views.repeat_interleave(int(per), dim=0).repeat(int(n), 1).contiguous()


def crop_image_views(x_u8, views, size=CROP_SIZE, layout="NCHW"):
    """x_u8: CUDA uint8 ``[n,c,h,w]`` (``layout="NCHW"``) or ``[n,h,w,c]`` (``"NHWC"``); views: CPU int32 ``[V,3]``
    (``ten_crop_views``) -> CUDA uint8 ``[n,V,c,size,size]``: every image through every view, the u8 input of
    ``Vgg16Stream.forward_views``."""
    if not isinstance(x_u8, torch.Tensor) or not x_u8.is_cuda or x_u8.dtype != torch.uint8 or x_u8.dim() != 4:
        raise ValueError("crop_image_views: x must be a 4-d CUDA uint8 tensor")
    if layout == "NCHW":
        n, c, h, w = x_u8.shape
    elif layout == "NHWC":
        n, h, w, c = x_u8.shape
    else:
        raise ValueError("crop_image_views: layout must be 'NCHW' or 'NHWC', got %r" % (layout,))
    check_views(views, h, w, size, "crop_image_views")
    V = views.shape[0]
    x_u8 = x_u8.contiguous()
    dev = x_u8.device
    out = torch.empty((n, V, c, size, size), dtype=torch.uint8, device=dev)
    dcrops = crops_to_device(expand_views(views, n), dev)
    _ffi.check(_ffi.lib().va_crop_images_u8_views(_ffi.ctx(dev.index), _ffi.ptr(x_u8), n, c, w, h, int(layout == "NHWC"), V,
                                                  _ffi.ptr(dcrops), size, size, _ffi.ptr(out), _ffi.stream_ptr(dev)))
    return out
