"""Crop and horizontal flip of full-size frames on the device: ``getTransforms()``'s ``RandomCrop(224)`` and
``RandomHorizontalFlip()`` (Sheet03/utils.py:143,145) for clips of any size >= 224, e.g. UCF-101's 320x240.

The random numbers are drawn on the host with Python's ``random`` (the global generator by default, as the reference's
transforms use it), in exactly the order the reference draws them, so that a seeded run replays the reference's data path
crop for crop.  A crop is one row ``{top, left, flip}`` of a CPU int32 ``[n,3]`` tensor; the kernels
(``va_crop_images_u8``, ``va_flow_to_stack_crop``: DESIGN.md S10) receive the rows as a device copy.

Ten-crop evaluation (``ten_crop_views``) uses the same rows: a CPU int32 ``[V,3]`` view table that every clip, and every
flow image of a clip, is seen through (``crop_image_views``, ``flow.crop_flow_to_stack_views``).

TSN's training augmentations (Sheet03/notes.txt:212-223), corner cropping and scale jittering, draw a
crop size as well: ``draw_scale_jitter_crops`` gives rows ``{top, left, ch, cw, flip}``, one per snippet, and
``snippet_tables`` expands them into the ``{src, top, left, ch, cw, flip}`` tables of the crop-resize gathers
(``resize_images``, ``flow.resize_flow_to_stack``), which resample every crop to 224x224.

Colour jitter: ``draw_color_jitter`` gives one row ``{op0, op1, op2, op3, f_brightness, f_contrast,
f_saturation, hue_shift}`` per image of a CPU float32 ``[n,8]`` table, ``color_jitter`` applies it on the device
(``va_color_jitter_u8``) with the optional PCA lighting offsets of ``draw_lighting``.
"""
import random

import torch

from . import _ffi
from . import utils

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


# ---- TSN's multi-scale crop ----

SCALE_JITTER_SCALES = (1, .875, .75, .66)  # TSN's scale_ratios


def scale_jitter_sizes(h, w, scales=SCALE_JITTER_SCALES):
    """-> (sizes, pairs): ``sizes[i] = int(min(h, w) * scales[i])``, a size within 3 of 224 becoming 224; ``pairs`` the
    candidate ``(cw, ch)`` = ``(sizes[j], sizes[i])`` with ``|i - j| <= 1`` in i-major order (ten for four scales)."""
    base = min(int(h), int(w))
    sizes = [int(base * s) for s in scales]
    sizes = [CROP_SIZE if abs(x - CROP_SIZE) < 3 else x for x in sizes]
    pairs = [(sizes[j], sizes[i]) for i in range(len(sizes)) for j in range(len(sizes)) if abs(i - j) <= 1]
    return sizes, pairs


def fixed_offsets(h, w, ch, cw, more=True):
    """The ``(left, top)`` corner-crop offsets of a ``ch x cw`` crop in an ``h x w`` frame: the four corners and the
    centre, with ``more`` also the four edge centres and the four quarter points (thirteen in all)."""
    ws, hs = (int(w) - int(cw)) // 4, (int(h) - int(ch)) // 4
    ret = [(0, 0), (4 * ws, 0), (0, 4 * hs), (4 * ws, 4 * hs), (2 * ws, 2 * hs)]
    if more:
        ret += [(0, 2 * hs), (4 * ws, 2 * hs), (2 * ws, 4 * hs), (2 * ws, 0), (ws, hs), (3 * ws, hs), (ws, 3 * hs),
                (3 * ws, 3 * hs)]
    return ret


def draw_scale_jitter_crops(n, h, w, rng=None, fix=True, more=True, scales=SCALE_JITTER_SCALES):
    """``n`` multi-scale crops of ``h x w`` frames -> CPU int32 ``[n,5]`` rows ``{top, left, ch, cw, flip}``.  Per crop, in
    this order: ``rng.choice`` of the size pairs, ``rng.choice`` of the fixed offsets (``fix=False``:
    ``rng.randint(0, w - cw)`` then ``rng.randint(0, h - ch)``), ``rng.random() < 0.5``.  One crop serves a whole snippet,
    its RGB frame and all 2L flow planes (TSN's group transform)."""
    rng = random if rng is None else rng
    h, w = int(h), int(w)
    _, pairs = scale_jitter_sizes(h, w, scales)
    pairs = [(cw, ch) for cw, ch in pairs if 1 <= cw <= w and 1 <= ch <= h]
    if not pairs:
        raise ValueError("draw_scale_jitter_crops: no crop size fits a %dx%d frame" % (w, h))
    rows = []
    for _ in range(int(n)):
        cw, ch = rng.choice(pairs)
        if fix:
            left, top = rng.choice(fixed_offsets(h, w, ch, cw, more))
        else:
            left = rng.randint(0, w - cw)
            top = rng.randint(0, h - ch)
        rows.append((top, left, ch, cw, int(rng.random() < 0.5)))
    return torch.tensor(rows, dtype=torch.int32).view(int(n), 5)


def check_jitter_crops(crops, n, h, w, who):
    """Host-side validation (ValueError) of ``n`` rows ``{top, left, ch, cw, flip}`` for ``h x w`` frames: CPU int32
    ``[n,5]``, ``1 <= ch <= h``, ``1 <= cw <= w``, the rectangle inside the frame, ``flip`` 0 or 1."""
    if not isinstance(crops, torch.Tensor) or crops.is_cuda or crops.dtype != torch.int32:
        raise ValueError("%s: crops must be a CPU int32 tensor (augment.draw_scale_jitter_crops)" % who)
    if crops.dim() != 2 or tuple(crops.shape) != (n, 5):
        raise ValueError("%s: crops must be [%d,5], got %s" % (who, n, tuple(crops.shape)))
    _check_rects(crops, h, w, who)


def _check_rects(rows, h, w, who):
    top, left, ch, cw, flip = (rows[:, i].to(torch.int64) for i in range(5))
    if bool((ch < 1).any()) or bool((ch > h).any()) or bool((cw < 1).any()) or bool((cw > w).any()):
        raise ValueError("%s: a crop size lies outside 1..%d x 1..%d" % (who, w, h))
    if bool((top < 0).any()) or bool((top + ch > h).any()) or bool((left < 0).any()) or bool((left + cw > w).any()):
        raise ValueError("%s: a crop rectangle leaves the %dx%d frame" % (who, w, h))
    if bool(((flip != 0) & (flip != 1)).any()):
        raise ValueError("%s: flip must be 0 or 1" % who)


def check_resize_table(table, n_src, h, w, who):
    """Host-side validation (ValueError) of a crop-resize table over ``n_src`` planes or images of
    ``h x w`` pixels: CPU int32 ``[n_out,6]`` rows ``{src, top, left, ch, cw, flip}`` with n_out >= 1, ``src`` in
    [0, n_src) and the rules of ``check_jitter_crops`` for the rest."""
    if not isinstance(table, torch.Tensor) or table.is_cuda or table.dtype != torch.int32:
        raise ValueError("%s: the table must be a CPU int32 tensor (augment.snippet_tables)" % who)
    if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] != 6:
        raise ValueError("%s: the table must be [n_out,6] with n_out >= 1, got %s" % (who, tuple(table.shape)))
    if bool((table[:, 0] < 0).any()) or bool((table[:, 0] >= n_src).any()):
        raise ValueError("%s: src must lie in [0, %d)" % (who, n_src))
    _check_rects(table[:, 1:], h, w, who)


def snippet_tables(crops, frames, flow_starts, flow_count):
    """One crop per snippet -> the two S17 tables.  crops: CPU int32 ``[n,5]`` (``draw_scale_jitter_crops``); ``frames[i]``:
    the index of snippet i's RGB frame among the images handed to ``resize_images``; ``flow_starts[i]``: the index of its
    first flow field among the fields handed to ``flow.resize_flow_to_stack``, its window being the ``flow_count`` = L
    fields from there.  Returns ``(rgb_table [n,6], flow_table [n*2L,6])``: flow row ``i*2L + c`` reads source plane
    ``2*flow_starts[i] + c`` through snippet i's crop (channel 2k = x flow of the window's pair k)."""
    if not isinstance(crops, torch.Tensor) or crops.dim() != 2 or crops.shape[1] != 5 or crops.dtype != torch.int32:
        raise ValueError("snippet_tables: crops must be a CPU int32 [n,5] tensor")
    n, C = crops.shape[0], 2 * int(flow_count)
    if len(frames) != n or len(flow_starts) != n or C < 2:
        raise ValueError("snippet_tables: need one frame and one flow start per crop and flow_count >= 1")
    fr = torch.tensor([int(f) for f in frames], dtype=torch.int32).view(n, 1)
    fs = torch.tensor([int(f) for f in flow_starts], dtype=torch.int32).view(n, 1)
    rgb = torch.cat([fr, crops], dim=1)
    src = (2 * fs + torch.arange(C, dtype=torch.int32).view(1, C)).reshape(n * C, 1)
    flow = torch.cat([src, crops.repeat_interleave(C, dim=0)], dim=1)
    return rgb.contiguous(), flow.contiguous()


def resize_images(x_u8, table, layout="NCHW", out=None):
    """x_u8: CUDA uint8 ``[n,c,h,w]`` (``layout="NCHW"``) or ``[n,h,w,c]`` (``"NHWC"``); table: CPU int32 ``[n_out,6]`` rows
    ``{src, top, left, ch, cw, flip}`` -> CUDA uint8 ``[n_out,c,224,224]`` NCHW: crop ``src``'s rectangle, resample it
    bilinearly to 224x224 and mirror it (``va_resize_images_u8``), into ``out`` when given."""
    if not isinstance(x_u8, torch.Tensor) or not x_u8.is_cuda or x_u8.dtype != torch.uint8 or x_u8.dim() != 4:
        raise ValueError("resize_images: x must be a 4-d CUDA uint8 tensor")
    if layout == "NCHW":
        n, c, h, w = x_u8.shape
    elif layout == "NHWC":
        n, h, w, c = x_u8.shape
    else:
        raise ValueError("resize_images: layout must be 'NCHW' or 'NHWC', got %r" % (layout,))
    check_resize_table(table, n, h, w, "resize_images")
    n_out = table.shape[0]
    x_u8 = x_u8.contiguous()
    dev = x_u8.device
    if out is None:
        out = torch.empty((n_out, c, CROP_SIZE, CROP_SIZE), dtype=torch.uint8, device=dev)
    elif (out.numel() != n_out * c * CROP_SIZE * CROP_SIZE or out.dtype != torch.uint8 or not out.is_contiguous()
          or out.device != dev):
        raise ValueError("resize_images: out must be a contiguous uint8 tensor of %d elements on x's device"
                         % (n_out * c * CROP_SIZE * CROP_SIZE))
    dtable = crops_to_device(table, dev)
    _ffi.check(_ffi.lib().va_resize_images_u8(_ffi.ctx(dev.index), _ffi.ptr(x_u8), n, c, w, h, int(layout == "NHWC"),
                                              _ffi.ptr(dtable), n_out, _ffi.ptr(out), _ffi.stream_ptr(dev)))
    return out.view(n_out, c, CROP_SIZE, CROP_SIZE)


# ---- colour jitter and PCA lighting ----

IDENTITY_JITTER_ROW = (0, 0, 0, 0, 1.0, 1.0, 1.0, 0)  # no op; the factors of the identity blend, no shift


def _jitter_row(ops):
    """``[(op, value), ...]`` in application order (``utils.drawColorJitter``) -> one table row."""
    row = list(IDENTITY_JITTER_ROW)
    for k, (op, value) in enumerate(ops):
        row[k] = op
        row[3 + op if op != utils.JITTER_HUE else 7] = value
    return row


def draw_color_jitter(n, brightness, contrast, saturation, hue, rng=None):
    """The jitter of ``n`` images -> CPU float32 ``[n,8]`` rows ``{op0, op1, op2, op3, f_brightness, f_contrast,
    f_saturation, hue_shift}``: the op codes (0 none, 1 brightness, 2 contrast, 3 saturation, 4 hue) in application order,
    the blend factors as float32 (what PIL's blend computes with) and the integer hue shift.  Per image the draws of
    ``utils.ColorJitter`` (``utils.drawColorJitter``): nothing is drawn for all-zero parameters."""
    utils.checkColorJitter(brightness, contrast, saturation, hue)
    rng = random if rng is None else rng
    rows = [_jitter_row(utils.drawColorJitter(rng, brightness, contrast, saturation, hue)) for _ in range(int(n))]
    return torch.tensor(rows, dtype=torch.float32).view(int(n), 8)


def check_color_jitter(params, n, who="color_jitter"):
    """Host-side validation (ValueError) of a jitter table for ``n`` images, before anything reaches the GPU: CPU float32
    ``[n,8]``; op codes integers in 0..4, each op at most once in a row; finite factors >= 0; the shift an integer in
    0..255."""
    if not isinstance(params, torch.Tensor) or params.is_cuda or params.dtype != torch.float32:
        raise ValueError("%s: the jitter table must be a CPU float32 tensor (augment.draw_color_jitter)" % who)
    if params.dim() != 2 or tuple(params.shape) != (n, 8):
        raise ValueError("%s: the jitter table must be [%d,8], got %s" % (who, n, tuple(params.shape)))
    if not bool(torch.isfinite(params).all()):
        raise ValueError("%s: the jitter table holds a value that is not finite" % who)
    ops, fac, shift = params[:, :4], params[:, 4:7], params[:, 7]
    if bool((ops != ops.round()).any()) or bool((ops < 0).any()) or bool((ops > 4).any()):
        raise ValueError("%s: op codes must be integers in 0..4" % who)
    for op in (1, 2, 3, 4):
        if bool(((ops == op).sum(dim=1) > 1).any()):
            raise ValueError("%s: op %d appears twice in a row" % (who, op))
    if bool((fac < 0).any()):
        raise ValueError("%s: blend factors must be >= 0" % who)
    if bool((shift != shift.round()).any()) or bool((shift < 0).any()) or bool((shift > 255).any()):
        raise ValueError("%s: the hue shift must be an integer in 0..255" % who)


def check_lighting(lighting, n, who="color_jitter"):
    """ValueError unless ``lighting`` is a CPU float32 ``[n,3]`` tensor of finite offsets (``draw_lighting``)."""
    if (not isinstance(lighting, torch.Tensor) or lighting.is_cuda or lighting.dtype != torch.float32
            or tuple(lighting.shape) != (n, 3) or not bool(torch.isfinite(lighting).all())):
        raise ValueError("%s: lighting must be a finite CPU float32 [%d,3] tensor (augment.draw_lighting)" % (who, n))


def color_jitter(x_u8, params, lighting=None, out=None):
    """x_u8: CUDA uint8 ``[n,3,h,w]``; params: CPU float32 ``[n,8]`` (``draw_color_jitter``); lighting: CPU float32 ``[n,3]``
    channel offsets (``draw_lighting``) or None -> CUDA uint8 ``[n,3,h,w]``: every image through its own row, then the
    lighting (``va_color_jitter_u8``).  ``out`` may be ``x_u8`` itself (in place)."""
    if not isinstance(x_u8, torch.Tensor) or not x_u8.is_cuda or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[1] != 3:
        raise ValueError("color_jitter: x must be a CUDA uint8 [n,3,h,w] tensor")
    n, _, h, w = x_u8.shape
    check_color_jitter(params, n)
    if lighting is not None:
        check_lighting(lighting, n)
    if out is x_u8:
        if not x_u8.is_contiguous():
            raise ValueError("color_jitter: in place needs a contiguous x")
    else:
        x_u8 = x_u8.contiguous()
    dev = x_u8.device
    if out is None:
        out = torch.empty_like(x_u8)
    elif out.numel() != x_u8.numel() or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev:
        raise ValueError("color_jitter: out must be a contiguous uint8 tensor of %d elements on x's device" % x_u8.numel())
    dparams = crops_to_device(params, dev)
    dlight = crops_to_device(lighting, dev) if lighting is not None else None
    # the partial sums of the gray level live in a workspace of this call (stream-ordered: the allocator hands the block
    # out again only to work enqueued after launch two); no row with contrast: no workspace, one launch
    work = None
    if bool((params[:, :4] == utils.JITTER_CONTRAST).any()):
        work = torch.empty((n, _ffi.VA_COLOR_JITTER_PARTIALS), dtype=torch.int32, device=dev)
    _ffi.check(_ffi.lib().va_color_jitter_u8(_ffi.ctx(dev.index), _ffi.ptr(x_u8), n, w, h, _ffi.ptr(dparams), _ffi.ptr(dlight),
                                             _ffi.ptr(out), _ffi.ptr(work), _ffi.stream_ptr(dev)))
    return out.view(n, 3, h, w)


def draw_image_transforms(n, h, w, jitter, size=CROP_SIZE, rng=None):
    """The draws of ``utils.getTransforms(jitter=jitter)`` for ``n`` images of ``h x w`` pixels, image by image in its order
    (crop, flip, jitter) -> ``(crops [n,3], params [n,8])`` for ``crop_images`` and ``color_jitter``: a seeded host
    transform and the two device calls see the same numbers."""
    _check_frame(h, w, size, "draw_image_transforms")
    b, c, s, hue = jitter if jitter else (0, 0, 0, 0)
    utils.checkColorJitter(b, c, s, hue)
    rng = random if rng is None else rng
    crops, rows = [], []
    for _ in range(int(n)):
        crops.append(_draw(rng, h, w, size))
        rows.append(_jitter_row(utils.drawColorJitter(rng, b, c, s, hue)))
    return torch.tensor(crops, dtype=torch.int32).view(int(n), 3), torch.tensor(rows, dtype=torch.float32).view(int(n), 8)


def rgb_pca(frames_u8):
    """The PCA of the RGB values of ``frames_u8``, uint8 ``[..., 3, h, w]`` on any device -> ``(eigval [3], eigvec [3,3])``,
    CPU float64, ``torch.linalg.eigh`` of the 3x3 covariance (over all N pixels, divided by N) in u8 units: ascending
    eigenvalues, eigenvector j in column j.  The sums of values and of products are exact integers (int64, accumulated
    with torch on the frames' device); the covariance is formed from them once."""
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() < 3 or frames_u8.shape[-3] != 3:
        raise ValueError("rgb_pca: frames must be a uint8 [...,3,h,w] tensor")
    x = frames_u8.reshape(-1, 3, frames_u8.shape[-2] * frames_u8.shape[-1])
    N = x.shape[0] * x.shape[2]
    if N < 1:
        raise ValueError("rgb_pca: no pixels")
    ch = [x[:, c].to(torch.int64) for c in range(3)]
    s1 = [int(c.sum()) for c in ch]
    cov = torch.empty((3, 3), dtype=torch.float64)
    for i in range(3):
        for j in range(i, 3):
            s2 = int((ch[i] * ch[j]).sum())
            cov[i, j] = cov[j, i] = (s2 * N - s1[i] * s1[j]) / (N * N)  # exact integers, one rounding
    return torch.linalg.eigh(cov)


def draw_lighting(n, eigval, eigvec, alphastd=0.1, rng=None):
    """AlexNet's PCA lighting noise for ``n`` images -> CPU float32 ``[n,3]`` channel offsets
    ``eigvec @ (alpha * eigval)``, ``alpha_j = rng.gauss(0, alphastd)`` drawn in j order per image; computed in float64
    and rounded to float32 once.  ``eigval [3]``, ``eigvec [3,3]`` (column j the j-th eigenvector): ``rgb_pca``."""
    rng = random if rng is None else rng
    ev = torch.as_tensor(eigval, dtype=torch.float64).reshape(3)
    evec = torch.as_tensor(eigvec, dtype=torch.float64).reshape(3, 3)
    alpha = torch.tensor([[rng.gauss(0, alphastd) for _ in range(3)] for _ in range(int(n))], dtype=torch.float64).view(int(n), 3)
    return ((alpha * ev) @ evec.t()).to(torch.float32).contiguous()
