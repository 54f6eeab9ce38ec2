"""Dense optical flow on MI355X by three methods (TV-L1, Brox, Farneback): host wrappers over ``va_tvl1_flow_opt``,
``va_brox_flow`` and ``va_farneback_flow``, and over what consumes their result (``va_flow_to_stack`` and its kin).

The reference never computes flow; it reads the ``flow_x_%04d.jpg`` / ``flow_y_%04d.jpg`` images of
an upstream TV-L1 tool (Sheet03/temporalModel.py:76-81, Sheet03/parameters.py:27,38-39).  These
functions are that tool, re-built for gfx950, producing directly the ``[2L,H,W]`` flow volume that
``TemporalDataset.__getitem__`` assembles (Sheet03/temporalModel.py:83-90).
"""
import collections
import ctypes

import torch

from . import _ffi
from .parameters import NORM_MEANS_TF, NORM_STDS_TF

FLOW_BOUND = 20.0  # 8-bit flow image convention: [-bound, bound] -> [0, 255]

_ws_cache = {}


def _workspace(nbytes, device, slot=0):
    """Grow-only per-device workspace (256-byte aligned by the torch caching allocator)."""
    key = (device.index, "tvl1", slot)
    t = _ws_cache.get(key)
    if t is None or t.numel() < nbytes:
        _ws_cache[key] = t = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return t


def release_workspaces():
    _ws_cache.clear()


def release_workspace(slot, device):
    """Drop one TV-L1 workspace slot of ``device`` (its owner has synchronised the stream that used it)."""
    _ws_cache.pop((device.index, "tvl1", slot), None)


# One row per flow method, all that _flow and pyramid_sizes know of it: the public function's name (it heads every message),
# the parameter class and its defaults, the two C entry points, whether the method has TV-L1's options (S55: they travel
# beside the parameters, and ``lambda`` is taken as ``lambda_``), whether ``params`` together with keyword overrides is
# refused (else the overrides are ignored), and the names of the fields that shape the pyramid.
_Method = collections.namedtuple("_Method", "who params defaults workspace_bytes flow tvl1_options refuses_both step levels")
_METHODS = (
    _Method("tvl1_flow", _ffi.Tvl1Params, _ffi.default_tvl1_params, "va_tvl1_workspace_bytes_opt", "va_tvl1_flow_opt",
            True, False, "scale_step", "nscales"),
    _Method("brox_flow", _ffi.BroxParams, _ffi.default_brox_params, "va_brox_workspace_bytes", "va_brox_flow",
            False, False, "scale_step", "nscales"),
    _Method("farneback_flow", _ffi.FarnebackParams, _ffi.default_farneback_params, "va_farneback_workspace_bytes", "va_farneback_flow",
            False, True, "pyr_scale", "levels"),
)
_TVL1, _BROX, _FARNEBACK = _METHODS


def _flow(m, frames, params, ws_slot, out, over):
    """The call the three public functions share: frames, parameters, workspace, ``out``, the library."""
    who = m.who
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise ValueError("%s: frames must be a CUDA tensor" % who)
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.dim() != 4:
        raise ValueError("%s: frames must be [S,F,H,W] or [F,H,W]" % who)
    if frames.dtype not in (torch.uint8, torch.float32):
        raise ValueError("%s: frames must be uint8 or float32" % who)
    if not m.tvl1_options:
        _refuse_median(params, over, who)
    frames = frames.contiguous()
    S, F, H, W = frames.shape
    p = params if params is not None else m.defaults(**over)
    if not m.tvl1_options and not isinstance(p, m.params):
        raise ValueError("%s: params must be an _ffi.%s" % (who, m.params.__name__))
    if m.refuses_both and params is not None and over:
        raise ValueError("%s: pass a %s or keyword overrides, not both" % (who, m.params.__name__))
    L = _ffi.lib()
    c = _ffi.ctx(frames.device.index)
    args = (ctypes.byref(p),)
    if m.tvl1_options:  # (S55: the median of the flow between blocks of inner iterations; NULL when no option is set)
        opt = _ffi.tvl1_options(p)
        args += (ctypes.byref(opt) if opt is not None else None,)
    nbytes = getattr(L, m.workspace_bytes)(W, H, S, F, *args)
    if nbytes == 0:
        raise ValueError(_ffi.last_error())
    ws = _workspace(nbytes, frames.device, ws_slot)
    if out is None:
        flow = torch.empty((S * (F - 1), 2, H, W), dtype=torch.float32, device=frames.device)
    else:
        flow = out
        if (tuple(flow.shape) != (S * (F - 1), 2, H, W) or flow.dtype != torch.float32 or flow.device != frames.device
                or not flow.is_contiguous()):
            raise ValueError("%s: out must be a contiguous float32 [%d,2,%d,%d] tensor on the frames' device" % (who, S * (F - 1), H, W))
    _ffi.check(getattr(L, m.flow)(c, _ffi.ptr(frames), int(frames.dtype == torch.uint8), S, F, W, H, *args,
                                  _ffi.ptr(flow), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(frames.device)))
    return flow


def tvl1_flow(frames, params=None, ws_slot=0, out=None, **over):
    """frames: cuda uint8 or float32 tensor ``[S, F, H, W]`` (or ``[F, H, W]``), gray values in [0,255].

    Returns float32 ``[S*(F-1), 2, H, W]`` (written into ``out`` when given): plane 0 = x flow, plane 1 = y
    flow of every consecutive frame pair.  ``params``: ``_ffi.Tvl1Params`` or keyword overrides (tau, lambda_, theta, nscales,
    warps, epsilon, iters, scale_step, block_iters).  ``lambda`` is a Python keyword: pass it as ``lambda_=0.1`` (or as
    ``**{"lambda": 0.1}``, which is taken as the same field).  Parameters out of range (``va_tvl1_params`` in include/va.h)
    raise ValueError.

    ``params`` may also be an ``_ffi.BroxParams``: the call is then ``brox_flow``'s, so that everything
    built on this function -- ``tvl1_flow_concurrent``, ``rerun_camera``'s second pass, ``flowVolumesFromFrames`` and
    ``TwoStreamPipeline`` with their ``tvl1_params`` -- computes Brox flow when it is handed one.  An
    ``_ffi.FarnebackParams`` does the same for ``farneback_flow``.
    """
    for m in (_BROX, _FARNEBACK):
        if isinstance(params, m.params):
            return _flow(m, frames, params, ws_slot, out, over)
    return _flow(_TVL1, frames, params, ws_slot, out, over)


def brox_flow(frames, params=None, ws_slot=0, out=None, **over):
    """Brox optical flow (``va_brox_flow``), the two-stream paper's own method: frames, result, ``out``
    and ``ws_slot`` as ``tvl1_flow`` has them (the two methods share the workspace slots).  ``params``: ``_ffi.BroxParams`` or
    keyword overrides (alpha, gamma, scale_step, omega, epsilon, nscales, warps, inner_iters, solver_iters).  Parameters out
    of range (``va_brox_params`` in include/va.h) raise ValueError; so does the median option of TV-L1 (S55), which this
    method does not have."""
    return _flow(_BROX, frames, params, ws_slot, out, over)


def farneback_flow(frames, params=None, ws_slot=0, out=None, **over):
    """Farneback optical flow (``va_farneback_flow``), the direct method of the three: frames, result,
    ``out`` and ``ws_slot`` as ``tvl1_flow`` has them (the three methods share the workspace slots).  ``params``:
    ``_ffi.FarnebackParams`` or keyword overrides (pyr_scale, poly_sigma, levels, winsize, iterations, poly_n, gaussian).
    Parameters out of range (``va_farneback_params`` in include/va.h) raise ValueError; so does the median option of TV-L1
    (S55), which this method does not have."""
    return _flow(_FARNEBACK, frames, params, ws_slot, out, over)


def _refuse_median(params, over, who):
    if "median" in over or "median_every" in over or getattr(params, "median", 0) or getattr(params, "median_every", 0):
        raise ValueError("%s: median and median_every are options of TV-L1 (S55); %s flow has no median filter"
                         % (who, who.split("_")[0].capitalize()))


def _tvl1_only(params, who):
    for m in (_BROX, _FARNEBACK):
        if isinstance(params, m.params):
            raise ValueError("%s: describes TV-L1's kernels and takes an _ffi.Tvl1Params, not a %s" % (who, m.params.__name__))


def median_filter(flow, ksize=5, out=None):
    """The filter of DESIGN.md S55 on stored flow (``va_flow_median``): flow ``[N,2,H,W]`` CUDA float32 -> the same shape,
    every plane replaced by its ``ksize`` x ``ksize`` median (3 or 5; window clamped to the plane, exact selection).
    ``out`` must not overlap ``flow``."""
    _check_flow(flow, "median_filter")
    flow = flow.contiguous()
    N, _, H, W = flow.shape
    out = _check_out(out, (N, 2, H, W), flow, "median_filter")
    _ffi.check(_ffi.lib().va_flow_median(_ffi.ctx(flow.device.index), _ffi.ptr(flow), N, W, H, int(ksize), _ffi.ptr(out),
                                         _ffi.stream_ptr(flow.device)))
    return out


_streams = {}


def flow_streams(device, n):
    """The ``n`` HIGH-priority HIP streams TV-L1 calls are spread over on ``device`` (created once): their launches
    are dispatched ahead of whatever runs beside them (the CNN stream of pipeline.py has normal priority)."""
    key = (device.index, n)
    if key not in _streams:
        _streams[key] = [torch.cuda.Stream(device=device, priority=-1) for _ in range(n)]
    return _streams[key]


def tvl1_flow_concurrent(frames, params=None, n_streams=2, out=None, after=None, join=True):
    """Same result as ``tvl1_flow`` for ``[S,F,H,W]`` frames (``params``: a ``Tvl1Params`` or a ``BroxParams``), with the sequences split into ``n_streams``
    groups that run on separate HIP streams (each with its own workspace).  Kernels of the groups
    then overlap on the GPU: the un-overlapped HBM round trips and partial last rounds of one
    group's tile launches are filled by the other's (measured +10 % at 320 pairs).

    ``after``: a CUDA event (or a list of events) the group streams wait for instead of the current stream (the frames -- and ``out`` --
    are ready when it fires).  ``join=False``: the current stream does NOT wait for the groups; the call returns
    ``(flow, events)`` with one event per group stream (pipeline.py chains the consumer on them, so that the next
    batch's TV-L1 can be enqueued behind this one without waiting for this batch's consumers)."""
    if frames.dim() != 4:
        raise ValueError("tvl1_flow_concurrent: frames must be [S,F,H,W]")
    S = frames.shape[0]
    n = max(1, min(int(n_streams), S))
    dev = frames.device
    F = frames.shape[1]
    if n == 1 and after is None and join:
        return tvl1_flow(frames, params, out=out)
    streams = flow_streams(dev, n)
    cur = torch.cuda.current_stream(dev)
    bounds = [(S * i) // n for i in range(n + 1)]
    if out is None:
        flow = torch.empty((S * (F - 1), 2, frames.shape[2], frames.shape[3]), dtype=torch.float32, device=dev)
    else:
        flow = out
        if tuple(flow.shape) != (S * (F - 1), 2, frames.shape[2], frames.shape[3]) or flow.dtype != torch.float32 or not flow.is_contiguous():
            raise ValueError("tvl1_flow_concurrent: out must be a contiguous float32 [%d,2,%d,%d] tensor" % (S * (F - 1), frames.shape[2], frames.shape[3]))
    events = []
    for i, st in enumerate(streams):
        if after is None:
            st.wait_stream(cur)
        else:
            for ev in (after if isinstance(after, (list, tuple)) else [after]):
                if ev is not None:
                    st.wait_event(ev)
        with torch.cuda.stream(st):
            part = frames[bounds[i]:bounds[i + 1]]
            part.record_stream(st)
            flow.record_stream(st)
            tvl1_flow(part, params, ws_slot=i + 1, out=flow[bounds[i] * (F - 1):bounds[i + 1] * (F - 1)])
            if not join:
                ev = torch.cuda.Event()
                ev.record(st)
                events.append(ev)
    if not join:
        return flow, events
    for st in streams:
        cur.wait_stream(st)
    return flow


def flow_to_stack(flow, bound=FLOW_BOUND, mean=NORM_MEANS_TF[0], std=NORM_STDS_TF[0], out=None):
    """flow ``[N,2,H,W]`` float32 -> ``[2N,H,W]`` float32 flow volume: 8-bit quantisation, ToTensor,
    Normalize with the single-channel rule (mean 0.485 / std 0.229: Sheet03/utils.py:148-150,
    SURVEY.md a5), channels interleaved x,y (Sheet03/temporalModel.py:83)."""
    if not isinstance(flow, torch.Tensor) or not flow.is_cuda or flow.dtype != torch.float32:
        raise ValueError("flow_to_stack: flow must be a CUDA float32 tensor")
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError("flow_to_stack: flow must be [N,2,H,W]")
    flow = flow.contiguous()
    N, _, H, W = flow.shape
    if out is None:
        out = torch.empty((2 * N, H, W), dtype=torch.float32, device=flow.device)
    elif out.numel() != 2 * N * H * W or out.dtype != torch.float32 or not out.is_contiguous() or out.device != flow.device:
        raise ValueError("flow_to_stack: out must be a contiguous float32 tensor of %d elements on the flow's device" % (2 * N * H * W))
    _ffi.check(_ffi.lib().va_flow_to_stack(_ffi.ctx(flow.device.index), _ffi.ptr(flow), N, W, H, float(bound),
                                           float(mean), float(std), _ffi.ptr(out), _ffi.stream_ptr(flow.device)))
    return out


def _check_flow(flow, who):
    if not isinstance(flow, torch.Tensor) or not flow.is_cuda or flow.dtype != torch.float32:
        raise ValueError("%s: flow must be a CUDA float32 tensor" % who)
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError("%s: flow must be [N,2,H,W]" % who)


def _check_out(out, shape, flow, who):
    n = 1
    for k in shape:
        n *= k
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=flow.device)
    if out.numel() != n or out.dtype != torch.float32 or not out.is_contiguous() or out.device != flow.device:
        raise ValueError("%s: out must be a contiguous float32 tensor of %d elements on the flow's device" % (who, n))
    return out


def _views_call(flow, dcrops, n_clips, flow_count, n_views, invert, size, bound, mean, std, out):
    N, _, H, W = flow.shape
    _ffi.check(_ffi.lib().va_flow_to_stack_views(_ffi.ctx(flow.device.index), _ffi.ptr(flow), n_clips, flow_count, n_views, W,
                                                 H, float(bound), float(mean), float(std), _ffi.ptr(dcrops), int(bool(invert)),
                                                 size, size, _ffi.ptr(out), _ffi.stream_ptr(flow.device)))


def crop_flow_to_stack(flow, crops, size=224, bound=FLOW_BOUND, mean=NORM_MEANS_TF[0], std=NORM_STDS_TF[0], out=None,
                       invert_x_on_flip=False):
    """``flow_to_stack`` of full-size flow with one crop and flip per output channel (then S9): flow
    ``[N,2,H,W]`` float32 (H, W >= ``size``), crops CPU int32 ``[2N,3]`` rows ``{top, left, flip}`` (row 2k: the x flow of
    pair k; ``augment.draw_flow_crops``) -> ``[2N,size,size]`` float32.  Only the crop windows are read.

    ``invert_x_on_flip``: a flipped x-flow image also becomes ``q -> 255 - q`` (TSN flips: mirroring reverses horizontal
    motion); the default mirrors without inverting, as the reference does."""
    from . import augment
    _check_flow(flow, "crop_flow_to_stack")
    N, _, H, W = flow.shape
    augment.check_crops(crops, 2 * N, H, W, size, "crop_flow_to_stack")
    flow = flow.contiguous()
    out = _check_out(out, (2 * N, size, size), flow, "crop_flow_to_stack")
    dcrops = augment.crops_to_device(crops, flow.device)
    if invert_x_on_flip:  # one "clip" of N pairs seen through one view: the crop table has one row per output plane
        _views_call(flow, dcrops, 1, N, 1, True, size, bound, mean, std, out)
        return out
    _ffi.check(_ffi.lib().va_flow_to_stack_crop(_ffi.ctx(flow.device.index), _ffi.ptr(flow), N, W, H, float(bound),
                                                float(mean), float(std), _ffi.ptr(dcrops), size, size, _ffi.ptr(out),
                                                _ffi.stream_ptr(flow.device)))
    return out


def crop_flow_to_stack_views(flow, views, flow_count, invert_x_on_flip=False, size=224, bound=FLOW_BOUND,
                             mean=NORM_MEANS_TF[0], std=NORM_STDS_TF[0], out=None):
    """Ten-crop flow volumes: flow ``[B*L,2,H,W]`` float32 of B clips of ``flow_count`` = L pairs, views
    CPU int32 ``[V,3]`` (``augment.ten_crop_views``) -> ``[B,V,2L,size,size]`` float32: every flow image of every clip
    seen through every view, quantised and normalised as ``crop_flow_to_stack``.  ``invert_x_on_flip``: TSN flips (a
    mirrored x-flow image becomes ``q -> 255 - q``); the default mirrors without inverting."""
    from . import augment
    _check_flow(flow, "crop_flow_to_stack_views")
    N, _, H, W = flow.shape
    L = int(flow_count)
    if L < 1 or N % L:
        raise ValueError("crop_flow_to_stack_views: %d flow pairs are not a whole number of clips of %d" % (N, L))
    augment.check_views(views, H, W, size, "crop_flow_to_stack_views")
    B, V = N // L, views.shape[0]
    flow = flow.contiguous()
    out = _check_out(out, (B, V, 2 * L, size, size), flow, "crop_flow_to_stack_views")
    dcrops = augment.crops_to_device(augment.expand_views(views, B, 2 * L), flow.device)
    _views_call(flow, dcrops, B, L, V, invert_x_on_flip, size, bound, mean, std, out)
    return out.view(B, V, 2 * L, size, size)


def check_starts(starts, n_pairs, flow_count, who):
    """Host-side validation (ValueError) of snippet starts for ``n_pairs`` flow fields: a CPU int32 ``[n]`` tensor (or a
    list of ints) with n >= 1 and every start in [0, n_pairs - flow_count] -> the CPU int32 tensor."""
    if not isinstance(starts, torch.Tensor):
        try:
            starts = torch.tensor([int(s) for s in starts], dtype=torch.int32)
        except (TypeError, ValueError):
            raise ValueError("%s: starts must be a CPU int32 [n] tensor or a list of ints" % who)
    if starts.is_cuda or starts.dtype != torch.int32 or starts.dim() != 1 or starts.shape[0] < 1:
        raise ValueError("%s: starts must be a CPU int32 [n] tensor with n >= 1" % who)
    if n_pairs < flow_count or bool((starts < 0).any()) or bool((starts > n_pairs - flow_count).any()):
        raise ValueError("%s: a window of %d pairs starting at %d..%d does not lie in the %d flow fields"
                         % (who, flow_count, int(starts.min()), int(starts.max()), n_pairs))
    return starts


def crop_flow_to_stack_snippets(flow, starts, views, flow_count, invert_x_on_flip=False, size=224, bound=FLOW_BOUND,
                                mean=NORM_MEANS_TF[0], std=NORM_STDS_TF[0], out=None):
    """The flow volumes of the snippets of one video: flow ``[N,2,H,W]`` float32, the video's flow fields
    each computed once; starts CPU int32 ``[n]`` (or a list), snippet s being the ``flow_count`` = L fields from
    ``starts[s]`` on (windows may overlap and repeat); views CPU int32 ``[V,3]`` -> ``[n,V,2L,size,size]`` float32,
    quantised and normalised as ``crop_flow_to_stack_views``: with ``starts = [0, L, 2L, ...]`` the same bits."""
    from . import augment
    _check_flow(flow, "crop_flow_to_stack_snippets")
    N, _, H, W = flow.shape
    L = int(flow_count)
    if L < 1:
        raise ValueError("crop_flow_to_stack_snippets: flow_count must be >= 1, got %d" % L)
    starts = check_starts(starts, N, L, "crop_flow_to_stack_snippets")
    augment.check_views(views, H, W, size, "crop_flow_to_stack_snippets")
    n, V = starts.shape[0], views.shape[0]
    flow = flow.contiguous()
    out = _check_out(out, (n, V, 2 * L, size, size), flow, "crop_flow_to_stack_snippets")
    dcrops = augment.crops_to_device(augment.expand_views(views, n, 2 * L), flow.device)
    dstarts = augment.crops_to_device(starts, flow.device)
    _ffi.check(_ffi.lib().va_flow_to_stack_snippets(_ffi.ctx(flow.device.index), _ffi.ptr(flow), N, _ffi.ptr(dstarts), n, L, V,
                                                    W, H, float(bound), float(mean), float(std), _ffi.ptr(dcrops),
                                                    int(bool(invert_x_on_flip)), size, size, _ffi.ptr(out),
                                                    _ffi.stream_ptr(flow.device)))
    return out.view(n, V, 2 * L, size, size)


def resize_flow_to_stack(flow, table, invert_x_on_flip=False, bound=FLOW_BOUND, mean=NORM_MEANS_TF[0], std=NORM_STDS_TF[0],
                         out=None):
    """The crop-resize gather of flow (then S9; ``va_flow_to_stack_resize``): flow ``[N,2,H,W]`` float32 (or
    an S11-S13 motion field of that shape), table CPU int32 ``[n_out,6]`` rows ``{src, top, left, ch, cw, flip}`` with
    ``src`` one of the 2N planes (``augment.snippet_tables``) -> ``[n_out,224,224]`` float32: the float field is resampled
    bilinearly inside the crop, then quantised and normalised once as ``flow_to_stack``.  ``invert_x_on_flip``: a flipped
    plane with an even ``src`` (x flow) also becomes ``q -> 255 - q`` (TSN flips)."""
    from . import augment
    _check_flow(flow, "resize_flow_to_stack")
    N, _, H, W = flow.shape
    augment.check_resize_table(table, 2 * N, H, W, "resize_flow_to_stack")
    n_out = table.shape[0]
    flow = flow.contiguous()
    out = _check_out(out, (n_out, 224, 224), flow, "resize_flow_to_stack")
    dtable = augment.crops_to_device(table, flow.device)
    _ffi.check(_ffi.lib().va_flow_to_stack_resize(_ffi.ctx(flow.device.index), _ffi.ptr(flow), N, W, H, float(bound),
                                                  float(mean), float(std), _ffi.ptr(dtable), n_out,
                                                  int(bool(invert_x_on_flip)), _ffi.ptr(out), _ffi.stream_ptr(flow.device)))
    return out.view(n_out, 224, 224)


# ---- stored optical flow ----
#
# The flow of a video, computed once and kept on the device: ``[T-1,2,H,W]``, field t the flow from frame t to frame t+1,
# as float32 (TV-L1's own output) or as uint8, the 8-bit flow images of S9 that TSN and the reference's JPEGs hold.  The
# float32 form goes through the gathers above; the uint8 form through the two below.

def _check_flowq(flowq, who):
    if not isinstance(flowq, torch.Tensor) or not flowq.is_cuda or flowq.dtype != torch.uint8:
        raise ValueError("%s: flowq must be a CUDA uint8 tensor (quantize_flow)" % who)
    if flowq.dim() != 4 or flowq.shape[1] != 2:
        raise ValueError("%s: flowq must be [N,2,H,W]" % who)


def quantize_flow(flow, bound=FLOW_BOUND, out=None):
    """S39: flow ``[N,2,H,W]`` CUDA float32 -> uint8 of the same shape (into ``out`` when given), the 8-bit flow images
    ``q = rint(clamp(255*(v+bound)/(2*bound), 0, 255))`` every flow gather forms (``utils.flowToImages`` on the device; a NaN
    becomes 0)."""
    _check_flow(flow, "quantize_flow")
    try:
        bound = float(bound)
    except (TypeError, ValueError):
        raise ValueError("quantize_flow: bound must be a number")
    if not 0.0 < bound < float("inf"):
        raise ValueError("quantize_flow: bound must be finite and > 0, got %r" % bound)
    N, _, H, W = flow.shape
    if N < 1 or H < 1 or W < 1:
        raise ValueError("quantize_flow: empty flow %s" % (tuple(flow.shape),))
    flow = flow.contiguous()
    if out is None:
        out = torch.empty((N, 2, H, W), dtype=torch.uint8, device=flow.device)
    elif (not isinstance(out, torch.Tensor) or out.numel() != flow.numel() or out.dtype != torch.uint8 or not out.is_contiguous()
          or out.device != flow.device):
        raise ValueError("quantize_flow: out must be a contiguous uint8 tensor of %d elements on the flow's device" % flow.numel())
    _ffi.check(_ffi.lib().va_flow_quantize_u8(_ffi.ctx(flow.device.index), _ffi.ptr(flow), N, W, H, bound, _ffi.ptr(out),
                                              _ffi.stream_ptr(flow.device)))
    return out.view(N, 2, H, W)


def flowq_to_stack_snippets(flowq, starts, views, flow_count, invert_x_on_flip=False, size=224, mean=NORM_MEANS_TF[0],
                            std=NORM_STDS_TF[0], out=None):
    """S40, ``crop_flow_to_stack_snippets`` of a uint8 stored flow: flowq ``[N,2,H,W]`` CUDA uint8 (``quantize_flow``), starts
    and views as there -> ``[n,V,2L,size,size]`` float32.  On ``quantize_flow(flow)`` it gives the bits
    ``crop_flow_to_stack_snippets(flow)`` gives."""
    from . import augment
    _check_flowq(flowq, "flowq_to_stack_snippets")
    N, _, H, W = flowq.shape
    L = int(flow_count)
    if L < 1:
        raise ValueError("flowq_to_stack_snippets: flow_count must be >= 1, got %d" % L)
    starts = check_starts(starts, N, L, "flowq_to_stack_snippets")
    augment.check_views(views, H, W, size, "flowq_to_stack_snippets")
    n, V = starts.shape[0], views.shape[0]
    flowq = flowq.contiguous()
    out = _check_out(out, (n, V, 2 * L, size, size), flowq, "flowq_to_stack_snippets")
    dcrops = augment.crops_to_device(augment.expand_views(views, n, 2 * L), flowq.device)
    dstarts = augment.crops_to_device(starts, flowq.device)
    _ffi.check(_ffi.lib().va_flowq_to_stack_snippets(_ffi.ctx(flowq.device.index), _ffi.ptr(flowq), N, _ffi.ptr(dstarts), n, L, V,
                                                     W, H, float(mean), float(std), _ffi.ptr(dcrops),
                                                     int(bool(invert_x_on_flip)), size, size, _ffi.ptr(out),
                                                     _ffi.stream_ptr(flowq.device)))
    return out.view(n, V, 2 * L, size, size)


def resize_flowq_to_stack(flowq, table, invert_x_on_flip=False, mean=NORM_MEANS_TF[0], std=NORM_STDS_TF[0], out=None):
    """S41, the crop-resize gather of a uint8 stored flow in TSN's order: flowq ``[N,2,H,W]`` CUDA uint8, table as
    ``resize_flow_to_stack`` takes it -> ``[n_out,224,224]`` float32.  The 8-bit IMAGE is resampled (to the value
    ``augment.resize_images`` gives for the plane), then inverted and normalised; at ``ch = cw = 224`` that is the plain
    crop of ``flowq_to_stack_snippets``, at other sizes it is not ``resize_flow_to_stack`` of the float field."""
    from . import augment
    _check_flowq(flowq, "resize_flowq_to_stack")
    N, _, H, W = flowq.shape
    augment.check_resize_table(table, 2 * N, H, W, "resize_flowq_to_stack")
    n_out = table.shape[0]
    flowq = flowq.contiguous()
    out = _check_out(out, (n_out, 224, 224), flowq, "resize_flowq_to_stack")
    dtable = augment.crops_to_device(table, flowq.device)
    _ffi.check(_ffi.lib().va_flowq_to_stack_resize(_ffi.ctx(flowq.device.index), _ffi.ptr(flowq), N, W, H, float(mean),
                                                   float(std), _ffi.ptr(dtable), n_out, int(bool(invert_x_on_flip)),
                                                   _ffi.ptr(out), _ffi.stream_ptr(flowq.device)))
    return out.view(n_out, 224, 224)


def check_stored_flow(flow, n_frames, h, w, who):
    """Host-side validation (ValueError; nothing is enqueued) of a stored flow for a video of ``n_frames`` frames of
    ``h x w`` pixels, short of its device: a contiguous uint8 or float32 ``[n_frames-1,2,h,w]`` tensor."""
    if not isinstance(flow, torch.Tensor) or flow.dtype not in (torch.uint8, torch.float32) or flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError("%s: a stored flow must be a uint8 or float32 [T-1,2,H,W] tensor (extract_flow)" % who)
    if not flow.is_contiguous():
        raise ValueError("%s: a stored flow must be contiguous" % who)
    if flow.shape[0] != n_frames - 1:
        raise ValueError("%s: %d frames need %d stored flow fields, got %d" % (who, n_frames, n_frames - 1, flow.shape[0]))
    if tuple(flow.shape[2:]) != (h, w):
        raise ValueError("%s: the stored flow is %dx%d but the frames are %dx%d" % (who, flow.shape[3], flow.shape[2], w, h))


# The temporal-ConvNet inputs of the two-stream paper: "stack" is optical-flow stacking (the default and
# the reference's input), "trajectory" samples the flow along the trajectory that starts at each pixel of the first frame,
# "bidirectional" stacks L/2 forward fields from the clip's centre frame on and L/2 backward ones from it back.
MOTIONS = ("stack", "trajectory", "bidirectional")


# Camera compensation of the flow: "homography" is TSN's warped optical flow, every field minus the
# displacement field of the homography fitted to it (or, with camera_form="rerun", TV-L1 of the pair warped by it: S53, S54);
# it comes before the motion options above, which then see the compensated field in place of the TV-L1 output.
CAMERAS = ("none", "homography")


def check_camera(camera, who):
    if not isinstance(camera, str) or camera not in CAMERAS:
        raise ValueError("%s: camera must be one of %s, got %r" % (who, ", ".join(CAMERAS), camera))


# The two forms of "homography" (DESIGN.md S22, S54): "subtract" takes the camera's displacement field from the TV-L1 field
# (S22, one TV-L1 pass, exact where that field is); "rerun" is TSN's own definition: the second frame of every pair is
# warped by the fitted homography (S53) and TV-L1 runs again on the pair, so that the residual motion is estimated directly.
CAMERA_FORMS = ("subtract", "rerun")
RERUN_WS_SLOT = "rerun"  # the second pass's TV-L1 workspace: never slot 0 or one of the flow streams' slots 1..n


def check_camera_form(camera_form, who, camera="homography"):
    """Host-side check (ValueError) of ``camera_form`` (``CAMERA_FORMS``) beside its ``camera``: an unknown form, and
    ``"rerun"`` without a camera to compensate."""
    if not isinstance(camera_form, str) or camera_form not in CAMERA_FORMS:
        raise ValueError("%s: camera_form must be one of %s, got %r" % (who, ", ".join(CAMERA_FORMS), camera_form))
    if camera_form == "rerun" and camera == "none":
        raise ValueError("%s: camera_form='rerun' needs camera='homography'; with camera='none' there is nothing to run again"
                         % who)


def check_motion(motion, mean_flow, flow_count, who, camera="none"):
    """Host-side checks of the motion options, before anything is enqueued: an unknown motion, trajectory stacking of
    bi-directional flow (the paper does not combine them), bi-directional flow of an odd L and an unknown camera raise
    ValueError."""
    check_camera(camera, who)
    parts = motion.split("+") if isinstance(motion, str) else list(motion) if isinstance(motion, (tuple, list)) else []
    if "trajectory" in parts and "bidirectional" in parts:
        raise ValueError("%s: trajectory stacking of bi-directional flow is not offered (the two-stream paper does not "
                         "combine them)" % who)
    if not isinstance(motion, str) or motion not in MOTIONS:
        raise ValueError("%s: motion must be one of %s, got %r" % (who, ", ".join(MOTIONS), motion))
    if motion == "bidirectional" and (flow_count < 2 or flow_count % 2):
        raise ValueError("%s: bi-directional flow needs an even number of flow pairs, got %d" % (who, flow_count))
    if not isinstance(mean_flow, bool):
        raise ValueError("%s: mean_flow must be True or False" % who)


def bidirectional_sequences(gray):
    """Bi-directional flow's TV-L1 input: gray ``[B,L+1,H,W]`` (L even; frame L/2 is tau) ->
    ``[2B,L/2+1,H,W]``, per clip the forward sequence ``(f_{L/2}, ..., f_L)`` and then the backward one
    ``(f_{L/2}, f_{L/2-1}, ..., f_0)``.  TV-L1 of it gives per clip L/2 forward fields tau+k -> tau+k+1 and then L/2
    backward fields tau-j -> tau-j-1: L pairs in the usual ``[B*L,2,H,W]`` layout.  Plain indexing (CPU tensors too)."""
    if not isinstance(gray, torch.Tensor) or gray.dim() != 4:
        raise ValueError("bidirectional_sequences: gray must be a [B,L+1,H,W] tensor")
    B, F, H, W = gray.shape
    L = F - 1
    if L < 2 or L % 2:
        raise ValueError("bidirectional_sequences: bi-directional flow needs an even number of flow pairs, got %d" % L)
    h = L // 2
    idx = torch.stack([torch.arange(h, L + 1), torch.arange(h, -1, -1)]).to(gray.device)  # [2, L/2+1]
    return gray[:, idx].reshape(2 * B, h + 1, H, W)


def flow_field_means(flow, out=None):
    """S11: flow ``[N,2,H,W]`` float32 -> ``[N,2]`` float32, the mean vector of every displacement field over the full
    frame, summed as exact 2^-16 fixed point (the same bits in any reduction order)."""
    _check_flow(flow, "flow_field_means")
    flow = flow.contiguous()
    N, _, H, W = flow.shape
    out = _check_out(out, (N, 2), flow, "flow_field_means")
    _ffi.check(_ffi.lib().va_flow_field_means(_ffi.ctx(flow.device.index), _ffi.ptr(flow), N, W, H, _ffi.ptr(out),
                                              _ffi.stream_ptr(flow.device)))
    return out.view(N, 2)


def _overlaps(a, b):
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def motion_field(flow, flow_count, trajectory=False, means=None, out=None):
    """S12: flow ``[N,2,H,W]`` float32 of clips of ``flow_count`` = L pairs -> a float32 array of the same shape and pair
    order, which every S9 / S10 consumer (``flow_to_stack``, ``crop_flow_to_stack``, ``crop_flow_to_stack_views``) takes
    as it takes flow.  ``trajectory``: pair k of a clip is sampled along the trajectory that starts at each pixel of the
    clip's first frame and follows the raw flow.  ``means``: CUDA float32 ``[N,2]`` (``flow_field_means``) subtracted
    from every value of its field.  ``out`` must not overlap ``flow``."""
    _check_flow(flow, "motion_field")
    N, _, H, W = flow.shape
    L = int(flow_count)
    if L < 1 or N % L:
        raise ValueError("motion_field: %d flow pairs are not a whole number of clips of %d" % (N, L))
    if not trajectory and means is None:
        raise ValueError("motion_field: nothing to do (no trajectory and no means)")
    if means is not None:
        if (not isinstance(means, torch.Tensor) or means.dtype != torch.float32 or means.device != flow.device
                or means.numel() != 2 * N):
            raise ValueError("motion_field: means must be a float32 [%d,2] tensor on the flow's device" % N)
        means = means.contiguous()
    flow = flow.contiguous()
    out = _check_out(out, (N, 2, H, W), flow, "motion_field")
    if _overlaps(out, flow):
        raise ValueError("motion_field: out must not overlap flow")
    _ffi.check(_ffi.lib().va_flow_motion(_ffi.ctx(flow.device.index), _ffi.ptr(flow), N // L, L, int(bool(trajectory)), W, H,
                                         _ffi.ptr(means), _ffi.ptr(out), _ffi.stream_ptr(flow.device)))
    return out.view(N, 2, H, W)


def fit_homography(flow, iters=16, c0=16.0, c_min=1.0):
    """S21: flow ``[N,2,H,W]`` float32 -> ``(H [N,3,3] float64, stats [N,2] float64)`` on the flow's device: per field the
    homography (pixel coordinates, ``H[2,2] = 1``) that a Tukey-reweighted least-squares fit over every pixel's
    correspondence finds -- the camera's motion where the background covers most of the frame -- and
    ``stats[:,0]`` the share of the frame the last solve trusted, ``stats[:,1]`` 1.0 for a degenerate field (``H = I``).
    ``iters`` solves; the scale of the biweight anneals from ``c0`` px, halving its square every iteration, to ``c_min`` px."""
    _check_flow(flow, "fit_homography")
    try:
        iters, c0, c_min = int(iters), float(c0), float(c_min)
    except (TypeError, ValueError):
        raise ValueError("fit_homography: iters, c0 and c_min must be numbers")
    if not 1 <= iters <= 1024:
        raise ValueError("fit_homography: iters must be in 1..1024, got %d" % iters)
    if not (0.0 < c_min <= c0 < 1e150):
        raise ValueError("fit_homography: need 0 < c_min <= c0, got c0=%r c_min=%r" % (c0, c_min))
    flow = flow.contiguous()
    N, _, H, W = flow.shape
    Hm = torch.empty((N, 3, 3), dtype=torch.float64, device=flow.device)
    stats = torch.empty((N, 2), dtype=torch.float64, device=flow.device)
    _ffi.check(_ffi.lib().va_flow_homography(_ffi.ctx(flow.device.index), _ffi.ptr(flow), N, W, H, iters, c0 * c0,
                                             c_min * c_min, _ffi.ptr(Hm), _ffi.ptr(stats), _ffi.stream_ptr(flow.device)))
    return Hm, stats


def compensate_camera(flow, H, out=None):
    """S22: flow ``[N,2,H,W]`` float32 minus the displacement field of ``H`` (CUDA float64 ``[N,3,3]``, ``fit_homography``)
    -> a float32 array of the same shape and pair order, which every S9 - S17 consumer takes as it takes flow.  ``out``
    may be ``flow`` itself (in place) or must not overlap it."""
    _check_flow(flow, "compensate_camera")
    N, _, h, w = flow.shape
    if (not isinstance(H, torch.Tensor) or H.dtype != torch.float64 or H.device != flow.device
            or tuple(H.shape) != (N, 3, 3)):
        raise ValueError("compensate_camera: H must be a float64 [%d,3,3] tensor on the flow's device" % N)
    if out is not None and not flow.is_contiguous():
        raise ValueError("compensate_camera: with out=, flow must be contiguous")
    flow = flow.contiguous()
    H = H.contiguous()
    out = _check_out(out, (N, 2, h, w), flow, "compensate_camera")
    if out.data_ptr() != flow.data_ptr() and _overlaps(out, flow):
        raise ValueError("compensate_camera: out must be flow itself or must not overlap it")
    _ffi.check(_ffi.lib().va_flow_compensate(_ffi.ctx(flow.device.index), _ffi.ptr(flow), N, w, h, _ffi.ptr(H), _ffi.ptr(out),
                                             _ffi.stream_ptr(flow.device)))
    return out.view(N, 2, h, w)


def _check_frames(frames, who):
    """TV-L1's input -> ``[S,F,h,w]`` (a ``[F,h,w]`` tensor is one sequence); ValueError for anything else."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise ValueError("%s: frames must be a CUDA tensor" % who)
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.dim() != 4 or frames.dtype not in (torch.uint8, torch.float32):
        raise ValueError("%s: frames must be uint8 or float32 [S,F,H,W] (or [F,H,W]), TV-L1's input" % who)
    if frames.shape[0] < 1 or frames.shape[1] < 2 or frames.shape[2] < 1 or frames.shape[3] < 1:
        raise ValueError("%s: frames %s hold no frame pair" % (who, tuple(frames.shape)))
    return frames


def warp_pairs(frames, H, out=None):
    """S53: frames ``[S,F,h,w]`` (or ``[F,h,w]``) CUDA uint8 or float32, TV-L1's input, and H CUDA float64 ``[N,3,3]``,
    ``N = S*(F-1)`` in TV-L1's pair order (``fit_homography`` of their flow) -> float32 ``[N,2,h,w]``, TV-L1 input again:
    pair n holds frame k as float and frame k+1 resampled at ``H[n] (x, y, 1)``, which takes the camera's motion out of the
    pair.  Pixels whose position is not inside frame k+1 keep frame k's value.  ``out`` must not overlap ``frames``."""
    frames = _check_frames(frames, "warp_pairs")
    S, F, h, w = frames.shape
    N = S * (F - 1)
    if (not isinstance(H, torch.Tensor) or H.dtype != torch.float64 or H.device != frames.device
            or tuple(H.shape) != (N, 3, 3)):
        raise ValueError("warp_pairs: H must be a float64 [%d,3,3] tensor on the frames' device" % N)
    frames = frames.contiguous()
    H = H.contiguous()
    out = _check_out(out, (N, 2, h, w), frames, "warp_pairs")
    if _overlaps(out, frames):
        raise ValueError("warp_pairs: out must not overlap frames")
    _ffi.check(_ffi.lib().va_frames_warp_pairs(_ffi.ctx(frames.device.index), _ffi.ptr(frames), int(frames.dtype == torch.uint8),
                                               S, F, w, h, _ffi.ptr(H), _ffi.ptr(out), _ffi.stream_ptr(frames.device)))
    return out.view(N, 2, h, w)


def rerun_camera(frames, flow, params=None, out=None):
    """S54, TSN's two-pass warped flow -> ``(field, H, share)``: ``fit_homography`` of ``flow`` (the TV-L1 field of
    ``frames``, S21: ``H`` and ``share`` are the subtract form's), ``warp_pairs`` of the frames under it (S53), and
    ``tvl1_flow`` of those pairs with the same ``params``: ``field`` is that second pass's flow, written into ``out`` (over
    the first pass when ``out is flow``; with a ``BroxParams`` the second pass is ``brox_flow``).  Everything runs on the current stream; the second pass uses the TV-L1 workspace
    slot ``RERUN_WS_SLOT``, one of its own.  (``TwoStreamPipeline`` runs the same three steps over its own buffers.)"""
    _check_flow(flow, "rerun_camera")
    frames = _check_frames(frames, "rerun_camera")
    S, F, h, w = frames.shape
    if frames.device != flow.device or tuple(flow.shape) != (S * (F - 1), 2, h, w):
        raise ValueError("rerun_camera: flow must be the [%d,2,%d,%d] TV-L1 field of the frames, on their device, got %s"
                         % (S * (F - 1), h, w, tuple(flow.shape)))
    H, stats = fit_homography(flow)
    return tvl1_flow(warp_pairs(frames, H), params, ws_slot=RERUN_WS_SLOT, out=out), H, stats[:, 0]


def apply_camera(flow, camera="none", in_place=False):
    """S21 + S22 for ``camera`` (``CAMERAS``) -> ``(field, H, share)``: with ``"none"`` the flow itself and two Nones (no
    kernel, no buffer); with ``"homography"`` the compensated field (written over ``flow`` when ``in_place``), the fitted
    ``H [N,3,3]`` and the trusted share ``[N]`` of every field.  This is the ``"subtract"`` form; ``rerun_camera`` is the
    other."""
    if camera == "none":
        return flow, None, None
    H, stats = fit_homography(flow)
    return compensate_camera(flow, H, out=flow if in_place else None), H, stats[:, 0]


def apply_motion(flow, flow_count, motion="stack", mean_flow=False, out=None, *, camera_form="subtract", frames=None,
                 tvl1_params=None, camera="none"):
    """The float array S9 / S10 read for the given motion options (checked by ``check_motion``): ``flow`` itself for
    plain or bi-directional stacking without means (no kernel, no buffer), else ``motion_field`` of it (into ``out``).
    ``camera="homography"`` compensates the camera first (S21, S22, into a new array: ``flow`` is left as it is) and the
    motion options then act on the compensated field.  ``camera_form="rerun"`` (``CAMERA_FORMS``) compensates in TSN's
    two-pass form instead (S53, S54; ``rerun_camera``): it needs ``frames``, the TV-L1 input ``flow`` came from, and runs
    the second pass with ``tvl1_params``, which must be the first pass's."""
    if camera != "none" and camera_form == "rerun":
        if frames is None:
            raise ValueError("apply_motion: camera_form='rerun' needs frames=, the TV-L1 input of the flow")
        flow = rerun_camera(frames, flow, tvl1_params)[0]
    elif camera != "none":
        flow = apply_camera(flow, camera)[0]
    if motion != "trajectory" and not mean_flow:
        return flow
    means = flow_field_means(flow) if mean_flow else None
    return motion_field(flow, flow_count, trajectory=motion == "trajectory", means=means, out=out)


def pyramid_sizes(w, h, params=None):
    """The level sizes of S1 for ``params``: an ``_ffi.Tvl1Params``, an ``_ffi.BroxParams`` (its ``scale_step`` and
    ``nscales``) or an ``_ffi.FarnebackParams`` (its ``pyr_scale`` and ``levels``); the three methods share the pyramid."""
    p = params if params is not None else _ffi.default_tvl1_params()
    for m in (_BROX, _FARNEBACK):  # (va_tvl1_pyramid_sizes reads two fields: the method's names for them)
        if isinstance(p, m.params):
            p = _ffi.default_tvl1_params(scale_step=getattr(p, m.step), nscales=getattr(p, m.levels))
    ws = (ctypes.c_int * 16)()
    hs = (ctypes.c_int * 16)()
    n = _ffi.lib().va_tvl1_pyramid_sizes(w, h, ctypes.byref(p), ws, hs)
    return [(ws[i], hs[i]) for i in range(n)]


def tile_plan(w, h, params=None):
    """The register tiling ``tvl1_flow`` will use per pyramid level (host logic, no GPU needed):
    list of dict(tile_w, tile_h, waves, block_iters, tiles_x, tiles_y).  A ``BroxParams`` raises ValueError."""
    _tvl1_only(params, "tile_plan")
    p = params if params is not None else _ffi.default_tvl1_params()
    out = (ctypes.c_int * 96)()
    n = _ffi.lib().va_tvl1_tile_plan(w, h, ctypes.byref(p), out)
    keys = ("tile_w", "tile_h", "waves", "block_iters", "tiles_x", "tiles_y")
    return [dict(zip(keys, [out[6 * s + k] for k in range(6)])) for s in range(n)]


def launch_plan(w, h, n_seq, frames_per_seq, params=None, **over):
    """The inner-iteration and median launches ``tvl1_flow`` makes for ``n_seq`` sequences of ``frames_per_seq`` frames of
    ``w`` x ``h``, in launch order, reported by the loop that makes them running dry (``va_tvl1_launch_plan``; host logic,
    no GPU needed): a list of dicts with the fields of ``va_tvl1_launch`` (include/va.h), ``family`` as one of
    ``_ffi.TVL1_LAUNCH_FAMILIES``.  ``params`` / keyword overrides as ``tvl1_flow`` takes them (``median``, ``median_every``
    included); parameters out of range raise ValueError.  A ``BroxParams`` raises ValueError."""
    _tvl1_only(params, "launch_plan")
    p = params if params is not None else _ffi.default_tvl1_params(**over)
    opt = _ffi.tvl1_options(p)
    ref = ctypes.byref(opt) if opt is not None else None
    L = _ffi.lib()
    n = L.va_tvl1_launch_plan(w, h, n_seq, frames_per_seq, ctypes.byref(p), ref, None, 0)
    if n < 0:
        raise ValueError(_ffi.last_error())
    recs = (_ffi.Tvl1Launch * max(n, 1))()
    if L.va_tvl1_launch_plan(w, h, n_seq, frames_per_seq, ctypes.byref(p), ref, recs, n) != n:
        raise RuntimeError("va_tvl1_launch_plan: two runs of one plan differ")
    names = [f[0] for f in _ffi.Tvl1Launch._fields_]
    out = []
    for r in recs[:n]:
        d = {k: getattr(r, k) for k in names}
        d["family"] = _ffi.TVL1_LAUNCH_FAMILIES[d["family"]]
        out.append(d)
    return out


def profile_enable(on=True, device=None):
    _tvl1_only(on, "profile_enable")
    _tvl1_only(device, "profile_enable")
    _ffi.check(_ffi.lib().va_tvl1_profile_enable(_ffi.ctx(device), int(bool(on))))


def profile_levels(n_levels, reset=True, device=None):
    """Per pyramid level since the last reset: list of dict(ms, px_iters, launches) (call ``profile_read(reset=False)``
    first: it synchronises the recorded events).  TV-L1's inner iterations only: a ``BroxParams`` raises ValueError."""
    _tvl1_only(n_levels, "profile_levels")
    out = (ctypes.c_double * (3 * n_levels))()
    _ffi.check(_ffi.lib().va_tvl1_profile_levels(_ffi.ctx(device), out, n_levels, int(bool(reset))))
    return [dict(ms=out[3 * s], px_iters=out[3 * s + 1], launches=out[3 * s + 2]) for s in range(n_levels)]


def profile_read(reset=True, device=None):
    """-> dict(ms, launches, px_iters, px_warps, union_ms) for the inner-iteration kernel since the last
    reset (``ms``: summed per-call kernel time; ``union_ms``: wall time with at least one call's
    inner-iteration launches in flight -- they differ when several streams overlap).  A ``BroxParams`` raises ValueError."""
    _tvl1_only(reset, "profile_read")
    out = (ctypes.c_double * 5)()
    _ffi.check(_ffi.lib().va_tvl1_profile_read(_ffi.ctx(device), out, int(bool(reset))))
    return dict(ms=out[0], launches=out[1], px_iters=out[2], px_warps=out[3], union_ms=out[4])
