"""The two-stream clip pipeline on one GPU: frames -> TV-L1 flow -> flow volume -> both VGG-16 streams.

One clip = 1 RGB frame ``u8[3,224,224]`` + 11 gray frames ``u8[11,224,224]`` -> 10 TV-L1 pairs ->
``f32[20,224,224]`` flow volume -> spatial and temporal forward -> class scores ``f32[2,101]`` and
descriptors ``f32[2,256]``.  Larger frames (UCF-101's 320x240) come with crops
(``augment.draw_clip_crops``): TV-L1 then runs on the full frames and the crop and flip of getTransforms() are applied on
the device, or go through V views each (``views=``: ten-crop evaluation) whose outputs are averaged.
In the reference the first half happens offline
(precomputed flow JPEGs, Sheet03/temporalModel.py:76-90) and the second half is ``validate()``'s
forward (Sheet03/spatialModel.py:212-218, Sheet03/temporalModel.py:241-247).
"""
import itertools
import types

import torch

from . import flow as vflow
from . import frames as vframes
from . import augment, fusion, rgbdiff, synth, vgg, video
from .parameters import (NACTION_CLASSES, NORM_MEANS_TF, NORM_STDS_TF, VIDEO_DESCRIPTOR_DIM,
                         VIDEO_INPUT_FLOW_COUNT)


def build_stream_weights(c_in, seed, device, n_classes=NACTION_CLASSES):
    """Random-init weights of one stream; the temporal first layer follows ``__copyFirstLayer__``.  ``n_classes``: the
    outputs of the last layer (a multi-task pipeline: the sum of its heads)."""
    w = synth.synth_vgg16_weights(c_in=c_in, n_classes=n_classes, desc_dim=VIDEO_DESCRIPTOR_DIM, seed=seed,
                                  device=device)
    if c_in != 3:
        w["conv_w"][0] = vgg.copy_first_layer(w["conv_w"][0].to(device), c_in)
    return w


def _check_rgb(rgb, msg, planes=3):
    """``rgb`` is a uint8 ``[*,planes,H,W]`` tensor (``planes=None``: any number of them), or ValueError(msg)."""
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8 or rgb.dim() != 4 or (planes and rgb.shape[1] != planes):
        raise ValueError(msg)


def _check_video_frames(rgb, gray, who):
    """The frames of one video: rgb uint8 ``[T,3,H,W]`` and gray uint8 or float32 ``[T,H,W]``, one per rgb frame."""
    _check_rgb(rgb, "%s: rgb must be a uint8 [T,3,H,W] tensor" % who)
    if not isinstance(gray, torch.Tensor) or gray.dim() != 3 or gray.dtype not in (torch.uint8, torch.float32):
        raise ValueError("%s: gray must be a uint8 or float32 [T,H,W] tensor" % who)
    if gray.shape[0] != rgb.shape[0]:
        raise ValueError("%s: %d rgb frames but %d gray frames" % (who, rgb.shape[0], gray.shape[0]))


def _check_view_pair(views, rgb_hw, gray_hw, who):
    """``views=`` of ``who`` -> (rgb_views, flow_views), each table checked against the size of its frames."""
    if not isinstance(views, (tuple, list)) or len(views) != 2:
        raise ValueError("%s: views= must be (rgb_views, flow_views), e.g. two augment.ten_crop_views tables" % who)
    rgb_views, flow_views = views
    augment.check_views(rgb_views, rgb_hw[0], rgb_hw[1], augment.CROP_SIZE, "%s(views=)" % who)
    augment.check_views(flow_views, gray_hw[0], gray_hw[1], augment.CROP_SIZE, "%s(views=)" % who)
    return rgb_views, flow_views


def _check_video_args(rgb, gray, flow_count, motion, n_snippets, views, consensus, fusion_weights, crops, m=2):
    """``check_video`` for a pipeline that fuses ``m`` streams -> (plan, rgb_views, flow_views, consensus mode, weights)."""
    who = "submit_video"
    if crops is not None:
        raise ValueError("submit_video: a video takes views=, not crops= (one table for all its snippets)")
    if motion != "stack":
        raise ValueError("submit_video: motion=%r is not offered for whole videos (its chains depend on the window); "
                         "use motion='stack'" % (motion,))
    _check_video_frames(rgb, gray, who)
    mode = fusion.check_consensus(consensus, who)
    ws = fusion.check_fusion_weights(fusion_weights, who) if m == 2 else fusion.check_fusion_weights_n(fusion_weights, m, who)
    try:
        plan = video.snippetPlan(int(gray.shape[0]), flow_count, int(n_snippets))
    except ValueError as e:
        raise ValueError("submit_video: %s" % e)
    if views is None:  # one view: the frame itself
        if tuple(rgb.shape[-2:]) != (224, 224) or tuple(gray.shape[-2:]) != (224, 224):
            raise ValueError("submit_video: frames of %dx%d need views= (augment.ten_crop_views)" % (rgb.shape[-1], rgb.shape[-2]))
        rgb_views = flow_views = torch.zeros((1, 3), dtype=torch.int32)
    else:
        rgb_views, flow_views = _check_view_pair(views, rgb.shape[2:], gray.shape[1:], who)
    for v in (rgb_views, flow_views):
        if v.shape[0] > vgg.Vgg16Stream.VIEW_CHUNK:
            raise ValueError("submit_video: at most %d views, got %d" % (vgg.Vgg16Stream.VIEW_CHUNK, v.shape[0]))
    return plan, rgb_views, flow_views, mode, ws


def check_video(rgb, gray, flow_count, motion, n_snippets, views, consensus, fusion_weights, crops=None):
    """The host-side checks of ``TwoStreamPipeline.submit_video`` (ValueError; nothing touches the device) ->
    (plan, rgb_views, flow_views, consensus mode, wa, wb)."""
    plan, rgb_views, flow_views, mode, (wa, wb) = _check_video_args(rgb, gray, flow_count, motion, n_snippets, views, consensus,
                                                               fusion_weights, crops)
    return plan, rgb_views, flow_views, mode, wa, wb


_rerun_slots = itertools.count()  # one TV-L1 workspace slot per pipeline for the second pass of camera_form="rerun" (S54)


class TwoStreamPipeline(object):
    """Batches flow through three sets of HIP streams:

      * TV-L1 of a batch on ``flow_streams`` HIGH-priority streams (its pairs split between them),
      * both CNN forwards, the flow quantisation and the outputs on ONE normal-priority stream (``cnn``): its kernels
        get the CUs the TV-L1 launches leave idle (the tails of their ~2000 launches per batch),
      * the caller's stream only records "inputs ready" and, when it wants the results, waits for the CNN stream.

    ``submit()`` enqueues a batch and returns at once; the TV-L1 launches of batch i + 1 queue directly behind those of
    batch i, so batch i's flow quantisation and temporal CNN (which can only start when its last flow is done) run
    beside batch i + 1's TV-L1 instead of holding the TV-L1 streams idle (12 ms of a 140 ms step in round 1).
    ``run_batch()`` = ``submit()`` + ``wait()``: the unpipelined form, same results bit for bit.
    Buffers that cross streams (flow, flow volume) are owned by the pipeline, ``depth`` of each, guarded by events.
    Every submit path goes through ``_enqueue``, which alone creates, records and waits for those events
    (``tests/test_pipeline_order_host.py`` pins their order without a GPU).

    ``submit_video()`` / ``run_video()`` classify a whole video on the same streams: its snippets share
    one TV-L1 pass over the frame pairs they need, and the scores of snippets and views are averaged and fused on the device.

    ``extract_flow()`` computes the flow of a whole video once and keeps it on the device;
    ``submit_video(flow=)`` / ``run_video(flow=)`` and ``train_videos(flows=)`` then run without TV-L1.

    ``motion`` / ``mean_flow``: the temporal model's input representation (``flow.MOTIONS``), applied
    to every batch that comes with gray frames.  Bi-directional flow reorders the gray frames on the caller's stream; the
    means and the trajectory resampling run on the CNN stream into a pipeline-owned full-frame buffer.

    ``camera``: ``"homography"`` turns the flow into TSN's warped optical flow (``flow.CAMERAS``): on the
    CNN stream, behind the TV-L1 events, a homography is fitted to every field and its displacement field subtracted in
    place in the slot's flow buffer; the motion options and every gather then read the compensated field.  The results
    gain ``homography`` f64 ``[pairs,3,3]`` and ``camera_share`` f64 ``[pairs]``.

    ``camera_form``: ``"rerun"`` takes TSN's own two-pass form of the warped flow instead (``flow.CAMERA_FORMS``; DESIGN.md
    S53, S54): at the same place on the CNN stream the homography is fitted, the second frame of every pair is warped by it
    into the slot's pairs buffer, and TV-L1 runs again on those pairs over the slot's flow buffer, with a workspace of this
    pipeline's own.  ``extract_flow`` then stores that flow and ``train_videos`` trains on it.  It costs a second TV-L1;
    ``homography`` and ``camera_share`` are the same.  ``"rerun"`` with ``camera="none"`` raises ValueError.

    ``tvl1_params``: an ``_ffi.Tvl1Params`` (None: TV-L1's defaults) or an ``_ffi.BroxParams``.  With the latter every flow of
    the pipeline -- ``run_batch``, ``run_video``, ``train_videos``, the second pass of ``camera_form="rerun"`` and what
    ``extract_flow`` stores -- is Brox flow, the two-stream paper's own method (``flow.brox_flow``).  An
    ``_ffi.FarnebackParams`` does the same for Farneback flow, the direct method (``flow.farneback_flow``).

    ``rgb_diff``: True adds TSN's RGB-difference stream: ``self.diff``, a third VGG-16 of
    ``3 * rgb_diff_count`` input channels (seed ``diff_seed`` or ``weights[2]``; its first layer is the cross-modality copy of
    an RGB one) that ``submit_video`` / ``run_video`` and ``train_videos`` feed with the differences of each snippet's first
    ``rgb_diff_count + 1`` RGB frames.  ``submit`` / ``run_batch`` receive one RGB frame per clip: they ignore the third
    stream.  With the default nothing is allocated and every result keeps its bits.

    ``heads``: a tuple of 1 to 8 class counts, one per dataset, builds every stream as a multi-task model: one
    shared network whose last layer holds ``sum(heads)`` outputs, head t the columns ``vgg.head_logits(., heads, t)``.
    ``train_videos`` then takes ``tasks=`` (one head per video, labels local to it) and ``submit_video`` / ``run_video``
    ``task=``; ``submit`` / ``run_batch`` return the logits of all heads side by side.  None (the default) builds exactly
    the single-head pipeline of ``NACTION_CLASSES`` classes."""

    def __init__(self, device=None, spatial_seed=1, temporal_seed=2, flow_count=VIDEO_INPUT_FLOW_COUNT,
                 tvl1_params=None, weights=None, flow_streams=2, cnn_dtype="f32", depth=2, motion="stack", mean_flow=False,
                 rgb_diff=False, rgb_diff_count=rgbdiff.RGB_DIFF_COUNT, diff_seed=3, heads=None, *, camera_form="subtract",
                 camera="none"):
        self.heads = None
        if heads is not None:
            vgg.check_heads(heads, None, "TwoStreamPipeline")
            self.heads = tuple(int(h) for h in heads)
        n_classes = NACTION_CLASSES if self.heads is None else sum(self.heads)
        vflow.check_motion(motion, mean_flow, flow_count, "TwoStreamPipeline", camera=camera)
        vflow.check_camera_form(camera_form, "TwoStreamPipeline", camera)
        self.D = rgbdiff.check_diff_count(rgb_diff_count, flow_count, "TwoStreamPipeline") if rgb_diff else 0
        if weights and len(weights) != (3 if rgb_diff and len(weights) > 2 else 2):
            raise ValueError("TwoStreamPipeline: weights= holds the spatial and temporal weights, and a third entry only with "
                             "rgb_diff=True; got %d entries" % len(weights))
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.device = dev
        self.L = flow_count
        self.motion, self.mean_flow, self.camera, self.camera_form = motion, mean_flow, camera, camera_form
        with torch.cuda.device(dev):
            ws = weights[0] if weights else build_stream_weights(3, spatial_seed, dev, n_classes)
            wt = weights[1] if weights else build_stream_weights(2 * flow_count, temporal_seed, dev, n_classes)
            self.spatial = vgg.Vgg16Stream(ws["conv_w"], ws["conv_b"], ws["fc_w"], ws["fc_b"], n_classes,
                                           VIDEO_DESCRIPTOR_DIM, NORM_MEANS_TF, NORM_STDS_TF, device=dev.index, ws_slot=1,
                                           dtype=cnn_dtype)
            self.temporal = vgg.Vgg16Stream(wt["conv_w"], wt["conv_b"], wt["fc_w"], wt["fc_b"], n_classes,
                                            VIDEO_DESCRIPTOR_DIM, device=dev.index, dtype=cnn_dtype)
            self.diff = None
            if rgb_diff:  # float input (the differences are normalised by the gather), a workspace of its own
                wd = weights[2] if weights and len(weights) > 2 else build_stream_weights(3 * self.D, diff_seed, dev, n_classes)
                self.diff = vgg.Vgg16Stream(wd["conv_w"], wd["conv_b"], wd["fc_w"], wd["fc_b"], n_classes,
                                            VIDEO_DESCRIPTOR_DIM, device=dev.index, ws_slot=2, dtype=cnn_dtype)
        self.tvl1_params = tvl1_params
        self.flow_streams = max(1, int(flow_streams))
        self.depth = max(1, int(depth))
        self._cnn = torch.cuda.Stream(device=dev, priority=0)
        self._cnn2 = torch.cuda.Stream(device=dev, priority=0)  # precomputed flow volumes: the temporal CNN beside the spatial one
        self._n = 0
        self._flow = [None] * self.depth      # per slot: flow [pairs,2,H,W] written by the TV-L1 streams
        self._stack = [None] * self.depth     # per slot: flow volume read by the temporal CNN
        self._motion = [None] * self.depth    # per slot: the motion field S9 / S10 read instead of the flow (S12)
        self._dstack = [None] * self.depth    # per slot: the RGB-difference volume (S23), written and read on the CNN stream
        self._pairs = [None] * self.depth     # per slot: the warped pairs (S53), written and read on the CNN stream ("rerun" only)
        self._rerun_slot = (vflow.RERUN_WS_SLOT, next(_rerun_slots))  # the second pass's workspace: this pipeline's CNN stream alone
        self._flow_read = [None] * self.depth  # per slot: event "the flow buffer has been quantised" (it may be overwritten)
        self._handed_out = []                 # output tensors allocated on the CNN stream since the last wait()
        self._retired = []                    # dropped cross-stream buffers + the events after which they may be freed
        self._t_done = None                   # event behind the temporal model's last forward (it owns ONE workspace)

    def flow_volume(self, gray):
        """gray u8/f32 ``[B, L+1, 224, 224]`` -> flow volume f32 ``[B, 2L, 224, 224]`` (ordered on the current stream)."""
        B, F, H, W = gray.shape
        if F != self.L + 1:
            raise ValueError("flow_volume: need %d gray frames per clip, got %d" % (self.L + 1, F))
        tv = self._tvl1_frames(gray)
        if self.flow_streams > 1:
            fl = vflow.tvl1_flow_concurrent(tv, self.tvl1_params, self.flow_streams)
        else:
            fl = vflow.tvl1_flow(tv, self.tvl1_params)
        if self._rerun():
            fl = vflow.apply_motion(fl, self.L, self.motion, self.mean_flow, camera_form="rerun", frames=tv,
                                    tvl1_params=self.tvl1_params, camera=self.camera)
        else:
            fl = vflow.apply_motion(fl, self.L, self.motion, self.mean_flow, camera=self.camera)
        return vflow.flow_to_stack(fl).view(B, 2 * self.L, H, W)

    def _tvl1_frames(self, gray):
        """The TV-L1 input of gray ``[B,L+1,H,W]``: the frames themselves, or with bi-directional flow the forward and
        backward sequences ``[2B,L/2+1,H,W]`` (S13), reordered on the current stream."""
        return vflow.bidirectional_sequences(gray) if self.motion == "bidirectional" else gray

    def _rerun(self):
        """The camera step takes the two-pass form (getattr: the host tests build pipelines attribute by attribute)."""
        return self.camera != "none" and getattr(self, "camera_form", "subtract") == "rerun"

    def _camera(self, flow, out, tv=None, k=None):
        """On the CNN stream, after the TV-L1 events and before ``_motion_field``: S21 and S22 in place in the flow buffer
        (no buffer of its own); the fitted homographies and trusted shares go into the result dict ``out``.

        ``camera_form="rerun"`` (S54): S21, then S53 of ``tv`` -- the TV-L1 input ``flow`` came from -- and TV-L1 again over the
        flow buffer.  With a slot ``k`` this runs on the CNN stream: the pairs go into slot k's buffer and the second pass
        has this pipeline's own workspace, which only its CNN stream uses; without one (``train_videos``, ``extract_flow``)
        everything is in order on the current stream."""
        if self._rerun():
            pairs, slot = None, vflow.RERUN_WS_SLOT
            if k is not None:
                tv.record_stream(self._cnn)
                pairs, slot = self._buffer(self._pairs, k, tuple(flow.shape)), self._rerun_slot
            Hm, stats = vflow.fit_homography(flow)  # flow.rerun_camera's three steps, over the pipeline's own buffers
            pairs = vflow.warp_pairs(tv, Hm, out=pairs)
            vflow.tvl1_flow(pairs, self.tvl1_params, ws_slot=slot, out=flow)
            out["homography"], out["camera_share"] = Hm, stats[:, 0]
        elif self.camera != "none":
            _, out["homography"], out["camera_share"] = vflow.apply_camera(flow, self.camera, in_place=True)
        return flow

    def _motion_field(self, flow, k):
        """On the CNN stream, after the TV-L1 events: the array S9 / S10 read -- the flow itself, or the
        motion field in slot k's buffer."""
        if self.motion != "trajectory" and not self.mean_flow:
            return flow
        return vflow.apply_motion(flow, self.L, self.motion, self.mean_flow,
                                  out=self._buffer(self._motion, k, tuple(flow.shape)))

    def _buffer(self, bank, k, shape):
        """Slot k's buffer, re-allocated when the batch shape changes (a ragged last batch).  The buffers are allocated on
        the caller's stream but read and written on the pipeline's own streams, which the caching allocator knows nothing
        about: a dropped buffer is therefore kept alive in ``_retired`` until everything those streams had queued at that
        moment has run (one event per stream), instead of being handed back while a quantisation on the CNN stream or a
        TV-L1 call that still uses it is pending.  (``Tensor.record_stream`` on the pipeline's streams would say the same to
        the allocator, but measured 10 % slower on the whole benchmark: 216 against 241 clips/s.)"""
        t = bank[k]
        if t is None or tuple(t.shape) != tuple(shape):
            if t is not None:
                evs = []
                for st in [self._cnn, self._cnn2] + list(vflow.flow_streams(self.device, self.flow_streams)):
                    ev = torch.cuda.Event()
                    ev.record(st)
                    evs.append(ev)
                self._retired.append((t, evs))
            self._retired = [(old, evs) for old, evs in self._retired if not all(e.query() for e in evs)]
            bank[k] = t = torch.empty(shape, dtype=torch.float32, device=self.device)
        return t

    def _check_views(self, rgb, gray, flow_stack, views):
        """Host-side checks of ``views=`` before anything is enqueued -> (rgb_views, flow_views)."""
        if flow_stack is not None:
            raise ValueError("submit: views= needs gray frames; flow_stack= is already cropped")
        _check_rgb(rgb, "submit: rgb must be a uint8 [B,3,H,W] tensor with views=", planes=None)
        if gray is None or gray.dim() != 4:
            raise ValueError("submit: gray must be [B,L+1,H,W] with views=")
        return _check_view_pair(views, rgb.shape[2:], gray.shape[2:], "submit")

    def _check_inputs(self, rgb, gray, flow_stack, crops):
        """Host-side checks before anything is enqueued -> (rgb_crops, flow_crops), either None where that input is used as
        it is (it must then be 224x224)."""
        rgb_crops = flow_crops = None
        if crops is not None:
            if not isinstance(crops, (tuple, list)) or len(crops) != 2:
                raise ValueError("submit: crops= must be (rgb_crops, flow_crops) as augment.draw_clip_crops returns")
            rgb_crops, flow_crops = crops
        if rgb_crops is not None:
            _check_rgb(rgb, "submit: cropped rgb must be a uint8 [B,3,H,W] tensor", planes=None)
            augment.check_crops(rgb_crops, rgb.shape[0], rgb.shape[2], rgb.shape[3], augment.CROP_SIZE, "submit(crops=)")
        elif tuple(rgb.shape[-2:]) != (224, 224):
            raise ValueError("submit: rgb frames of %dx%d need crops= (augment.draw_clip_crops)" % (rgb.shape[-1], rgb.shape[-2]))
        if flow_stack is not None:
            if flow_crops is not None:
                raise ValueError("submit: flow_stack= is already cropped; pass crops=(rgb_crops, None)")
        elif flow_crops is not None:
            B, F, H, W = gray.shape
            augment.check_crops(flow_crops, B * 2 * self.L, H, W, augment.CROP_SIZE, "submit(crops=)")
        elif tuple(gray.shape[-2:]) != (224, 224):
            raise ValueError("submit: gray frames of %dx%d need crops= (augment.draw_clip_crops)" % (gray.shape[-1], gray.shape[-2]))
        return rgb_crops, flow_crops

    def submit(self, rgb, gray=None, flow_stack=None, crops=None, views=None, invert_flow_x=False):
        """Enqueue one batch; -> dict(logits_s, logits_t, desc_s, desc_t, done) of tensors that the CNN stream is still
        writing (``done``: the event recorded behind them): call ``wait()`` (or ``run_batch``) before reading them
        on another stream.  ``flow_stack``
        (precomputed volumes, the reference's actual input) skips TV-L1.

        ``crops``: ``(rgb_crops [B,3], flow_crops [B*2L,3])`` from ``augment.draw_clip_crops`` for frames larger than
        224x224 (u8 rgb ``[B,3,Hr,Wr]``, gray ``[B,L+1,Hg,Wg]``, each side >= 224): TV-L1 runs on the full gray frames
        and both inputs are cropped and flipped on the CNN stream.  Either entry may be None for an input that is
        224x224 already.

        ``views``: ``(rgb_views [Vs,3], flow_views [Vt,3])`` view tables (``augment.ten_crop_views``): every clip is seen
        through every view of its stream (ten-crop evaluation).  ``logits_*`` / ``desc_*`` are then the
        view means ``[B,...]`` and ``logits_*_views`` / ``desc_*_views`` hold the per-view outputs ``[B,V,...]``.  Not
        with ``crops=`` or ``flow_stack=``.  ``invert_flow_x``: TSN flips, a mirrored x-flow image becomes
        ``q -> 255 - q`` (with ``views=`` or ``crops=``; the default mirrors without inverting, as the reference).
        The pipeline's ``motion`` / ``mean_flow`` apply with and without ``crops=`` / ``views=``; they need gray frames.
        A batch holds one RGB frame per clip, so an ``rgb_diff=True`` pipeline ignores its third stream here: the results
        are those of a plain pipeline.  On a pipeline with ``heads`` the logits are full width, all heads side by side:
        ``vgg.head_logits(logits, heads, task)`` takes one head's columns."""
        if flow_stack is not None and (self.motion != "stack" or self.mean_flow):
            raise ValueError("submit: motion=%r / mean_flow=%r need gray frames; flow_stack= is already quantised"
                             % (self.motion, self.mean_flow))
        if flow_stack is not None and self.camera != "none":
            raise ValueError("submit: camera=%r needs gray frames; flow_stack= is already quantised" % (self.camera,))
        if views is not None:
            if crops is not None:
                raise ValueError("submit: views= and crops= exclude each other")
            rgb_views, flow_views = self._check_views(rgb, gray, flow_stack, views)
            return self._submit_views(rgb, gray, rgb_views, flow_views, bool(invert_flow_x))
        if invert_flow_x and flow_stack is not None:
            raise ValueError("submit: invert_flow_x needs gray frames; flow_stack= is already quantised")
        rgb_crops, flow_crops = self._check_inputs(rgb, gray, flow_stack, crops)
        if flow_stack is None and gray.shape[1] != self.L + 1:
            raise ValueError("submit: need %d gray frames per clip, got %d" % (self.L + 1, gray.shape[1]))
        extra = {}

        def spatial(k):
            rgb.record_stream(self._cnn)
            return self.spatial.forward(rgb if rgb_crops is None else augment.crop_images(rgb, rgb_crops))[1:]

        def temporal(stack):
            return self.temporal.forward(stack)[1:]

        def finish(s, t):
            (desc_s, logits_s), (desc_t, logits_t) = s, t
            return dict(logits_s=logits_s, logits_t=logits_t, desc_s=desc_s, desc_t=desc_t, **extra)

        if flow_stack is not None:
            def given_stack(flow, k):
                flow_stack.record_stream(self._cnn2)
                return flow_stack
            return self._enqueue(spatial, given_stack, temporal, finish, beside=True)
        B, F, H, W = gray.shape
        tv = self._tvl1_frames(gray)

        def to_stack(flow, k):
            src = self._motion_field(self._camera(flow, extra, tv, k), k)
            if flow_crops is None:
                return vflow.flow_to_stack(src, out=self._buffer(self._stack, k, (B, 2 * self.L, H, W)))
            # the flow buffer is full-frame, the volume 224x224
            return vflow.crop_flow_to_stack(src, flow_crops, out=self._buffer(self._stack, k, (B, 2 * self.L, 224, 224)),
                                            invert_x_on_flip=bool(invert_flow_x))
        return self._enqueue(spatial, to_stack, temporal, finish, tv=tv, flow_shape=(B * self.L, 2, H, W))

    def _submit_views(self, rgb, gray, rgb_views, flow_views, invert):
        """``submit(views=)``: the stream layout of the crops= path, with B*V images per stream and the view means."""
        B, F, H, W = gray.shape
        if F != self.L + 1:
            raise ValueError("submit: need %d gray frames per clip, got %d" % (self.L + 1, F))
        Vt = flow_views.shape[0]
        extra = {}
        tv = self._tvl1_frames(gray)

        def spatial(k):
            rgb.record_stream(self._cnn)
            return self.spatial.forward_views(augment.crop_image_views(rgb, rgb_views))

        def to_stack(flow, k):
            src = self._motion_field(self._camera(flow, extra, tv, k), k)
            return vflow.crop_flow_to_stack_views(src, flow_views, self.L, invert_x_on_flip=invert,
                                                  out=self._buffer(self._stack, k, (B, Vt, 2 * self.L, 224, 224)))

        def finish(s, t):
            (desc_s, logits_s, desc_sv, logits_sv), (desc_t, logits_t, desc_tv, logits_tv) = s, t
            return dict(logits_s=logits_s, logits_t=logits_t, desc_s=desc_s, desc_t=desc_t, logits_s_views=logits_sv,
                        logits_t_views=logits_tv, desc_s_views=desc_sv, desc_t_views=desc_tv, **extra)
        return self._enqueue(spatial, to_stack, self.temporal.forward_views, finish, tv=tv, flow_shape=(B * self.L, 2, H, W))

    def _enqueue(self, spatial, to_stack, temporal, finish, tv=None, flow_shape=None, beside=False):
        """The stream choreography of every submit path (the class docstring); the only place that creates, records or waits
        for the pipeline's events.  The caller has prepared its inputs on the current stream and supplies what differs:

          * ``tv``, ``flow_shape``: the TV-L1 input and the shape of the slot's flow buffer; None when the flow is given (a
            stored flow or ``flow_stack=``): no TV-L1 is started and no flow-read event is recorded;
          * ``spatial(k)``: what runs on the CNN stream before it waits for TV-L1 (the spatial forward, the third stream);
          * ``to_stack(flow, k)`` -> the temporal input, on the CNN stream behind the TV-L1 events (camera, motion, a gather
            into slot k's volume);
          * ``temporal(stack)``: the temporal forward;
          * ``finish(s, t)``: what follows on the CNN stream (consensus, view means, fusion) -> the result dict, from what
            ``spatial`` and ``temporal`` returned.

        ``beside``: the ``flow_stack=`` form.  There is no TV-L1 to share the GPU with: the two CNNs (independent models,
        workspaces of their own) run on two streams, so that the half-empty last round of one layer's workgroups overlaps the
        other model's layer (measured on the bf16 stack: 2.63 -> 2.53 ms per batch)."""
        cur = torch.cuda.current_stream(self.device)
        ready = torch.cuda.Event()
        ready.record(cur)  # the inputs are complete here; nothing below makes `cur` wait for anything
        k = self._n % self.depth
        self._n += 1
        flow, evs = None, []
        if tv is not None:
            flow, evs = vflow.tvl1_flow_concurrent(tv, self.tvl1_params, self.flow_streams,
                                                   out=self._buffer(self._flow, k, flow_shape),
                                                   after=[ready, self._flow_read[k]], join=False)
        with torch.cuda.stream(self._cnn):
            self._cnn.wait_event(ready)
            s = spatial(k)
            for ev in evs:
                self._cnn.wait_event(ev)
            if beside:
                self._cnn2.wait_event(ready)
                with torch.cuda.stream(self._cnn2):
                    t = self._guarded_temporal(self._cnn2, lambda: temporal(to_stack(flow, k)))
                self._cnn.wait_stream(self._cnn2)
            else:
                stack = to_stack(flow, k)
                if tv is not None:
                    self._flow_read[k] = torch.cuda.Event()  # after the motion kernel and the gather: both have read the flow
                    self._flow_read[k].record(self._cnn)
                t = self._guarded_temporal(self._cnn, lambda: temporal(stack))
            out = finish(s, t)
            finished = torch.cuda.Event()
            finished.record(self._cnn)
        self._handed_out.extend(v for v in out.values() if isinstance(v, torch.Tensor))
        out["done"] = finished  # host-side throttle: out["done"].synchronize() blocks the HOST until this batch is complete
        return out

    def _guarded_temporal(self, stream, forward):
        """``forward()`` on ``stream`` (the current one), between the wait for the temporal model's previous forward and the
        record behind this one: the model owns ONE workspace, whichever stream it runs on."""
        if self._t_done is not None:
            stream.wait_event(self._t_done)
        t = forward()
        self._t_done = torch.cuda.Event()
        self._t_done.record(stream)
        return t

    def extract_flow(self, frames, rescale=None, dtype=torch.uint8, return_camera=False):
        """The stored flow of one video: TV-L1 once on all ``T - 1`` consecutive frame pairs, kept on the
        device for ``submit_video(flow=)``, ``train_videos(flows=)`` and ``video.evaluateVideos(flows=)``, which then launch no
        TV-L1 at all.  ``frames``: gray ``[T,H,W]`` (uint8 or float32) or decoded RGB uint8 ``[T,3,H,W]`` on the pipeline's
        device; for RGB the gray frames and ``rescale=`` go through ``frames.prepare_frames`` as in ``submit_video``.

        The pairs are split into ``flow_streams`` contiguous chunks, each one TV-L1 sequence that includes its boundary frame
        (every frame's pyramid is built once per chunk), with the pipeline's ``tvl1_params`` (a ``BroxParams`` there stores Brox flow, ``flow.brox_flow``); field t is the flow from frame
        t to frame t + 1 and equals ``flow.tvl1_flow`` of those two frames bit for bit.  The pipeline's ``camera`` step (S21,
        S22) is applied to every field before anything is stored, so the store of a ``camera="homography"`` pipeline is TSN's
        warped flow; with ``camera_form="rerun"`` it is TSN's own two-pass warped flow (S53, S54: the second TV-L1 is paid
        here, once per video).  ``dtype``: ``torch.float32`` keeps TV-L1's output, exact; ``torch.uint8`` (the default, a quarter of the
        size) quantises it last to the 8-bit flow images of S9 (``flow.quantize_flow``).

        Returns the store ``[T-1,2,H,W]``, ready on the current stream; with ``return_camera=True``
        ``(store, homography, camera_share)``, the last two None without a camera step.  A bi-directional pipeline raises
        ValueError (its backward fields are not consecutive pairs), as do frames of another type, rank or device and fewer
        than two frames, before anything is enqueued."""
        who = "extract_flow"
        if self.motion == "bidirectional":
            raise ValueError("%s: a bi-directional pipeline computes backward fields, which are not the consecutive pairs a "
                             "stored flow holds" % who)
        if dtype not in (torch.uint8, torch.float32):
            raise ValueError("%s: dtype must be torch.uint8 or torch.float32, got %r" % (who, dtype))
        if not isinstance(frames, torch.Tensor) or frames.dim() not in (3, 4):
            raise ValueError("%s: frames must be gray [T,H,W] or rgb uint8 [T,3,H,W]" % who)
        size = None
        if frames.dim() == 4:
            _, _, _, oh, ow = vframes.check_frames(frames, rescale, "NCHW", who)
            size = (oh, ow)
        else:
            if rescale is not None:
                raise ValueError("%s: rescale= acts on rgb frames (the gray of rescaled frames is not the rescaled gray)" % who)
            if frames.dtype not in (torch.uint8, torch.float32):
                raise ValueError("%s: gray frames must be uint8 or float32" % who)
        if frames.shape[0] < 2:
            raise ValueError("%s: %d frames hold no frame pair" % (who, frames.shape[0]))
        self._check_on_device(who, "frames", frames)
        dev = self.device
        gray = frames.contiguous() if size is None else vframes.prepare_frames(frames, size)[1]
        T, H, W = gray.shape
        P = T - 1
        n = min(self.flow_streams, P)
        bounds = [(P * i) // n for i in range(n + 1)]
        cur = torch.cuda.current_stream(dev)
        flow = torch.empty((P, 2, H, W), dtype=torch.float32, device=dev)
        if n == 1:
            vflow.tvl1_flow(gray.unsqueeze(0), self.tvl1_params, out=flow)
        else:
            streams = vflow.flow_streams(dev, self.flow_streams)[:n]
            for i, st in enumerate(streams):
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    part = gray[bounds[i]:bounds[i + 1] + 1]  # pairs bounds[i] .. bounds[i+1]-1 and their boundary frame
                    part.record_stream(st)
                    flow.record_stream(st)
                    vflow.tvl1_flow(part.unsqueeze(0), self.tvl1_params, ws_slot=i + 1, out=flow[bounds[i]:bounds[i + 1]])
            for st in streams:
                cur.wait_stream(st)
        if self._rerun():  # S54 on the current stream: the warp sees the video as the one sequence it is
            cam = {}
            self._camera(flow, cam, gray.unsqueeze(0))
            Hm, share = cam["homography"], cam["camera_share"]
        else:
            flow, Hm, share = vflow.apply_camera(flow, self.camera, in_place=True)
        store = vflow.quantize_flow(flow) if dtype == torch.uint8 else flow
        return (store, Hm, share) if return_camera else store

    def _check_task(self, task, who):
        """``task=`` against the pipeline's ``heads`` -> the head's index, or None on a pipeline without heads."""
        heads = getattr(self, "heads", None)
        if heads is None:
            if task is not None:
                raise ValueError("%s: task= needs a pipeline built with heads=" % who)
            return None
        if task is None:
            raise ValueError("%s: this pipeline has the heads %s; task= must name the video's head" % (who, heads))
        return vgg.check_task(task, heads, who)

    @staticmethod
    def _prepared_shapes(rgb, gray, rescale, who):
        """``gray=None`` / ``rescale=`` of one video, on the host (ValueError) -> None when the frames are used as they are,
        else ``(size, rgb_like, gray_like)``: the size ``frames.prepare_frames`` takes and storage-free stand-ins with the
        shapes it will return, for the shape checks that run before anything is enqueued."""
        if rescale is not None and gray is not None:
            raise ValueError("%s: rescale= derives gray from the rescaled rgb (gray=None): a gray rescaled on its own is not "
                             "the gray of the rescaled frames" % who)
        if gray is not None:
            return None
        n, _, _, oh, ow = vframes.check_frames(rgb, rescale, "NCHW", who)
        return ((oh, ow), torch.empty((n, 3, oh, ow), dtype=torch.uint8, device="meta"),
                torch.empty((n, oh, ow), dtype=torch.uint8, device="meta"))

    def _check_video(self, rgb, gray, n_snippets, views, consensus, fusion_weights, crops, rescale=None, flow=None):
        """Host-side checks of ``submit_video`` before anything is enqueued -> (plan, rgb_views, flow_views, mode, weights,
        size): one fusion weight per stream, None meaning all ones; ``size`` is None for frames used as they are, else what
        ``frames.prepare_frames`` takes (``gray=None`` / ``rescale=``: the checks then see the prepared shapes).  ``flow``: a
        stored flow, checked against the prepared frames."""
        who = "submit_video"
        if flow is not None and gray is not None:
            raise ValueError("submit_video: flow= replaces the gray frames and their TV-L1; pass gray=None with it")
        prep = self._prepared_shapes(rgb, gray, rescale, who)
        decoded = rgb
        if prep is not None:
            _, rgb, gray = prep
        m = 2 if self.diff is None else 3
        if fusion_weights is None:
            fusion_weights = (1.0,) * m
        try:
            given = len(fusion_weights)
        except TypeError:
            raise ValueError("submit_video: fusion weights must be %d numbers, got %r" % (m, fusion_weights))
        if given != m:
            raise ValueError("submit_video: this pipeline fuses %d streams (spatial, temporal%s), got %d fusion weights"
                             % (m, ", difference" if m == 3 else "", given))
        plan, rgb_views, flow_views, mode, ws = _check_video_args(rgb, gray, self.L, self.motion, n_snippets, views, consensus,
                                                             fusion_weights, crops, m)
        if flow is not None:
            self._check_stored_flow(flow, gray, who, "a uint8 stored flow is")
        if prep is not None:
            self._check_on_device(who, "rgb", decoded)
        else:
            self._check_on_device(who, "rgb and gray", rgb, gray)
        if flow is not None:
            self._check_on_device(who, "the stored flow", flow)
        return plan, rgb_views, flow_views, mode, ws, None if prep is None else prep[0]

    def _check_stored_flow(self, flow, gray, who, uint8_flow_is):
        """The rules of one video's stored flow but the device: its type and its shape against the
        (prepared) gray frames, and a uint8 store only where nothing acts on the float field."""
        vflow.check_stored_flow(flow, int(gray.shape[0]), int(gray.shape[1]), int(gray.shape[2]), who)
        if flow.dtype == torch.uint8 and (self.motion != "stack" or self.mean_flow):
            raise ValueError("%s: motion=%r / mean_flow=%r act on the float field; %s already quantised (store float32 flow for "
                             "them)" % (who, self.motion, self.mean_flow, uint8_flow_is))

    def _decoded(self, video, who):
        """A path to a Motion-JPEG AVI in the place of a video's rgb frames, alone or as ``(path, None)``
        -> its frames u8 ``[T,3,H,W]`` in the same form, decoded on the pipeline's device on the current stream; anything else
        comes back as it is.  This runs ahead of the other checks, which need the frames' shape: the file is parsed (ValueError
        for a codec or a JPEG the decoder does not take), uploaded and decoded, and the decoder's status is read, one
        synchronisation.  A path that brings gray frames raises ValueError: they are derived from the decoded frames."""
        import os
        pair = isinstance(video, (tuple, list)) and len(video) == 2
        path = video[0] if pair else video
        if not isinstance(path, (str, os.PathLike)):
            return video
        if pair and video[1] is not None:
            raise ValueError("%s: a video given as a file's path comes without gray frames (gray=None)" % who)
        from . import utils
        frames = utils.loadVideoFrames(path, self.device)
        return (frames, None) if pair else frames

    def _check_on_device(self, who, what, *tensors):
        """Every tensor is on the pipeline's device, or ValueError "<who>: <what> must be on <device>"."""
        if any(not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != self.device for t in tensors):
            raise ValueError("%s: %s must be on %s" % (who, what, self.device))

    def submit_video(self, rgb, gray=None, n_snippets=video.N_SNIPPETS, views=None, invert_flow_x=False, consensus="softmax",
                     fusion_weights=None, crops=None, task=None, rescale=None, flow=None):
        """Enqueue one whole video (the test protocol of Sheet03/notes.txt:113-116 and 225-230):
        rgb u8 ``[T,3,H,W]``, gray u8 or f32 ``[T,H,W]``, the frames of one video on the device.  ``n_snippets`` snippets
        are placed by ``video.snippetStarts``; the frame pairs they share go through TV-L1 once each
        (``video.snippetPlan``), every snippet is seen through every view, and the class scores are averaged over snippets
        and views (``consensus``: ``"softmax"`` or ``"logits"``, ``fusion.score_consensus``) and fused with
        ``fusion_weights`` = (spatial, temporal) (``fusion.fuse_scores``; None: all ones).

        On an ``rgb_diff=True`` pipeline snippet s also gives the differences of frames ``starts[s] ..
        starts[s] + rgb_diff_count`` of ``rgb``, read in place through every RGB view (``rgbdiff.rgb_diff_stack``), to the
        third stream, beside the TV-L1 that is still running; ``fusion_weights`` then takes three entries (spatial, temporal,
        difference; ``fusion.fuse_scores_n``) and the result gains ``scores_d``, ``desc_d`` and ``logits_d_items``.

        ``views=(rgb_views, flow_views)`` as in ``submit(views=)``; None is one view of 224x224 frames.  Returns a dict of
        tensors the CNN stream is still writing (``wait()`` first): ``scores_s``, ``scores_t``, ``scores`` f32 ``[C]``,
        ``pred`` int32 ``[]``, ``desc_s``, ``desc_t`` f32 ``[256]`` (the mean over snippets and views in item order),
        ``logits_s_items``, ``logits_t_items`` ``[n,V,C]``, and ``starts`` (the snippets' first pairs, a list), ``plan``,
        ``done``.  The stream layout is ``submit(views=)``'s: the TV-L1 of the next video queues behind this one's.
        ``mean_flow=True`` subtracts every planned field's own mean and ``camera="homography"`` compensates every planned
        field (the result gains ``homography`` and ``camera_share``, one entry per planned pair); trajectory and
        bi-directional pipelines raise ValueError, as do bad shapes, a video shorter than one snippet and ``crops=``, before anything is enqueued.

        On a pipeline with ``heads`` ``task`` names the video's head and is required: every stream's item
        logits go through ``vgg.head_logits(., heads, task)`` before the consensus and the fusion, so ``scores*`` hold the
        ``heads[task]`` classes of that head and ``pred`` is local to it; ``logits_*_items`` stay full width, and the result
        gains ``task``.  ``task=`` on a pipeline without heads raises ValueError.

        Decoded frames: ``gray=None`` derives the gray frames from ``rgb`` on the device, and
        ``rescale=`` (an int: the short side, torchvision's ``Resize`` rule; or ``(height, width)``) first rescales every
        frame as PIL's bilinear ``Image.resize`` does (``frames.prepare_frames``); ``views`` are then tables for the new
        size.  Both run on the current stream ahead of everything else, so the TV-L1 and CNN streams wait for them as they
        wait for the inputs.  ``rescale=`` with a given ``gray`` raises ValueError.  The result holds ``frame_size``, the
        ``(height, width)`` TV-L1 and the views saw.

        Stored flow: ``flow=`` is the video's flow computed once (``extract_flow``), a contiguous float32
        or uint8 ``[T-1,2,H,W]`` tensor on the pipeline's device, of the prepared frames' size; ``gray`` must then be None.  No
        TV-L1 is launched and the camera step is not applied again (the store of a ``camera="homography"`` pipeline already
        holds the warped flow; the result has no ``homography`` / ``camera_share``): snippet s reads the L fields from field
        ``plan.starts[s]`` on through the flow views, and everything else is as above.  A float32 store goes through
        ``mean_flow`` and the float gather and keeps the bits of the live call; a uint8 store goes through
        ``flow.flowq_to_stack_snippets``, needs ``mean_flow=False`` and keeps the bits too.  ``flow=`` with ``gray=``, a store
        of another type, shape, size or device and a uint8 store on a ``mean_flow`` pipeline raise ValueError before
        anything is enqueued.

        Motion-JPEG files: ``rgb`` may be the path of a Motion-JPEG AVI (with ``gray=None``); its frames
        are decoded on the device on the current stream (``utils.loadVideoFrames``) and everything above follows.  Any
        other codec raises ValueError naming it.  The decode comes FIRST, ahead of the checks above, which need the frames'
        shape: with a path a bad argument is found only after the file was uploaded and decoded, and the call waits once on
        the host for the decoder's status (a frame that does not decode raises ValueError) before it enqueues the rest --
        ``evaluateVideos`` therefore runs ahead by less than a video when it is fed paths.  Decode with
        ``utils.loadVideoFrames`` and pass the tensor where neither is wanted."""
        task = self._check_task(task, "submit_video")
        rgb, gray = self._decoded((rgb, gray), "submit_video")
        stored = flow
        plan, rgb_views, flow_views, mode, fw, size = self._check_video(rgb, gray, n_snippets, views, consensus, fusion_weights,
                                                                       crops, rescale, stored)
        n, U = plan.n, len(plan.pairs)
        if stored is not None:  # the gray frames only fed TV-L1: the frames are rescaled (S38) or used as they are
            if size is not None and tuple(size) != tuple(rgb.shape[2:]):
                rgb, _ = vframes.prepare_frames(rgb, size)
            T, H, W = int(rgb.shape[0]), int(rgb.shape[2]), int(rgb.shape[3])
            tv = None
        else:
            if gray is None:  # S38: on the current stream, ahead of the gathers and of `ready`
                rgb, gray = vframes.prepare_frames(rgb, size)
            T, H, W = gray.shape
            tv = self._take(gray, plan.sequences)                          # [U,2,H,W]: one two-frame sequence per planned pair
        frames = self._take(rgb, plan.starts)                              # [n,3,H,W]
        Vt = flow_views.shape[0]
        extra = {}

        def spatial(k):
            frames.record_stream(self._cnn)
            s = self.spatial.forward_views(augment.crop_image_views(frames, rgb_views))[2:]
            if self.diff is None:
                return s, None
            # S23 / S25: before the wait for TV-L1, so that it fills the time TV-L1 is still running
            Vs, C = rgb_views.shape[0], 3 * self.D
            rgb.record_stream(self._cnn)
            dstack = rgbdiff.rgb_diff_stack(rgb, rgbdiff.view_table(plan.starts, rgb_views), self.D,
                                            out=self._buffer(self._dstack, k, (n, Vs, C, 224, 224)))
            return s, self.diff.forward_views(dstack.view(n, Vs, C, 224, 224))[2:]

        def to_stack(flow, k):
            if stored is None:
                src = self._camera(flow, extra, tv, k)  # per planned field, like the means
            else:  # the store is complete at `ready`; its windows start at the snippets' own pairs
                stored.record_stream(self._cnn)
                src = stored
            if self.mean_flow:  # S11 / S12 per planned field: no chains, so the clip length does not matter
                src = vflow.apply_motion(src, 1, "stack", True, out=self._buffer(self._motion, k, tuple(src.shape)))
            first = plan.index if stored is None else plan.starts
            gather = vflow.flowq_to_stack_snippets if src.dtype == torch.uint8 else vflow.crop_flow_to_stack_snippets
            return gather(src, first, flow_views, self.L, invert_x_on_flip=bool(invert_flow_x),
                          out=self._buffer(self._stack, k, (n, Vt, 2 * self.L, 224, 224)))

        def temporal(stack):
            return self.temporal.forward_views(stack)[2:]

        def finish(s, t):
            ((desc_sv, logits_sv), d), (desc_tv, logits_tv) = s, t
            own = (lambda x: x) if task is None else (lambda x: vgg.head_logits(x, self.heads, task))  # S26: the video's head
            scores_s = fusion.score_consensus(own(logits_sv).unsqueeze(0), consensus)
            scores_t = fusion.score_consensus(own(logits_tv).unsqueeze(0), consensus)
            desc_s = vgg.view_mean(desc_sv.view(1, -1, desc_sv.shape[-1]))
            desc_t = vgg.view_mean(desc_tv.view(1, -1, desc_tv.shape[-1]))
            if d is None:
                scores, pred = fusion.fuse_scores(scores_s, scores_t, fw)
            else:
                desc_dv, logits_dv = d
                scores_d = fusion.score_consensus(own(logits_dv).unsqueeze(0), consensus)
                scores, pred = fusion.fuse_scores_n([scores_s, scores_t, scores_d], fw)
                desc_d = vgg.view_mean(desc_dv.view(1, -1, desc_dv.shape[-1]))
                extra.update(scores_d=scores_d[0], desc_d=desc_d[0], logits_d_items=logits_dv)
            out = dict(scores_s=scores_s[0], scores_t=scores_t[0], scores=scores[0], pred=pred[0], desc_s=desc_s[0],
                       desc_t=desc_t[0], logits_s_items=logits_sv, logits_t_items=logits_tv, **extra)
            out["starts"] = list(plan.starts)
            out["plan"] = plan
            out["frame_size"] = (int(H), int(W))
            if task is not None:
                out["task"] = task
            return out
        return self._enqueue(spatial, to_stack, temporal, finish, tv=tv, flow_shape=(U, 2, H, W))

    def _take(self, t, idx):
        """``t[idx]`` for a device tensor and a host list of indices (the index goes to the device on the current stream)."""
        return t[augment.crops_to_device(torch.tensor(idx, dtype=torch.int64), self.device)]

    def run_video(self, rgb, gray=None, n_snippets=video.N_SNIPPETS, views=None, invert_flow_x=False, consensus="softmax",
                  fusion_weights=None, crops=None, task=None, rescale=None, flow=None):
        """``submit_video`` + ``wait()``: the results are ready on the current stream."""
        out = self.submit_video(rgb, gray, n_snippets, views, invert_flow_x, consensus, fusion_weights, crops, task, rescale,
                                flow)
        self.wait()
        return out

    @staticmethod
    def _check_accumulate(n, k, micro_videos, clip_norm, data_parallel):
        """The accumulate arguments of ``train_videos`` -> videos per micro-batch, or None for the fused
        step (all three at their defaults).  ValueError for a bad value or combination; nothing touches a device."""
        import numbers
        who = "train_videos"
        vgg.check_clip_norm(clip_norm, who)
        if not isinstance(data_parallel, bool):
            raise ValueError("%s: data_parallel must be True or False, got %r" % (who, data_parallel))
        if data_parallel:
            import torch.distributed as tdist
            if not (tdist.is_available() and tdist.is_initialized()):
                raise ValueError("%s: data_parallel=True needs an initialised process group (dist.init)" % who)
        if micro_videos is None:
            if clip_norm is None and not data_parallel:
                return None
            if n < 1 or k < 1 or n * k > 64:
                raise ValueError("%s: %d videos x %d snippets out of range (n*k in 1..64); micro_videos= takes larger batches" % (who, n, k))
            return n
        if isinstance(micro_videos, bool) or not isinstance(micro_videos, numbers.Integral) or micro_videos < 1:
            raise ValueError("%s: micro_videos must be a positive integer, got %r" % (who, micro_videos))
        if k < 1 or micro_videos * k > 64:
            raise ValueError("%s: micro-batches of %d videos x %d snippets out of range (micro_videos*k in 1..64)" % (who, micro_videos, k))
        if n < 1:
            raise ValueError("%s: no videos" % who)
        return int(micro_videos)

    def _check_train_videos(self, videos, labels, k, starts, crops, rng, tasks=None, micro=None, rescale=None, flows=None):
        """Host-side checks and draws of ``train_videos`` before anything is enqueued -> a namespace of ``videos``, ``labels``,
        ``plans``, ``crops``, ``tasks``, ``sizes`` and ``flows``; ``tasks`` is None on a pipeline without heads.  ``micro``: videos per micro-batch (``_check_accumulate``),
        which lifts the limit on ``n*k``.  ``videos`` comes back as ``(rgb, gray)`` pairs, gray None where it is to be derived;
        ``sizes[i]`` is then what ``frames.prepare_frames`` takes for video i (None for a video used as it is), and every
        shape check has seen the prepared shapes.  ``flows``: None or one stored flow per video (DESIGN.md
        S39-S41), checked against the prepared frames; it comes back as a list."""
        who = "train_videos"
        heads = getattr(self, "heads", None)  # getattr: the host tests build pipelines attribute by attribute, some without heads
        if heads is None and tasks is not None:
            raise ValueError("%s: tasks= needs a pipeline built with heads=" % who)
        if heads is not None and tasks is None:
            raise ValueError("%s: this pipeline has the heads %s; tasks= must name every video's head" % (who, heads))
        if self.spatial.dtype != "f32" or self.temporal.dtype != "f32":
            raise ValueError("%s: training is fp32 only; this pipeline was built with cnn_dtype=%r" % (who, self.spatial.dtype))
        videos = list(videos)
        n, k = len(videos), int(k)
        if n < 1 or k < 1 or (micro is None and n * k > 64):
            raise ValueError("%s: %d videos x %d snippets out of range (n*k in 1..64)" % (who, n, k))
        if heads is not None:  # S26: one head per video, labels local to it
            labels, tasks = vgg.check_tasks(labels, tasks, heads, n, who)
        given = [(v, None) if isinstance(v, torch.Tensor) else v for v in videos]  # a bare rgb tensor: gray is derived
        videos, sizes, on_device = [], [], []  # what the shape checks see (S38: the prepared shapes) and how each video gets there
        for v in given:
            if not isinstance(v, (tuple, list)) or len(v) != 2:
                raise ValueError("%s: videos must be a list of (rgb u8 [T,3,H,W], gray [T,H,W]) pairs, (rgb, None) or rgb "
                                 "alone" % who)
            rgb, gray = v
            _check_rgb(rgb, "%s: rgb must be a uint8 [T,3,H,W] tensor" % who)
            prep = self._prepared_shapes(rgb, gray, rescale, who)
            on_device += [rgb] if prep is not None else [rgb, gray]
            if prep is not None:
                _, rgb, gray = prep
            _check_video_frames(rgb, gray, who)
            videos.append((rgb, gray))
            sizes.append(None if prep is None else prep[0])
            if (tuple(rgb.shape[2:]) != tuple(videos[0][0].shape[2:]) or tuple(gray.shape[1:]) != tuple(videos[0][1].shape[1:])
                    or gray.dtype != videos[0][1].dtype):
                raise ValueError("%s: the videos of one step must share their frame size and gray dtype" % who)
        if tuple(videos[0][0].shape[2:]) != tuple(videos[0][1].shape[1:]):
            raise ValueError("%s: one crop serves a snippet's RGB frame and flow planes: rgb and gray frames must have one "
                             "size" % who)
        if flows is not None:
            if self.motion == "bidirectional":
                raise ValueError("%s: a bi-directional pipeline needs backward fields; a stored flow holds consecutive pairs" % who)
            try:
                flows = list(flows)
            except TypeError:
                raise ValueError("%s: flows must be a list of one stored flow per video" % who)
            if len(flows) != n:
                raise ValueError("%s: %d videos but %d stored flows" % (who, n, len(flows)))
            if any(g is not None for _, g in given):
                raise ValueError("%s: flows= replaces the gray frames and their TV-L1; pass (rgb, None) or rgb alone with it" % who)
            for f, (_, gray) in zip(flows, videos):
                self._check_stored_flow(f, gray, who, "uint8 stored flows are")
            if any(f.dtype != flows[0].dtype for f in flows):
                raise ValueError("%s: the stored flows of one step must share their type" % who)
            on_device += flows
        self._check_on_device(who, "rgb and gray" + ("" if flows is None else " and the stored flows"), *on_device)
        H, W = (int(d) for d in videos[0][1].shape[1:])
        if not isinstance(labels, torch.Tensor):
            try:
                labels = torch.tensor([int(l) for l in labels], dtype=torch.int64)
            except (TypeError, ValueError):
                raise ValueError("%s: labels must be a tensor or a list of %d class indices" % (who, n))
        if labels.dim() != 1 or labels.shape[0] != n:
            raise ValueError("%s: %d videos but labels of shape %s" % (who, n, tuple(labels.shape)))
        vgg._check_labels(labels, self.spatial.n_classes, who)
        if starts is not None and (not isinstance(starts, (tuple, list)) or len(starts) != n):
            raise ValueError("%s: starts must hold one list of %d window starts per video" % (who, k))
        plans = []
        try:
            for i, (_, gray) in enumerate(videos):
                T = int(gray.shape[0])
                if starts is None:
                    st = video.segmentStarts(T, k, self.L, rng)
                else:
                    st = [int(x) for x in starts[i]]
                    if len(st) != k:
                        raise ValueError("video %d has %d starts, not k=%d" % (i, len(st), k))
                plans.append(video.segmentPlan(T, st, self.L))
        except (TypeError, ValueError) as e:
            raise ValueError("%s: %s" % (who, e))
        if crops is None:
            crops = augment.draw_scale_jitter_crops(n * k, H, W, rng)
        augment.check_jitter_crops(crops, n * k, H, W, who)
        return types.SimpleNamespace(videos=[tuple(v) for v in given], labels=labels, plans=plans, crops=crops, tasks=tasks,
                                     sizes=sizes, flows=flows)

    @staticmethod
    def _check_jitter(n_snippets, color_jitter, jitter, lighting, rng):
        """The colour-jitter arguments of ``train_videos``, checked (ValueError) and drawn before anything is enqueued -> the
        table, CPU float32 ``[n_snippets,8]``, or None."""
        who = "train_videos"
        if color_jitter is not None and jitter is not None:
            raise ValueError("%s: give color_jitter= (parameters to draw from) or jitter= (a table), not both" % who)
        if color_jitter is not None:
            try:
                b, c, s, h = color_jitter
            except (TypeError, ValueError):
                raise ValueError("%s: color_jitter must be (brightness, contrast, saturation, hue)" % who)
            jitter = augment.draw_color_jitter(n_snippets, b, c, s, h, rng)
        if jitter is not None:
            augment.check_color_jitter(jitter, n_snippets, who)
        if lighting is not None:
            augment.check_lighting(lighting, n_snippets, who)
        return jitter

    def _check_solver(self, solver):
        """``solver=`` of ``train_videos`` -> [(stream, Solver), ...] to set, in the order spatial, temporal, difference."""
        who = "train_videos"
        streams = [self.spatial, self.temporal] + ([self.diff] if self.diff is not None else [])
        if solver is None:
            return []
        if isinstance(solver, vgg.Solver):
            return [(m, solver) for m in streams]
        if not isinstance(solver, (tuple, list)) or len(solver) != len(streams) or not all(isinstance(s, vgg.Solver) for s in solver):
            raise ValueError("%s: solver must be None, a vgg.Solver or %d of them (spatial, temporal%s), got %r"
                             % (who, len(streams), ", difference" if len(streams) == 3 else "", solver))
        return list(zip(streams, solver))

    def _accumulate_step(self, n, k, micro, labels, tasks, lr, momentum, dropout_seed, clip_norm, data_parallel):
        """-> step(model, x) of ``train_videos`` in its accumulate form: the micro-batches of x ``[n*k,C,224,224]`` through
        ``train_accumulate``, the all-reduce of a data-parallel step, ``train_apply`` -> (stats, descriptors); ``step.norms``
        maps each model to the norm its apply reported."""
        from . import dist as vdist
        heads = self.heads if tasks is not None else None
        H = len(heads) if heads is not None else 0
        slices = vgg.micro_slices(n, micro)
        host_tasks = [int(t) for t in tasks.tolist()] if tasks is not None else None  # a device tensor is read back once
        first_micro, n_total, head_totals = 0, n, None
        if data_parallel:  # one small all-reduce: videos, videos per head, micro-batches of every rank
            rank, world = vdist.rank_world()
            counts = [n] + [sum(1 for t in host_tasks if t == h) for h in range(H)] + [len(slices) if r == rank else 0 for r in range(world)]
            counts = [int(v) for v in vdist.all_reduce_sum(torch.tensor(counts, dtype=torch.int64)).tolist()]
            n_total, head_totals, first_micro = counts[0], counts[1:1 + H] if H else None, sum(counts[1 + H:1 + H + rank])
        scales = vgg.micro_scales(slices, n_total, host_tasks, H, head_totals)

        def step(model, x):
            stats, descs = [], []
            for j, (lo, hi) in enumerate(slices):
                st, d = model.train_accumulate(x[lo * k:hi * k], labels[lo:hi], k=k, tasks=None if tasks is None else tasks[lo:hi],
                                               heads=heads, scales=scales[j], first=(j == 0), dropout_seed=dropout_seed + first_micro + j)
                stats.append(st)
                descs.append(d)
            out = vgg.combine_micro_stats(stats, scales, H)
            if data_parallel:
                vdist.all_reduce_gradients(model.grad())
                out = vdist.all_reduce_sum(out)
            step.norms[model] = model.train_apply(lr, momentum, clip_norm)
            return out, torch.cat(descs)
        step.norms = {}  # model -> the norm its apply reported (None without clip_norm)
        return step

    def train_videos(self, videos, labels, k=video.N_SEGMENTS, starts=None, crops=None, lr=1e-3, momentum=0.9, dropout_seed=0,
                     invert_flow_x=False, rng=None, tasks=None, micro_videos=None, clip_norm=None, data_parallel=False,
                     color_jitter=None, jitter=None, lighting=None, rescale=None, flows=None, solver=None):
        """One TSN training step of both streams on whole videos (Sheet03/notes.txt:165-185, 212-223).
        ``videos``: a list of n ``(rgb u8 [T,3,H,W], gray [T,H,W])`` pairs on the device, one frame size, any lengths;
        ``labels``: their n class indices; ``n*k <= 64``.

        Each video gives ``k`` snippets, one per temporal segment (``starts``: a list of k window starts per video;
        None draws them with ``video.segmentStarts``), and each snippet one scale-jitter crop for its RGB frame and its
        2L flow planes (``crops``: CPU int32 ``[n*k,5]`` rows ``{top, left, ch, cw, flip}``, video-major; None draws them
        with ``augment.draw_scale_jitter_crops``); ``rng``: the ``random.Random`` of both draws (starts of all videos
        first, then the crops).  TV-L1 runs once on each frame pair the snippets need (``video.segmentPlan``), the
        pipeline's ``motion`` / ``mean_flow`` apply per snippet window, the two crop-resize gathers build the 224x224
        inputs, and each stream takes one step on the consensus loss (``Vgg16Stream.train_step_consensus``) with ``lr``,
        ``momentum`` and ``dropout_seed``.  ``invert_flow_x``: TSN flips.

        Returns a dict: ``stats_s``, ``stats_t`` f32 ``[2]`` = (loss, hits) and ``desc_s``, ``desc_t`` f32 ``[n*k,256]``
        per stream, ready on the current stream, and ``starts``, ``crops``, ``plans``, ``flow`` (the planned TV-L1
        fields, video-major; with ``camera="homography"`` the compensated fields, beside ``homography`` and
        ``camera_share``).  Everything runs in order on the current stream, TV-L1 on the flow streams in between; batches
        submitted before are waited for, later ones see the updated weights.  A bf16 pipeline, ``n*k > 64``, a video
        shorter than one snippet and a bad table raise ValueError before anything is enqueued.

        On an ``rgb_diff=True`` pipeline the third stream takes the same step on the differences of each
        snippet's first ``rgb_diff_count + 1`` RGB frames, seen through the snippet's crop (``rgbdiff.rgb_diff_stack``);
        the result gains ``stats_d`` and ``desc_d``.

        On a pipeline with ``heads`` ``tasks`` gives one head per video and is required, ``labels`` are local
        to the video's head, every stream takes ``Vgg16Stream.train_step_multitask`` instead, and ``stats_*`` are f32
        ``[2+2H]`` = (loss, hits, loss of every head, hits of every head).  ``tasks=`` on a pipeline without heads, a missing
        ``tasks=`` on one with heads, a task outside the heads and a label outside its head raise ValueError before anything
        is enqueued.

        Gradient accumulation.  With ``micro_videos``, ``clip_norm`` and ``data_parallel`` at their
        defaults every stream takes the fused step above.  ``micro_videos=m`` (``m*k <= 64``) lifts the limit on ``n``: the
        inputs are built for all n videos as above (one TV-L1 plan, one gather per stream), then each stream runs
        ``ceil(n/m)`` ``Vgg16Stream.train_accumulate`` calls on slices of m videos -- dropout seed ``dropout_seed + j`` and
        scale ``n_j / n`` for micro-batch j (with heads: per head, its videos in the slice over its videos in the batch) --
        and one ``train_apply``.  ``clip_norm``: ``torch.nn.utils.clip_grad_norm_`` on each stream's whole gradient before its
        update (alone, with ``n*k <= 64``: one accumulate and one apply); the result gains ``norm_s``, ``norm_t``
        (``norm_d``), CUDA float64 ``[1]``.  ``stats_*`` are the scale-weighted sum of the micro-batches' losses and the
        sum of their hits (``vgg.combine_micro_stats``), on the device.  ``data_parallel=True`` under an initialised process
        group: ``videos`` is this rank's shard; the denominators of the scales (videos, videos per head) and the numbering of
        the micro-batches (rank-major, for the dropout seeds) come from one small all-reduce, each stream's gradient is
        all-reduced once between its last accumulate and its apply (``dist.all_reduce_gradients``), loss and hits are
        all-reduced too, and every rank ends with the same weights.  A bad value or combination raises ValueError before
        anything is enqueued.

        Colour jitter acts on the spatial stream's input alone, between ``resize_images`` and the step:
        ``color_jitter=(brightness, contrast, saturation, hue)`` draws one row per snippet from ``rng`` after the starts and
        the crops (``augment.draw_color_jitter``); ``jitter=`` passes the table itself, CPU float32 ``[n*k,8]``, as ``crops=``
        does; ``lighting``: CPU float32 ``[n*k,3]`` channel offsets (``augment.draw_lighting``), applied after the jitter.  The
        result gains ``jitter`` (None when nothing was asked for).  The temporal and the RGB-difference streams are
        untouched.  With all three at None nothing is drawn and nothing is launched.

        Decoded frames: an entry of ``videos`` may be ``(rgb, None)`` or ``rgb`` alone; its gray frames
        are then derived on the device, after ``rescale=`` (an int: the short side; or ``(height, width)``) has rescaled its
        frames (``frames.prepare_frames``).  The crops are drawn and checked for the new size, and colour jitter still acts
        on the spatial input alone: the gray frames come from the prepared frames, before it.  ``rescale=`` with an entry
        that brings its own gray raises ValueError.

        Stored flow: ``flows=`` is a list with one stored flow per video (``extract_flow``; float32 or
        uint8 ``[T-1,2,H,W]``, all of one type, of the prepared frames' size), and every entry of ``videos`` then comes without
        gray frames.  The planned fields (``plan.pairs``) are taken from the stores -- fields no snippet needs are never
        copied -- and neither TV-L1 nor the camera step runs.  With float32 everything from the motion options on is the code
        above and the step keeps the bits of the live one (``motion="trajectory"`` included; a bi-directional pipeline raises
        ValueError).  With uint8 the temporal input comes from ``flow.resize_flowq_to_stack``: TSN's order, the 8-bit image is
        resampled; equal to the live step for ``ch = cw = 224`` crops, not for resampling ones; it needs ``motion="stack"`` and
        ``mean_flow=False``.  The result's ``flow`` holds the planned fields in the stored type.

        The solver: ``solver=`` is one ``vgg.Solver`` for every stream, or one per stream in the order
        spatial, temporal, difference (TSN's dropout ratios differ per stream); each stream keeps it for later steps too
        (``Vgg16Stream.set_solver``).  None leaves the streams as they are.  Anything else raises ValueError before
        anything is enqueued.

        Motion-JPEG files: an entry of ``videos`` may be the path of a Motion-JPEG AVI in the place of
        ``rgb``, alone or as ``(path, None)``; its frames are decoded on the device first (``utils.loadVideoFrames``): ahead
        of every check above, with one wait on the host per file for the decoder's status, so with paths a bad argument is
        found only after the files were decoded."""
        videos = [self._decoded(v, "train_videos") for v in videos]
        solvers = self._check_solver(solver)
        micro = self._check_accumulate(len(videos), int(k), micro_videos, clip_norm, data_parallel)
        c = self._check_train_videos(videos, labels, k, starts, crops, rng, tasks, micro, rescale, flows)
        n, k = len(c.videos), int(k)
        jitter = self._check_jitter(n * k, color_jitter, jitter, lighting, rng)
        for m, sv in solvers:  # host state of each stream: nothing is enqueued
            m.set_solver(sv)
        if c.flows is None:
            videos = [v if v[1] is not None else vframes.prepare_frames(v[0], size) for v, size in zip(c.videos, c.sizes)]  # S38
        else:  # the gray frames only fed TV-L1: the frames are rescaled (S38) or used as they are
            videos = [(v[0] if tuple(size) == tuple(v[0].shape[2:]) else vframes.prepare_frames(v[0], size)[0], None)
                      for v, size in zip(c.videos, c.sizes)]
        labels, tasks = c.labels, c.tasks
        if micro is not None:
            step = self._accumulate_step(n, k, micro, labels, tasks, lr, momentum, dropout_seed, clip_norm, data_parallel)
        elif tasks is None:
            step = lambda m, x: m.train_step_consensus(x, labels, k, lr, momentum, dropout_seed)
        else:
            step = lambda m, x: m.train_step_multitask(x, labels, tasks, self.heads, k, lr, momentum, dropout_seed)
        cur = torch.cuda.current_stream(self.device)
        extra = {}
        xs, xt, flow = self._train_inputs(c, videos, jitter, lighting, bool(invert_flow_x), extra)
        cur.wait_stream(self._cnn)   # forwards submitted earlier read the weights this step updates
        cur.wait_stream(self._cnn2)
        stats_s, desc_s = step(self.spatial, xs)
        stats_t, desc_t = step(self.temporal, xt)
        if micro is not None and clip_norm is not None:
            extra["norm_s"], extra["norm_t"] = step.norms[self.spatial], step.norms[self.temporal]
        if self.diff is not None:
            extra["stats_d"], extra["desc_d"] = step(self.diff, self._train_diff_input(videos, c.plans, c.crops))
            if micro is not None and clip_norm is not None:
                extra["norm_d"] = step.norms[self.diff]
        self._cnn.wait_stream(cur)
        self._cnn2.wait_stream(cur)
        return dict(stats_s=stats_s, desc_s=desc_s, stats_t=stats_t, desc_t=desc_t, starts=[list(p.starts) for p in c.plans],
                    crops=c.crops, plans=c.plans, flow=flow, jitter=jitter, **extra)

    @staticmethod
    def _planned_positions(plans):
        """-> for every snippet of every plan, video-major, the position of its first field among the planned fields of all
        plans laid out one plan after the other (the order TV-L1 writes them)."""
        first, base = [], 0
        for p in plans:
            first += [base + j for j in p.index]
            base += len(p.pairs)
        return first

    def _train_inputs(self, c, videos, jitter, lighting, invert_flow_x, extra):
        """The inputs of one ``train_videos`` step from its checked arguments ``c`` (``_check_train_videos``) and the prepared
        ``videos``, in order on the current stream -> (spatial input u8 ``[n*k,3,224,224]``, temporal input f32
        ``[n*k,2L,224,224]``, the planned flow fields).  ``extra`` receives the camera step's results."""
        L, plans, flows = self.L, c.plans, c.flows
        n_snippets = sum(len(p.starts) for p in plans)
        windows = [i * L for i in range(n_snippets)]  # the first field of every snippet where each has L fields of its own
        frames = torch.cat([self._take(rgb, p.starts) for (rgb, _), p in zip(videos, plans)])  # [n*k,3,H,W]
        if flows is not None:  # the planned fields of every store, in the order TV-L1 would have written them
            flow = torch.cat([self._take(f, p.pairs) for f, p in zip(flows, plans)])
            first = self._planned_positions(plans)
        elif self.motion == "bidirectional":  # S13 per snippet window: its own forward and backward sequences, no sharing
            win = torch.cat([self._take(gray, [[s + f for f in range(L + 1)] for s in p.starts])
                             for (_, gray), p in zip(videos, plans)])  # [n*k,L+1,H,W]
            tv = vflow.bidirectional_sequences(win)
            first = windows
        else:
            tv = torch.cat([self._take(gray, p.sequences) for (_, gray), p in zip(videos, plans)])  # [U,2,H,W]: one two-frame sequence per planned pair
            first = self._planned_positions(plans)
        if flows is None:
            flow = vflow.tvl1_flow_concurrent(tv, self.tvl1_params, self.flow_streams)
            flow = self._camera(flow, extra, tv)  # per planned field, in place: everything below reads the compensated field
        if flow.dtype == torch.uint8:  # S41: the stored images themselves
            src = flow
        elif self.motion == "trajectory":  # S12 chains follow a window: the windows are laid out one after the other
            src = vflow.apply_motion(self._take(flow, [f + j for f in first for j in range(L)]), L, "trajectory", self.mean_flow)
            first = windows
        elif self.motion == "bidirectional":
            src = vflow.apply_motion(flow, L, "bidirectional", self.mean_flow)
        else:  # S11 / S12 per planned field
            src = vflow.apply_motion(flow, 1, "stack", self.mean_flow)
        rgb_table, flow_table = augment.snippet_tables(c.crops, list(range(n_snippets)), first, L)
        xs = augment.resize_images(frames, rgb_table)
        if jitter is not None or lighting is not None:  # S35: the spatial stream's input alone, in place
            table = jitter if jitter is not None else torch.tensor([augment.IDENTITY_JITTER_ROW] * n_snippets, dtype=torch.float32)
            xs = augment.color_jitter(xs, table, lighting, out=xs)
        gather = vflow.resize_flowq_to_stack if src.dtype == torch.uint8 else vflow.resize_flow_to_stack
        xt = gather(src, flow_table, invert_x_on_flip=invert_flow_x).view(n_snippets, 2 * L, 224, 224)
        return xs, xt, flow

    def _train_diff_input(self, videos, plans, crops):
        """The third stream's input of one ``train_videos`` step (S25): the windows' frames one after the other, one S23 call
        on the snippets' crops -> f32 ``[n*k,3D,224,224]``."""
        D = self.D
        win = torch.cat([self._take(rgb, [s + f for s in p.starts for f in range(D + 1)])
                         for (rgb, _), p in zip(videos, plans)])  # [n*k*(D+1),3,H,W]
        return rgbdiff.rgb_diff_stack(win, rgbdiff.window_table([i * (D + 1) for i in range(len(crops))], crops), D)

    def wait(self, stream=None):
        """Make ``stream`` (default: the current one) wait for every batch submitted so far."""
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        s.wait_stream(self._cnn)
        for t in self._handed_out:
            t.record_stream(s)
        self._handed_out = []

    def run_batch(self, rgb, gray=None, flow_stack=None, crops=None, views=None, invert_flow_x=False):
        """-> dict(logits_s, logits_t, desc_s, desc_t), ready on the current stream (``submit`` + ``wait``); with
        ``views=`` also the per-view ``*_views`` entries."""
        out = self.submit(rgb, gray, flow_stack, crops, views, invert_flow_x)
        self.wait()
        return out

    def close(self):
        self._cnn2.synchronize()
        self._cnn.synchronize()
        vflow.release_workspace(self._rerun_slot, self.device)  # the second pass's own (S54), if there was one
        self.spatial.close()
        self.temporal.close()
        if self.diff is not None:
            self.diff.close()
