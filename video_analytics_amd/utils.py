"""Host-side helpers of the two-stream path: the reference's ``Sheet03/utils.py`` surface.

Pure-Python string/indexing logic is bit-exact with the reference lines cited per function.
The image transforms restate the torchvision ~0.2 classes the reference composes
(``getTransforms``, Sheet03/utils.py:137-151) on numpy/torch, because torchvision is not part of this
stack; they draw from Python's global ``random`` module in the same order as that torchvision
generation (crop top, crop left, flip, then the colour jitter's numbers: DESIGN.md S32).  Training bookkeeping (``makeCheckpoint``, ``savePerformance``) and
frame extraction (``extractEveryNthFrame``, ``convertVideosToFrames``) are provided too; the reference decodes
with ``cv2.VideoCapture``, absent here, so ``iterVideoFrames`` reads RIFF/AVI Motion-JPEG itself and refuses
other codecs by name; ``loadVideoFrames``, ``loadFrameImages`` and ``loadFlowImages(device=)`` decode
the same JPEGs on the device.
"""
from __future__ import division

import csv
import os
import shutil
import random

import numpy as np
import torch
from PIL import Image
from torch.utils.data import DataLoader

from .parameters import *  # noqa: F401,F403  (the reference star-imports its config the same way)
from .parameters import (COLOR_JITTERS, CROP_SIZE_TF, HORIZONTAL_FLIP_TF, NORM_MEANS_TF, NORM_STDS_TF,
                         NWORKERS_LOADER, SHUFFLE_LOADER, TEMPORAL_BATCH_SIZE)


def checkAndMakeDirectories(*args):
    """Create missing directories; item i is True if directory i already existed
    (Sheet03/utils.py:14-26)."""
    exists = [True] * len(args)
    for i, arg in enumerate(args):
        if not os.path.exists(arg):
            exists[i] = False
            os.makedirs(arg)
    return exists


def makeCheckpoint(modelState, isBest, ckpLoc, bestModel):
    """Save the training state; copy it to ``bestModel`` when ``isBest`` (Sheet03/utils.py:29-35)."""
    torch.save(modelState, ckpLoc)
    if isBest:
        shutil.copyfile(ckpLoc, bestModel)


def savePerformance(precision, loss, csvLoc):
    """Append ``precision,loss`` of one epoch (Sheet03/utils.py:198-205)."""
    with open(csvLoc, "a") as csvFile:
        csvFile.write(str(precision) + "," + str(loss) + "\n")


def multiStepLr(baseLr, milestones, lastEpoch, gamma=0.1):
    """``MultiStepLR.get_lr()`` of torch 0.4 (the reference's scheduler, Sheet03/spatialModel.py:119):
    baseLr * gamma ** bisect_right(milestones, lastEpoch).  ``lastEpoch`` is whatever was passed to
    ``scheduler.step(...)`` -- the reference passes the validation LOSS (Sheet03/spatialModel.py:278, quirk)."""
    import bisect
    return baseLr * gamma ** bisect.bisect_right(sorted(milestones), lastEpoch)


def videoJpegs(videoLoc):
    """The JPEG byte strings of a video file's frames, in order: RIFF/AVI with Motion-JPEG streams (``MJPG``: every
    ``##dc`` / ``##db`` chunk of the ``movi`` list is one JPEG).  Any other codec (UCF-101 ships XviD) raises ValueError
    naming its fourcc: there is no decoder for it here."""
    import struct
    with open(videoLoc, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError("iterVideoFrames: %s is not a RIFF/AVI file" % videoLoc)
    fourcc = None
    k = data.find(b"strh")
    while k >= 0:  # the video stream header: 'strh' <size> 'vids' <handler fourcc>
        if data[k + 8:k + 12] == b"vids":
            fourcc = data[k + 12:k + 16]
            break
        k = data.find(b"strh", k + 4)
    if fourcc is None or fourcc.upper() not in (b"MJPG", b"JPEG"):
        raise ValueError("iterVideoFrames: no decoder for video codec %r of %s in this image (OpenCV is absent; "
                         "Motion-JPEG AVI files are supported)" % (fourcc, videoLoc))
    k = data.find(b"movi")
    if k < 0:
        raise ValueError("iterVideoFrames: %s has no movi list" % videoLoc)
    end = k - 4 + 8 + struct.unpack("<I", data[k - 4:k])[0]
    k += 4
    jpegs = []
    while k + 8 <= min(end, len(data)):
        cid, size = data[k:k + 4], struct.unpack("<I", data[k + 4:k + 8])[0]
        if cid == b"LIST":  # 'rec ' groups: descend
            k += 12
            continue
        if cid[2:4] in (b"dc", b"db") and size > 0:
            jpegs.append(data[k + 8:k + 8 + size])
        k += 8 + size + (size & 1)
    return jpegs


def iterVideoFrames(videoLoc):
    """Decoded frames (PIL RGB images) of a video file, in order.  The reference decodes with ``cv2.VideoCapture``
    (Sheet03/utils.py:57-68); OpenCV is not in this image, so the container is parsed here (``videoJpegs``: RIFF/AVI with
    Motion-JPEG streams) and every frame is decoded with PIL.  Any other codec raises ValueError naming its fourcc."""
    import io
    for jpg in videoJpegs(videoLoc):
        yield Image.open(io.BytesIO(jpg)).convert("RGB")


def loadVideoFrames(videoLoc, device):
    """The frames of a Motion-JPEG AVI decoded on the device -> uint8 ``[T,3,H,W]``, the stack of what
    ``iterVideoFrames`` yields, bit for bit: what ``run_video(rgb, rescale=..., views=...)``, ``extract_flow`` and
    ``train_videos`` take.  Gray frames come back with three equal channels, as ``convert("RGB")`` gives them.  ValueError as
    ``videoJpegs``, for a file without frames, and as ``jpeg.decode_jpegs``."""
    from . import jpeg
    jpegs = videoJpegs(videoLoc)
    if not jpegs:
        raise ValueError("loadVideoFrames: %s holds no frames" % videoLoc)
    out, _ = jpeg.decode_jpegs(jpegs, device)
    return out if out.dim() == 4 else out.unsqueeze(1).repeat(1, 3, 1, 1)


def loadFrameImages(paths, device):
    """The numbered frame files ``convertVideosToFrames`` wrote (or any baseline JPEG files of one size) decoded on the
    device in one call -> uint8 ``[N,3,H,W]``, or ``[N,H,W]`` for gray files, PIL's pixels bit for bit.
    ValueError for a missing file and as ``jpeg.decode_jpegs``."""
    from . import jpeg
    datas = []
    for p in paths:
        if not os.path.isfile(p):
            raise ValueError("loadFrameImages: missing %s" % p)
        with open(p, "rb") as f:
            datas.append(f.read())
    return jpeg.decode_jpegs(datas, device)[0]


def extractEveryNthFrame(videoLoc, N):
    """Every N-th frame (0, N, 2N, ...) of the video at ``videoLoc`` (Sheet03/utils.py:51-69); ValueError if the
    file does not exist."""
    if not (os.path.exists(videoLoc) and os.path.isfile(videoLoc)):
        raise ValueError("Video does not exist: %s" % (videoLoc))
    frameList = []
    for frameIdx, frame in enumerate(iterVideoFrames(videoLoc)):
        if frameIdx % N == 0:
            frameList.append(frame)
    return frameList


def saveFrameImages(frames, frameDir, quality=95, restartBlocks=None):
    """Write a uint8 ``[T,3,H,W]`` device tensor (what ``loadVideoFrames`` returns) as the numbered frame files
    ``frameDir/0.jpg, 1.jpg, ...`` that ``SpatialDataset.__getitem__`` opens: one ``jpeg.encode_jpegs`` call on the device
    (DESIGN.md S49-S52), 4:2:0 like PIL's default, byte for byte the files ``Image.save(..., quality=quality)`` writes.
    ``restartBlocks``: a restart marker every so many MCUs, which the device decoder reads with one lane per interval.
    Returns the file count; ValueError as ``jpeg.encode_jpegs`` and for a tensor that is not ``[T,3,H,W]``."""
    from . import jpeg
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError("saveFrameImages: frames must be a uint8 tensor [T,3,H,W]")
    files = jpeg.encode_jpegs(frames, quality=quality, subsampling=2, restart_blocks=restartBlocks)
    checkAndMakeDirectories(frameDir)
    for i, data in enumerate(files):
        with open(os.path.join(frameDir, str(i) + FRAME_EXTN), "wb") as f:
            f.write(data)
    return len(files)


def convertVideosToFrames(rootDir, saveDir, videoListLoc, sampleRate=VIDEO_FRAME_SAMPLE_RATE, mode="train", device=None):
    """Sheet03/utils.py:95-121: every ``sampleRate``-th frame of each listed video goes to
    ``saveDir/<category>/<videoName>/<i>.jpg`` (i = 0, 1, ... counts the SAMPLED frames: the names
    ``SpatialDataset.__getitem__`` opens, Sheet03/spatialModel.py:75-77).  A video whose frame directory already
    exists is skipped, like in the reference (it takes an existing directory as 'frames written already').

    ``device``: decode every video there (``loadVideoFrames``) and write its sampled frames with ``saveFrameImages``: the
    same files byte for byte (the device decodes PIL's pixels and encodes PIL's bytes), and no pixel visits the host."""
    if not rootDir.endswith("/"):
        rootDir = rootDir + "/"
    if not saveDir.endswith("/"):
        saveDir = saveDir + "/"
    with open(videoListLoc, "r") as videoListFile:
        for line in videoListFile:
            videoLoc, videoName, _, actionCategory, _, _ = videoInfo(line, mode)
            videoLoc = rootDir + videoLoc
            frameDir = saveDir + actionCategory + "/" + videoName
            if all(checkAndMakeDirectories(frameDir)):
                continue
            if device is not None:
                if not (os.path.exists(videoLoc) and os.path.isfile(videoLoc)):
                    raise ValueError("Video does not exist: %s" % (videoLoc))
                saveFrameImages(loadVideoFrames(videoLoc, device)[::sampleRate].contiguous(), frameDir, quality=95)
                continue
            frameList = extractEveryNthFrame(videoLoc, sampleRate)
            for i in range(len(frameList)):
                frameList[i].save(frameDir + "/" + str(i) + FRAME_EXTN, quality=95)  # cv2.imwrite's default JPEG quality
    return


def videoInfo(line, mode):
    """Parse one video-list line (Sheet03/utils.py:73-91).

    Returns (videoLoc, videoName, actionLabel or None, actionCategory, ngroup, nclip).
    train lines are ``"Cat/v_Cat_gNN_cNN.avi K"`` (exactly one space), test lines have no label.
    Raises ValueError exactly where the reference's tuple unpacking does (wrong number of
    ``" "``, ``"/"`` or ``"_"`` separated parts).
    """
    actionLabel = None
    if mode == "train":
        videoLoc, actionLabel = line.split(" ")
        actionLabel = actionLabel.strip()
    else:
        videoLoc = line
    videoLoc = videoLoc.strip()
    actionCategory, videoName = videoLoc.split("/")
    actionCategory = actionCategory.strip()
    videoName = videoName[:videoName.rfind(".")]
    _, _, ngroup, nclip = videoName.split("_")
    return videoLoc, videoName, actionLabel, actionCategory, ngroup, nclip


def spatialFrameIndex(nFrames, r=None):
    """Index of the frame ``SpatialDataset.__getitem__`` opens: ``random.randint(0, nFrames-1)``,
    both ends inclusive (Sheet03/spatialModel.py:74-77).  ``r`` overrides the draw (tests)."""
    if nFrames < 1:
        raise ValueError("empty range for randrange() (0, %d, %d)" % (nFrames, nFrames))
    return random.randint(0, nFrames - 1) if r is None else r


def temporalFlowIndices(nFiles, flowSampleSize, r=None):
    """Start index and the 2L interleaved (prefix, index) pairs ``TemporalDataset.__getitem__`` opens
    (Sheet03/temporalModel.py:78-83).

    ``nFlows = nFiles / 2`` is a TRUE division in the reference (``from __future__ import division``)
    and Python 2's ``randint`` rejects a non-integral float bound, so an odd file count raises
    ValueError; the start lies in [1, nFlows - L] (the last flow index nFlows is never read).
    Order: x_s, y_s, x_{s+1}, y_{s+1}, ... (exactly 2L entries).
    """
    nFlows = nFiles / 2
    if nFlows != int(nFlows):
        raise ValueError("non-integer stop for randrange()")
    nFlows = int(nFlows)
    hi = nFlows - flowSampleSize
    if hi < 1:
        raise ValueError("empty range for randrange() (1, %d, %d)" % (hi + 1, hi))
    start = random.randint(1, hi) if r is None else r
    order = []
    for idx in range(start, start + flowSampleSize):
        order.append(("x", idx))
        order.append(("y", idx))
    return start, order


def flowFileName(prefix, idx, extn=".jpg"):
    """``flow_x_0007.jpg`` naming: prefix + 4-digit zero-padded 1-based index (Sheet03/temporalModel.py:80-81)."""
    return prefix + str(idx).zfill(4) + extn


def flowToImages(flow, bound=20.0):
    """flow ``[N,2,H,W]`` float32 (torch or numpy) -> uint8 ``[N,2,H,W]``: the 8-bit flow image
    convention the reference's flow JPEGs follow, ``q = rint(clamp(255*(v+bound)/(2*bound), 0, 255))``
    (the quantisation step of ``va_flow_to_stack``)."""
    f = flow.detach().cpu().numpy() if isinstance(flow, torch.Tensor) else np.asarray(flow)
    f = f.astype(np.float32)
    t = (np.float32(255.0) * (f + np.float32(bound))) / np.float32(2.0 * bound)
    return np.rint(np.clip(t, 0.0, 255.0)).astype(np.uint8)


def saveFlowImages(flow, flowDir, bound=20.0, firstIndex=1, quality=95, restartBlocks=None):
    """Write the flow of the N consecutive pairs of one video as the files the reference reads:
    ``flow_x_%04d.jpg`` / ``flow_y_%04d.jpg``, 1-based, single-channel 'L' JPEGs
    (Sheet03/temporalModel.py:78-81, Sheet03/parameters.py:38-39).  Returns the file count.  ``restartBlocks``: PIL's
    ``restart_marker_blocks``, a restart marker every so many 8x8 blocks, so that the device decoder works on every image
    with more than one lane; None writes the files without restart markers, byte for byte as before.
    ``saveFlowImagesDevice`` writes the same files without bringing the flow to the host."""
    from PIL import Image
    from .parameters import FRAME_EXTN, X_PREFIX_FLOW, Y_PREFIX_FLOW
    checkAndMakeDirectories(flowDir)
    q = flowToImages(flow, bound)
    extra = {} if restartBlocks is None else {"restart_marker_blocks": int(restartBlocks)}
    for k in range(q.shape[0]):
        for prefix, plane in ((X_PREFIX_FLOW, 0), (Y_PREFIX_FLOW, 1)):
            Image.fromarray(q[k, plane], mode="L").save(os.path.join(flowDir, flowFileName(prefix, firstIndex + k, FRAME_EXTN)),
                                                         quality=quality, **extra)
    return 2 * q.shape[0]


def saveFlowImagesDevice(flow, flowDir, device, bound=20.0, firstIndex=1, quality=95, restartBlocks=None):
    """``saveFlowImages`` on ``device``, the mirror of ``loadFlowImages(device=)``: a float32 flow
    ``[N,2,H,W]`` is quantised there (``flow.quantize_flow``), a uint8 one (a stored flow) is taken as it is, all ``2 N``
    planes are encoded in one ``jpeg.encode_jpegs`` call, and the files ``saveFlowImages`` writes for the same flow,
    ``quality`` and ``restartBlocks`` come out byte for byte.  (A function of its own: the signature of ``saveFlowImages``
    is held by the tests as it stands.)  Returns the file count; ValueError for another dtype or shape and as
    ``jpeg.encode_jpegs``."""
    from . import flow as vflow
    from . import jpeg
    from .parameters import FRAME_EXTN, X_PREFIX_FLOW, Y_PREFIX_FLOW
    t = flow if isinstance(flow, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(flow))
    if t.dim() != 4 or t.shape[1] != 2 or t.dtype not in (torch.float32, torch.uint8):
        raise ValueError("saveFlowImagesDevice: flow must be float32 or uint8 [N,2,H,W], got %s %s" % (t.dtype, list(t.shape)))
    t = t.to(device).contiguous()
    q = t if t.dtype == torch.uint8 else vflow.quantize_flow(t, bound)
    files = jpeg.encode_jpegs(q.view(2 * q.shape[0], q.shape[2], q.shape[3]), quality=quality, restart_blocks=restartBlocks)
    checkAndMakeDirectories(flowDir)
    for i, data in enumerate(files):
        name = flowFileName((X_PREFIX_FLOW, Y_PREFIX_FLOW)[i % 2], firstIndex + i // 2, FRAME_EXTN)
        with open(os.path.join(flowDir, name), "wb") as f:
            f.write(data)
    return len(files)


def _flowImagePaths(flowDir, first, count):
    """Yields the ``[x path, y path]`` pairs ``loadFlowImages`` reads, in order; ValueError for a bad ``count`` and, when its
    pair is reached, for a missing file."""
    from .parameters import FRAME_EXTN, X_PREFIX_FLOW, Y_PREFIX_FLOW
    first = int(first)
    if count is not None and int(count) < 1:
        raise ValueError("loadFlowImages: count must be >= 1, got %r" % (count,))
    seen, k = False, first
    while count is None or k < first + int(count):
        paths = [os.path.join(flowDir, flowFileName(prefix, k, FRAME_EXTN)) for prefix in (X_PREFIX_FLOW, Y_PREFIX_FLOW)]
        there = [os.path.isfile(p) for p in paths]
        if count is None and not any(there) and seen:
            break
        if not all(there):
            raise ValueError("loadFlowImages: missing %s" % paths[there.index(False)])
        yield paths
        seen, k = True, k + 1


def loadFlowImages(flowDir, first=1, count=None, device=None):
    """The reader of what ``saveFlowImages`` and the reference's flow directory hold: ``flow_x_%04d.jpg`` /
    ``flow_y_%04d.jpg`` from index ``first`` (1-based) on -> uint8 numpy ``[N,2,H,W]``, plane 0 x and plane 1 y, a uint8
    stored flow once on the device.  ``count``: how many pairs to read; None reads on until an index has
    neither file.  ValueError for a missing file, images of different sizes and an image that is not single-channel 'L'.

    ``device``: decode all ``2 N`` images on that device in one call -> a uint8 tensor ``[N,2,H,W]``
    there, the same bytes and the same ValueErrors; files outside the decoder's subset raise ValueError too."""
    from PIL import Image
    if device is not None:
        from . import jpeg
        hdrs = []
        for paths in _flowImagePaths(flowDir, first, count):
            for p in paths:
                with open(p, "rb") as f:
                    hdr = jpeg.parse_jpeg(f.read())
                if len(hdr["components"]) != 1:
                    raise ValueError("loadFlowImages: %s has %d components, not the single-channel 'L' of flow images"
                                     % (p, len(hdr["components"])))
                if hdrs and (hdr["width"], hdr["height"]) != (hdrs[0]["width"], hdrs[0]["height"]):
                    raise ValueError("loadFlowImages: %s is %dx%d, not the size of the images before it"
                                     % (paths[0], hdr["width"], hdr["height"]))
                hdrs.append(hdr)
        out, _ = jpeg.decode_jpegs(hdrs, device)
        return out.view(len(hdrs) // 2, 2, out.shape[1], out.shape[2])
    fields = []
    for paths in _flowImagePaths(flowDir, first, count):
        planes = []
        for p in paths:
            with Image.open(p) as img:
                if img.mode != "L":
                    raise ValueError("loadFlowImages: %s has mode %r, not the single-channel 'L' of flow images" % (p, img.mode))
                planes.append(np.asarray(img, dtype=np.uint8))
        if planes[0].shape != planes[1].shape or (fields and planes[0].shape != fields[0].shape[1:]):
            raise ValueError("loadFlowImages: %s is %dx%d, not the size of the images before it"
                             % (paths[0], planes[1].shape[1], planes[1].shape[0]))
        fields.append(np.stack(planes))
    return np.stack(fields)


# ----------------------------------------------------------------------------- transforms ------

class RandomCrop(object):
    """``transforms.RandomCrop(224)``: top = randint(0, h-th), left = randint(0, w-tw)."""

    def __init__(self, size):
        self.size = (int(size), int(size))

    def __call__(self, img):
        h, w = img.shape[0], img.shape[1]
        th, tw = self.size
        if w == tw and h == th:
            return img
        if h < th or w < tw:
            raise ValueError("Required crop size %s is larger than input image size %s" % ((th, tw), (h, w)))
        i = random.randint(0, h - th)
        j = random.randint(0, w - tw)
        return img[i:i + th, j:j + tw]


class RandomHorizontalFlip(object):
    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, img):
        if random.random() < self.p:
            return img[:, ::-1]
        return img


# ---- colour jitter: PIL's arithmetic on numpy u8 arrays, op by op ----

JITTER_NONE, JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION, JITTER_HUE = 0, 1, 2, 3, 4


def blendU8(d, v, f):
    """``Image.blend(degenerate, image, f)`` on u8 values: ``t = d + f*(v - d)`` in float32, multiply then add; for
    ``0 <= f <= 1`` the result is ``(u8)(int)t``, otherwise 0 where ``t <= 0``, 255 where ``t >= 255``, else ``(int)t``."""
    f = np.float32(f)
    d = np.asarray(d).astype(np.int32)
    v = np.asarray(v).astype(np.int32)
    t = d.astype(np.float32) + f * (v - d).astype(np.float32)
    if not (f >= 0 and f <= 1):
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.int32).astype(np.uint8)


def grayLevel(img):
    """PIL's ``convert('L')`` of an HWC RGB u8 array: ``(19595 R + 38470 G + 7471 B + 32768) >> 16``; an HW array is its
    own gray level."""
    a = np.asarray(img)
    if a.ndim == 2:
        return a.astype(np.uint8)
    a = a.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 32768) >> 16).astype(np.uint8)


def contrastMean(img):
    """The gray value contrast blends with: ``(2 S + N) // (2 N)``, S the sum of ``grayLevel`` over the image and N its
    pixel count (the mean rounded half up, in integers)."""
    L = grayLevel(img)
    S, N = int(L.sum(dtype=np.int64)), int(L.size)
    return (2 * S + N) // (2 * N)


def adjustBrightness(img, f):
    return blendU8(0, img, f)


def adjustContrast(img, f, m=None):
    """``m``: the degenerate gray value; None takes the image's own ``contrastMean``."""
    return blendU8(contrastMean(img) if m is None else int(m), img, f)


def adjustSaturation(img, f):
    a = np.asarray(img)
    if a.ndim == 2:
        return a
    return blendU8(grayLevel(a)[..., None], a, f)


def rgbToHsv(img):
    """PIL's ``convert('HSV')`` of an HWC RGB u8 array, with its operand widths: the saturation and the three channel
    ratios are float32 divisions, the hue expression and ``fmod(h/6 + 1, 1)`` are evaluated in double and rounded to
    float32, and both scalings by 255 are double products truncated to integers."""
    a = np.asarray(img).astype(np.int32)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    gray = mx == mn
    cr = np.where(gray, 1, mx - mn).astype(np.float32)
    s = cr / np.where(gray, 1, mx).astype(np.float32)
    rc, gc, bc = ((mx - c).astype(np.float32) / cr for c in (r, g, b))
    rc64, gc64, bc64 = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
    h = np.where(r == mx, bc64 - gc64, np.where(g == mx, 2.0 + rc64 - bc64, 4.0 + gc64 - rc64)).astype(np.float32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    return np.stack([np.where(gray, 0, uh), np.where(gray, 0, us), mx], axis=-1).astype(np.uint8)


def _roundHalfAway(x):
    """C ``round`` of non-negative doubles."""
    fl = np.floor(x)
    return fl + ((x - fl) >= 0.5)


def hsvToRgb(img):
    """PIL's HSV -> RGB on an HWC u8 array: ``h6 = h*6/255``, ``i = floor(h6)``, ``f = h6 - i`` and ``fs = s/255`` rounded to
    float32, the product ``fs*f`` in float32, the rest in double; ``p, q, t`` by C ``round``."""
    a = np.asarray(img)
    h, s, v = a[..., 0].astype(np.float64), a[..., 1].astype(np.float64), a[..., 2].astype(np.float64)
    h6 = h * 6.0 / 255.0
    i = np.floor(h6)
    f = (h6 - i).astype(np.float32)
    fs = (s / 255.0).astype(np.float32)
    f64, fs64 = f.astype(np.float64), fs.astype(np.float64)
    p = _roundHalfAway(v * (1.0 - fs64))
    q = _roundHalfAway(v * (1.0 - (fs * f).astype(np.float64)))
    t = _roundHalfAway(v * (1.0 - fs64 * (1.0 - f64)))
    p, q, t = (np.clip(x, 0, 255).astype(np.uint8) for x in (p, q, t))
    v8, k = a[..., 2], i.astype(np.int32) % 6
    r = np.choose(k, [v8, q, p, p, t, v8])
    g = np.choose(k, [t, v8, v8, q, p, p])
    b = np.choose(k, [p, p, t, v8, v8, q])
    flat = a[..., 1] == 0
    return np.stack([np.where(flat, v8, r), np.where(flat, v8, g), np.where(flat, v8, b)], axis=-1).astype(np.uint8)


def hueShift(hueFactor):
    """``(int)(hue_factor * 255)``, truncated toward zero, modulo 256: the u8 wrap-around add of the hue plane."""
    return int(hueFactor * 255) % 256


def adjustHue(img, shift):
    """``shift``: the integer of ``hueShift``."""
    a = np.asarray(img)
    if a.ndim == 2:
        return a
    hsv = rgbToHsv(a)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) & 255
    return hsvToRgb(hsv)


def applyLighting(img, off):
    """PCA lighting: ``(u8) rint(clamp((float)v + off_c, 0, 255))`` with one float32 offset per channel of an HWC array."""
    a = np.asarray(img).astype(np.float32) + np.asarray(off, dtype=np.float32)
    return np.rint(np.clip(a, np.float32(0), np.float32(255))).astype(np.uint8)


def checkColorJitter(brightness, contrast, saturation, hue):
    """torchvision's parameter rules: ValueError unless brightness, contrast, saturation >= 0 and 0 <= hue <= 0.5."""
    for name, p in (("brightness", brightness), ("contrast", contrast), ("saturation", saturation)):
        if not p >= 0:
            raise ValueError("ColorJitter: %s must be >= 0, got %r" % (name, p))
    if not (hue >= 0 and hue <= 0.5):
        raise ValueError("ColorJitter: hue must lie in [0, 0.5], got %r" % (hue,))


def drawColorJitter(rng, brightness, contrast, saturation, hue):
    """The draws of one image -> ``[(op, value), ...]`` in application order: in the order brightness,
    contrast, saturation, hue every non-zero parameter draws one number (``uniform(max(0, 1-p), 1+p)``; hue
    ``uniform(-p, p)``, kept as the integer ``hueShift``), then ``rng.shuffle`` of the active ops.  All zero: no call."""
    ops = []
    for op, p in ((JITTER_BRIGHTNESS, brightness), (JITTER_CONTRAST, contrast), (JITTER_SATURATION, saturation)):
        if p:
            ops.append((op, rng.uniform(max(0, 1 - p), 1 + p)))
    if hue:
        ops.append((JITTER_HUE, hueShift(rng.uniform(-hue, hue))))
    if ops:
        rng.shuffle(ops)
    return ops


def applyColorJitter(img, ops):
    """``ops``: ``[(op, value), ...]`` as ``drawColorJitter`` gives them, applied in order to an HWC or HW u8 array."""
    fn = {JITTER_BRIGHTNESS: adjustBrightness, JITTER_CONTRAST: adjustContrast, JITTER_SATURATION: adjustSaturation,
          JITTER_HUE: adjustHue}
    a = np.asarray(img)
    for op, value in ops:
        if op != JITTER_NONE:
            a = fn[op](a, value)
    return a


class ColorJitter(object):
    """``transforms.ColorJitter`` on HWC (RGB) or HW ('L') u8 arrays: PIL's arithmetic, this project's
    draw order.  On an HW array brightness and contrast act on the plane, saturation and hue leave it as it is.
    ``ColorJitter(0,0,0,0)`` (Sheet03/parameters.py:21) is the identity and draws no random numbers."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, rng=None):
        checkColorJitter(brightness, contrast, saturation, hue)
        self.params = (brightness, contrast, saturation, hue)
        self.rng = rng

    def __call__(self, img):
        ops = drawColorJitter(random if self.rng is None else self.rng, *self.params)
        return applyColorJitter(img, ops) if ops else img


class ToTensor(object):
    """u8 HWC (or HW) -> float32 CHW / 255."""

    def __call__(self, img):
        a = np.ascontiguousarray(img)
        if a.ndim == 2:
            a = a[:, :, None]
        t = torch.from_numpy(a.transpose(2, 0, 1).copy())
        return t.to(torch.float32).div(255)


class Normalize(object):
    """Per-channel (t - mean)/std over ``zip(tensor, mean, std)``: a 1-channel flow image therefore
    uses only the FIRST mean/std pair (0.485 / 0.229) -- SURVEY.md a5, appendix quirk 3."""

    def __init__(self, mean, std):
        self.mean, self.std = list(mean), list(std)

    def __call__(self, t):
        out = t.clone()
        for c, (m, s) in enumerate(zip(self.mean, self.std)):
            if c >= out.shape[0]:
                break
            out[c] = (out[c] - m) / s
        return out


class Compose(object):
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, img):
        img = np.asarray(img)
        for t in self.transforms:
            img = t(img)
        return img


def getTransforms(cropSize=CROP_SIZE_TF, hortizontalFlip=HORIZONTAL_FLIP_TF, normMeans=NORM_MEANS_TF,
                  normStds=NORM_STDS_TF, jitter=COLOR_JITTERS):
    """Sheet03/utils.py:137-151.  The crop is the literal 224 of the reference whatever ``cropSize``
    says (``:143``); the same random transforms are used at test time (Sheet03/spatialModel.py:293-294)."""
    imgTrans = []
    if cropSize:
        imgTrans.append(RandomCrop(224))
    if hortizontalFlip:
        imgTrans.append(RandomHorizontalFlip())
    if jitter:
        imgTrans.append(ColorJitter(*jitter))
    imgTrans.append(ToTensor())
    if normMeans and normStds:
        imgTrans.append(Normalize(mean=normMeans, std=normStds))
    return Compose(imgTrans)


class TenCrop(object):
    """Ten-crop evaluation (the test protocol of the two-stream paper; torchvision's ``TenCrop``): an image -> float32
    ``[10,C,224,224]``, the four corners and the centre, then the same five of the mirrored image
    (``augment.ten_crop_views``), each through ``ToTensor`` and ``Normalize``.  ``nViews`` tells the datasets that one
    image gives ten.  ``flowX=True`` marks an x-flow image: with ``invertFlowX`` its mirrored views are inverted,
    ``q -> 255 - q`` (TSN flips: mirroring reverses horizontal motion).  Draws no random numbers."""

    nViews = 10

    def __init__(self, size=224, normMeans=NORM_MEANS_TF, normStds=NORM_STDS_TF, invertFlowX=False):
        self.size = int(size)
        self.invertFlowX = bool(invertFlowX)
        self.toTensor = ToTensor()
        self.normalize = Normalize(mean=normMeans, std=normStds) if normMeans and normStds else None

    def __call__(self, img, flowX=False):
        from .augment import ten_crop_views
        a = np.asarray(img)
        s = self.size
        out = []
        for top, left, flip in ten_crop_views(a.shape[0], a.shape[1], s).tolist():
            v = a[top:top + s, left:left + s]
            if flip:
                v = v[:, ::-1]
                if flowX and self.invertFlowX:
                    v = (255 - v.astype(np.int32)).astype(a.dtype)
            t = self.toTensor(v)
            out.append(self.normalize(t) if self.normalize is not None else t)
        return torch.stack(out)


def getTenCropTransforms(normMeans=NORM_MEANS_TF, normStds=NORM_STDS_TF, invertFlowX=False):
    """The deterministic test-time counterpart of ``getTransforms()``: ten 224x224 views of every image (``TenCrop``),
    for ``SpatialDataset`` / ``TemporalDataset`` and the five-dimensional batches ``validate()`` then averages over."""
    return TenCrop(224, normMeans, normStds, invertFlowX)


def getDataLoader(dataset, batchSize=TEMPORAL_BATCH_SIZE, nWorkers=NWORKERS_LOADER, shuffle=SHUFFLE_LOADER):
    """Sheet03/utils.py:125-133: default collate, last batch partial, shuffle on (also for test)."""
    return DataLoader(dataset=dataset, batch_size=batchSize, shuffle=shuffle, num_workers=nWorkers)


class AverageMeter(object):
    """Running mean (Sheet03/utils.py:154-171)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def saveVideoDescriptors(videoDescDict, csvLoc, gpu=False):
    """One CSV row per video: ``name,label,`` then the descriptor as float64 reprs
    (Sheet03/utils.py:174-195; the width is VIDEO_DESCRIPTOR_DIM = 256, not the docstring's 4096)."""
    try:
        os.remove(csvLoc)
    except OSError:
        pass
    with open(csvLoc, "a") as csvFile:
        writer = csv.writer(csvFile, delimiter=",")
        for videoName in videoDescDict.keys():
            label = videoDescDict[videoName][1]
            videoLabel = label.cpu().numpy() if isinstance(label, torch.Tensor) else np.asarray(label)
            csvFile.write(videoName + "," + str(videoLabel) + ",")
            videoDesc = videoDescDict[videoName][0].avg
            videoDesc = videoDesc.detach().cpu().numpy().astype(float)
            writer.writerow(videoDesc)
