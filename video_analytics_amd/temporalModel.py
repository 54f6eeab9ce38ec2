"""Temporal stream: the reference's ``Sheet03/temporalModel.py`` call surface over the gfx950 kernels.

``TemporalDataset`` reads the precomputed ``flow_x_%04d.jpg`` / ``flow_y_%04d.jpg`` images exactly as
the reference does (Sheet03/temporalModel.py:67-92); ``flowVolumesFromFrames`` is the MI355X-native
replacement of that offline step (frames -> TV-L1 -> 2L-channel flow volume on the GPU).
"""
from __future__ import division

import os

import torch
from PIL import Image
from torch.utils.data import Dataset

from . import flow as vflow
from . import synth, vgg
from .parameters import *  # noqa: F401,F403
from .parameters import (FRAME_EXTN, TEMPORAL_TEST_CSV_LOC, VIDEO_INPUT_FLOW_COUNT, X_PREFIX_FLOW, Y_PREFIX_FLOW)
from .spatialModel import SpatialNetwork, _read_label_dict
from .utils import ToTensor, flowFileName, saveVideoDescriptors, temporalFlowIndices, videoInfo


class TemporalDataset(Dataset):
    """2L flow frames from a random start per video per invocation (Sheet03/temporalModel.py:22-92)."""

    def __init__(self, videoListLoc, rootDir, imageTransforms=None, flowSampleSize=VIDEO_INPUT_FLOW_COUNT,
                 mode="train", actionLabelLoc=None):
        super(TemporalDataset, self).__init__()
        self.rootDir = rootDir if rootDir.endswith("/") else rootDir + "/"
        self.imageTransforms = imageTransforms
        self.flowSampleSize = flowSampleSize
        self.mode = mode
        with open(videoListLoc, "r") as videoListFile:
            self.videoList = [line for line in videoListFile]
        if actionLabelLoc is None:
            raise ValueError("Action label dictionary required!")
        self.actionLabelDict = _read_label_dict(actionLabelLoc)

    def __len__(self):
        return len(self.videoList)

    def __getitem__(self, index):
        _, videoName, actionLabel, actionCategory, _, _ = videoInfo(self.videoList[index], self.mode)
        if self.mode == "test":
            actionLabel = self.actionLabelDict[actionCategory]
        actionLabel = int(actionLabel)
        flowDir = self.rootDir + actionCategory + "/" + videoName + "/"
        nFiles = len([fName for fName in os.listdir(flowDir)])
        _, order = temporalFlowIndices(nFiles, self.flowSampleSize)
        flowFrames = [flowDir + flowFileName(X_PREFIX_FLOW if ax == "x" else Y_PREFIX_FLOW, idx, FRAME_EXTN)
                      for (ax, idx) in order]
        # the transform is applied to each of the 2L images independently: 2L independent random
        # crops / flips (Sheet03/temporalModel.py:86, quirk 2)
        tf = self.imageTransforms if self.imageTransforms is not None else ToTensor()
        if getattr(tf, "nViews", None):
            # a multi-view transform (utils.getTenCropTransforms): each image gives [V,1,224,224] and is told whether it
            # is x flow; the volume is [V,2L,224,224], views first, so that the default collate gives [B,V,2L,224,224]
            views = [tf(Image.open(frame), flowX=(ax == "x")) for frame, (ax, _) in zip(flowFrames, order)]
            return torch.cat(views, dim=1), actionLabel, videoName
        loadedFrames = [tf(Image.open(frame)) for frame in flowFrames]
        flowVolume = torch.squeeze(torch.stack(loadedFrames, dim=0))  # [2L,1,H,W] -> [2L,H,W]
        return flowVolume, actionLabel, videoName


def flowVolumesFromFrames(gray, flowSampleSize=VIDEO_INPUT_FLOW_COUNT, tvl1_params=None, bound=vflow.FLOW_BOUND, crops=None,
                          views=None, invert_flow_x=False, motion="stack", mean_flow=False, *, camera_form="subtract",
                          camera="none"):
    """gray CUDA u8/f32 ``[B, L+1, H, W]`` -> flow volumes f32 ``[B, 2L, H, W]`` on the GPU: TV-L1 on the
    L consecutive pairs, 8-bit quantisation, ToTensor+Normalize, x/y interleave -- the tensor
    ``TemporalDataset.__getitem__`` would have assembled from the upstream tool's JPEGs.  ``tvl1_params`` takes an
    ``_ffi.Tvl1Params`` or an ``_ffi.BroxParams``; with the latter the flow is Brox flow (``flow.brox_flow``).
    An ``_ffi.FarnebackParams`` gives Farneback flow (``flow.farneback_flow``).

    ``crops``: CPU int32 ``[B*2L,3]`` (``augment.draw_flow_crops``): frames of any size >= 224 then give
    ``[B, 2L, 224, 224]``, each flow image cropped and flipped by its own row (Sheet03/temporalModel.py:86).
    ``views``: CPU int32 ``[V,3]`` (``augment.ten_crop_views``): ``[B, V, 2L, 224, 224]``, every clip through every view.
    ``invert_flow_x``: with ``crops`` or ``views``, a mirrored x-flow image becomes ``q -> 255 - q`` (TSN flips).
    ``motion``: ``"stack"`` (optical-flow stacking), ``"trajectory"`` (trajectory stacking) or ``"bidirectional"`` (L/2
    forward and L/2 backward fields around frame L/2; L even); ``mean_flow``: every field minus its mean vector (DESIGN.md
    S11-S13).  ``camera``: ``"homography"`` subtracts from every field the displacement field of the homography fitted to it
    (TSN's warped optical flow), before the motion options; ``camera_form="rerun"`` takes TSN's own
    two-pass form instead: every pair's second frame is warped by that homography and TV-L1 runs again on the pair
    (twice the TV-L1 time).  ``"rerun"`` with ``camera="none"`` raises ValueError.  All act on the
    full-frame float flow, before the crops and views."""
    if gray.dim() != 4 or gray.shape[1] != flowSampleSize + 1:
        raise ValueError("flowVolumesFromFrames: gray must be [B,%d,H,W]" % (flowSampleSize + 1))
    if crops is not None and views is not None:
        raise ValueError("flowVolumesFromFrames: crops= and views= exclude each other")
    vflow.check_motion(motion, mean_flow, flowSampleSize, "flowVolumesFromFrames", camera=camera)
    vflow.check_camera_form(camera_form, "flowVolumesFromFrames", camera)
    B, _, H, W = gray.shape
    if views is not None:
        from . import augment
        augment.check_views(views, H, W, 224, "flowVolumesFromFrames")
    if motion == "bidirectional":
        gray = vflow.bidirectional_sequences(gray)
    fl = vflow.apply_motion(vflow.tvl1_flow(gray, tvl1_params), flowSampleSize, motion, mean_flow, camera_form=camera_form,
                            frames=gray, tvl1_params=tvl1_params, camera=camera)
    if views is not None:
        return vflow.crop_flow_to_stack_views(fl, views, flowSampleSize, invert_x_on_flip=invert_flow_x, bound=bound)
    if crops is not None:
        return vflow.crop_flow_to_stack(fl, crops, bound=bound, invert_x_on_flip=invert_flow_x).view(B, 2 * flowSampleSize,
                                                                                                      224, 224)
    return vflow.flow_to_stack(fl, bound=bound).view(B, 2 * flowSampleSize, H, W)


class TemporalNetwork(SpatialNetwork):
    """Wrapper of the motion stream (Sheet03/temporalModel.py:96-312)."""

    def __init__(self, nActionClasses, flowSampleSize, nEpochs, lr, momentumVal, descriptorDim, trainLoader, testLoader,
                 lrMilestones, ckpLoc, gpu=False, weights=None, seed=2, solver=None):
        self.flowSampleSize = flowSampleSize
        self.C_IN = 2 * flowSampleSize
        if weights is None and torch.cuda.is_available():
            dev = torch.device("cuda", torch.cuda.current_device())
            weights = synth.synth_vgg16_weights(c_in=self.C_IN, n_classes=nActionClasses, desc_dim=descriptorDim,
                                                seed=seed, device=dev)
            weights["conv_w"][0] = self.__copyFirstLayer__(weights["conv_w"][0].to(dev))
        super(TemporalNetwork, self).__init__(nActionClasses, nEpochs, lr, momentumVal, descriptorDim, trainLoader,
                                              testLoader, lrMilestones, ckpLoc, gpu=gpu, weights=weights, seed=seed,
                                              solver=solver)

    def __copyFirstLayer__(self, w_rgb):
        """Sheet03/temporalModel.py:149-162: RGB-mean kernel replicated over the 2L input channels
        (the first-layer bias is NOT copied: whatever bias the weights carry is kept)."""
        return vgg.copy_first_layer(w_rgb, 2 * self.flowSampleSize)

    def _build(self, weights):
        if weights["conv_w"][0].shape[1] == 3:
            weights = dict(weights)
            weights["conv_w"] = [self.__copyFirstLayer__(weights["conv_w"][0].to(self.device))] + list(weights["conv_w"][1:])
        return vgg.Vgg16Stream(weights["conv_w"], weights["conv_b"], weights["fc_w"], weights["fc_b"],
                               self.nActionClasses, self.descriptorDim, device=self.device.index)

    CKP_FILE, BEST_FILE = MOTION_CKP_FILE, MOTION_BEST_FILE
    TRAIN_CSV, TEST_CSV, PERFORMANCE_CSV = TEMPORAL_TRAIN_CSV_LOC, TEMPORAL_TEST_CSV_LOC, TEMPORAL_PERFORMANCE_LOC


def main(weights=None):
    """The motion-stream script (Sheet03/temporalModel.py:315-324): datasets over the flow-image directory, loaders,
    network, ``execute()``."""
    from . import parameters as P
    from .utils import getDataLoader, getTransforms
    tf = getTransforms()
    L = P.VIDEO_INPUT_FLOW_COUNT
    trainSet = TemporalDataset(P.VIDEOLIST_TRAIN, P.FLOW_DATA_DIR, tf, flowSampleSize=L, actionLabelLoc=P.ACTIONLABEL_FILE)
    testSet = TemporalDataset(P.VIDEOLIST_TEST, P.FLOW_DATA_DIR, tf, flowSampleSize=L, mode="test",
                              actionLabelLoc=P.ACTIONLABEL_FILE)
    net = TemporalNetwork(P.NACTION_CLASSES, L, P.NEPOCHS, P.INITIAL_LR, P.MOMENTUM_VAL, P.VIDEO_DESCRIPTOR_DIM,
                          getDataLoader(trainSet, batchSize=P.TEMPORAL_BATCH_SIZE),
                          getDataLoader(testSet, batchSize=P.TEMPORAL_BATCH_SIZE), P.MILESTONES_LR, P.CHECKPOINT_DIR,
                          gpu=True, weights=weights)
    return net.execute()


if __name__ == "__main__":
    main()
