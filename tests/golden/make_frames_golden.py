"""Builds tests/golden/frames_small.npz with PIL, the judge of DESIGN.md S36: ``Image.resize((ow, oh), Image.BILINEAR)`` and
``convert('L')`` of seeded random RGB frames.

    python tests/golden/make_frames_golden.py

Per case ``NAME`` (``HxW_to_OHxOW``) the file holds ``in_NAME`` u8 ``[2,h,w,3]`` (two frames, HWC as PIL reads them),
``rgb_NAME`` u8 ``[2,oh,ow,3]`` and ``gray_NAME`` u8 ``[2,oh,ow]``.  Frame 0 is uniform noise; frame 1 is noise with a band
of 255 and a band of 0 across it (the taps of an output sample sum to 2**22 give or take a few units, so a saturated
neighbourhood is where the final clamp and the rounding offset matter).  Nothing here imports the package: the expected
values are PIL's alone.
"""
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "frames_small.npz")
# (h, w) -> (oh, ow)
CASES = (
    ((37, 53), (16, 23)),   # down on both axes, odd sizes
    ((30, 40), (64, 85)),   # up on both axes
    ((50, 50), (50, 31)),   # the vertical pass is skipped
    ((24, 32), (24, 32)),   # gray only
    ((64, 66), (4, 5)),     # factors 16 and 13.2: the widest taps allowed
    ((9, 7), (1, 1)),
)
FRAMES = 2


def name(case):
    (h, w), (oh, ow) = case
    return "%dx%d_to_%dx%d" % (h, w, oh, ow)


def frames(h, w):
    """u8 [FRAMES,h,w,3]."""
    rs = np.random.RandomState(100 * h + w)
    a = rs.randint(0, 256, size=(FRAMES, h, w, 3)).astype(np.uint8)
    a[1, h // 4:h // 4 + max(h // 5, 1)] = 255
    a[1, :, w // 2:w // 2 + max(w // 6, 1)] = 0
    return a


def compute():
    out = {}
    for case in CASES:
        (h, w), (oh, ow) = case
        a = frames(h, w)
        ims = [Image.fromarray(f).resize((ow, oh), Image.BILINEAR) for f in a]
        out["in_" + name(case)] = a
        out["rgb_" + name(case)] = np.stack([np.asarray(im) for im in ims])
        out["gray_" + name(case)] = np.stack([np.asarray(im.convert("L")) for im in ims])
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **compute())
    print(OUT, os.path.getsize(OUT), "bytes")
