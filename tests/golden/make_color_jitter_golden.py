"""Builds tests/golden/color_jitter_small.npz with PIL, the judge of DESIGN.md S32: ``ImageEnhance.Brightness / Contrast /
Color`` and ``convert('HSV')`` and back, composed in all 24 orders of the four ops on three random RGB images.

    python tests/golden/make_color_jitter_golden.py

Per image ``NAME`` (``5x7``, ``33x61``, ``224x224``; height x width) the file holds ``table_NAME`` float32 ``[24,8]``, the rows
of ``augment.draw_color_jitter``'s format, one per order, each with its own factors and hue shift.  The two small images are
stored (``image_NAME`` u8 HWC) with their 24 expected outputs (``out_NAME`` u8 ``[24,h,w,3]``).  Twenty-four outputs of the
224x224 image would be 3.6 MB of incompressible bytes, so that image is regenerated from its seed (``image()``; its SHA-256
is stored as ``image_sha_224x224``) and each expected output is stored as its SHA-256 (``sha_224x224`` u8 ``[24,32]``)
beside its per-channel sums (``sums_224x224`` int64 ``[24,3]``): equal digests are equal bits.  ``table_placement`` /
``out_placement``: the 33x61 image through the two-op rows (brightness, contrast) and (contrast, brightness) with the
same factors, whose results differ because brightness moves contrast's gray value.  Nothing here imports the
package: the expected values are PIL's alone.
"""
import hashlib
import itertools
import os

import numpy as np
from PIL import Image, ImageEnhance

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "color_jitter_small.npz")
SIZES = ((5, 7), (33, 61), (224, 224))  # (h, w): 35 and 2013 pixels are no multiples of 4 (the byte tails); 50176 is
STORED = ("5x7", "33x61")
ORDERS = list(itertools.permutations((1, 2, 3, 4)))  # 1 brightness, 2 contrast, 3 saturation, 4 hue


def name(h, w):
    return "%dx%d" % (h, w)


def image(h, w):
    """Random RGB u8 [h,w,3]; 33x61 has a dark band (values 0..3), 224x224 a saturated one (every channel 0 or 255)."""
    rs = np.random.RandomState(1000 * h + w)
    a = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    if (h, w) == (33, 61):
        a[4:9] = rs.randint(0, 4, size=(5, w, 3)).astype(np.uint8)
    if (h, w) == (224, 224):
        a[100:116] = (rs.randint(0, 2, size=(16, w, 3)) * 255).astype(np.uint8)
    return a


def table(h, w):
    """float32 [24,8]: one row per order; factors below and above 1, the first rows at the edges 0, 1 and 2; any hue shift."""
    rs = np.random.RandomState(h * w)
    rows = []
    for i, order in enumerate(ORDERS):
        f = rs.uniform(0.3, 1.9, size=3)
        if i < 3:
            f[i] = (0.0, 1.0, 2.0)[i]
        rows.append(list(order) + [float(x) for x in f] + [int(rs.randint(0, 256))])
    return np.array(rows, dtype=np.float32)


def pil_op(im, op, value):
    """One op on a PIL RGB (or 'L') image: ``value`` the blend factor, for hue the integer shift of the hue plane."""
    if op == 1:
        return ImageEnhance.Brightness(im).enhance(float(value))
    if op == 2:
        return ImageEnhance.Contrast(im).enhance(float(value))
    if op == 3:
        return ImageEnhance.Color(im).enhance(float(value))
    if op == 4:
        if im.mode == "L":
            return im
        h, s, v = im.convert("HSV").split()
        nh = ((np.array(h, dtype=np.uint8).astype(np.int32) + int(value)) & 255).astype(np.uint8)
        return Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
    return im


def pil_row(img, row):
    """A table row applied to a u8 array (HWC RGB or HW) with PIL -> u8 array."""
    im = Image.fromarray(np.ascontiguousarray(img))
    for k in range(4):
        op = int(row[k])
        if op:
            im = pil_op(im, op, row[7] if op == 4 else row[3 + op])
    return np.asarray(im)


def compute():
    out = {}
    for h, w in SIZES:
        nm, img, tab = name(h, w), image(h, w), table(h, w)
        res = np.stack([pil_row(img, row) for row in tab])
        out["table_" + nm] = tab
        if nm in STORED:
            out["image_" + nm] = img
            out["out_" + nm] = res
        else:
            out["image_sha_" + nm] = np.frombuffer(hashlib.sha256(img.tobytes()).digest(), dtype=np.uint8)
            out["sha_" + nm] = np.stack([np.frombuffer(hashlib.sha256(r.tobytes()).digest(), dtype=np.uint8) for r in res])
            out["sums_" + nm] = res.reshape(len(tab), -1, 3).sum(axis=1, dtype=np.int64)
    img = image(33, 61)
    place = np.array([[1, 2, 0, 0, 1.6, 0.5, 1, 0], [2, 1, 0, 0, 1.6, 0.5, 1, 0]], dtype=np.float32)
    out["table_placement"] = place
    out["out_placement"] = np.stack([pil_row(img, row) for row in place])
    assert not np.array_equal(out["out_placement"][0], out["out_placement"][1])
    return out


if __name__ == "__main__":
    np.savez(OUT, **compute())
    print(OUT, os.path.getsize(OUT), "bytes")
