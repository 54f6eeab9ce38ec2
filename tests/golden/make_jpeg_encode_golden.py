"""Writes tests/golden/jpeg_encode_small.npz: small images, from seeds, and the bytes PIL (libjpeg-turbo) wrote for them where
this file ran -- the contract of the device encoder, so that the PIL of the machine that runs the tests is
no part of it.  Every case is encoded by the host model as well, which must give PIL's bytes, and its counters are asserted:
the set really holds stuffed bytes, ZRL, blocks without EOB, dummy blocks, every number of fill bits named below, ...

    python tests/golden/make_jpeg_encode_golden.py

Per case k of the list ``cases`` (a JSON string: name, quality, subsampling, restart): ``img_k`` uint8 [n,h,w] or [n,3,h,w],
``bytes_k`` uint8, the n files back to back, ``lens_k`` their lengths."""
import io
import json
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from video_analytics_amd import jpeg  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_encode_small.npz")


def pil_bytes(img, quality, subsampling, restart):
    f = io.BytesIO()
    im = Image.fromarray(img if img.ndim == 2 else np.ascontiguousarray(img.transpose(1, 2, 0)))
    extra = {} if restart is None else {"restart_marker_blocks": restart}
    im.save(f, "JPEG", quality=quality, subsampling=subsampling, **extra)
    return f.getvalue()


def textured(rng, h, w, colour):
    yy, xx = np.mgrid[0:h, 0:w]
    planes = []
    for c in range(3 if colour else 1):
        a = 128 + 70 * np.sin(xx / (2.0 + c) + c) * np.cos(yy / (3.0 + c)) + 30 * np.sin((xx + 2 * yy) / 7.0)
        planes.append(np.clip(a + rng.integers(-12, 13, (h, w)), 0, 255).astype(np.uint8))
    return np.stack(planes) if colour else planes[0]


def noise(rng, h, w, colour):
    return rng.integers(0, 256, (3, h, w) if colour else (h, w), dtype=np.uint8)


def ramp(rng, h, w, colour):
    """A smooth ramp with a flat band and a faint checkerboard in one corner: zero blocks, long zero runs in front of the
    highest frequencies."""
    yy, xx = np.mgrid[0:h, 0:w]
    a = (2 * xx + yy).astype(np.int64)
    a[:, : w // 2] = 90
    a[h // 2:, w // 2:] += 80 * ((xx + yy)[h // 2:, w // 2:] & 1)
    a = np.clip(a, 0, 255).astype(np.uint8)
    return np.stack([a, a, 255 - a]) if colour else a


def extreme(rng, h, w, colour):
    """Black and white 8x8 squares with a little noise, on the block grid in the first 16 columns (the largest DC differences) and
    four pixels off it behind them (the largest AC values)."""
    yy, xx = np.mgrid[0:h, 0:w]
    a = 255 * ((np.where(xx < 16, xx, xx + 4) // 8 + yy // 8) & 1)
    a = (a ^ rng.integers(0, 4, (h, w))).astype(np.uint8)
    return np.stack([a, a, a]) if colour else a


MAKERS = dict(textured=textured, noise=noise, ramp=ramp, extreme=extreme)

# name, maker, (h, w), colour, n, quality, subsampling, restart
SPEC = [
    ("gray_3x3_q95", "textured", (3, 3), False, 1, 95, 0, None),
    ("gray_8x8_q50", "textured", (8, 8), False, 1, 50, 0, None),
    ("gray_17x8_q75", "textured", (17, 8), False, 1, 75, 0, None),
    ("gray_37x53_q95", "textured", (37, 53), False, 1, 95, 0, None),
    ("gray_40x24_q1", "textured", (40, 24), False, 1, 1, 0, None),
    ("gray_40x24_noise_q100", "noise", (40, 24), False, 1, 100, 0, None),
    ("gray_40x24_extreme_q100", "extreme", (40, 24), False, 1, 100, 0, None),
    ("gray_48x64_ramp_q20", "ramp", (48, 64), False, 1, 20, 0, None),
    ("gray_47x33_r3", "textured", (47, 33), False, 1, 95, 0, 3),
    ("gray_47x33_noise_q100_r3", "noise", (47, 33), False, 1, 100, 0, 3),
    ("gray_17x8_r1000", "textured", (17, 8), False, 1, 75, 0, 1000),
    ("c444_17x8_q95", "textured", (17, 8), True, 1, 95, 0, None),
    ("c444_17x8_noise_q100_r1", "noise", (17, 8), True, 1, 100, 0, 1),
    ("c422_37x19_q95", "textured", (37, 19), True, 1, 95, 1, None),
    ("c422_30x19_q50", "textured", (30, 19), True, 1, 50, 1, None),
    ("c422_37x19_noise_q100_r2", "noise", (37, 19), True, 1, 100, 1, 2),
    ("c420_53x37_q95", "textured", (53, 37), True, 1, 95, 2, None),
    ("c420_40x24_q75", "textured", (40, 24), True, 1, 75, 2, None),
    ("c420_16x16_q1", "textured", (16, 16), True, 1, 1, 2, None),
    ("c420_53x37_noise_q100", "noise", (53, 37), True, 1, 100, 2, None),
    ("c420_53x37_r1", "textured", (53, 37), True, 1, 95, 2, 1),
    ("c420_53x37_row", "textured", (53, 37), True, 1, 75, 2, 3),   # three MCUs across: one interval per MCU row
    ("c420_40x24_ramp_q30", "ramp", (40, 24), True, 1, 30, 2, None),
    ("c420_16x16_r1000", "textured", (16, 16), True, 1, 50, 2, 1000),
    # more than 256 blocks: the entropy workgroup takes them in rounds, an interval (and an MCU) across the round's end
    ("gray_136x160_r7", "textured", (136, 160), False, 1, 75, 0, 7),
    ("c420_136x160_r4", "textured", (136, 160), True, 1, 75, 2, 4),
    ("batch5_gray_19x30_r2", "textured", (19, 30), False, 5, 95, 0, 2),
    ("batch5_c420_24x40", "textured", (24, 40), True, 5, 95, 2, None),
    ("batch70_gray_16x24_r2", "textured", (16, 24), False, 70, 95, 0, 2),
]


def main():
    cases, arrays = [], {}
    total = {}
    paddings = set()
    per_case = {}
    for k, (name, maker, (h, w), colour, n, quality, sub, restart) in enumerate(SPEC):
        rng = np.random.default_rng(1000 + k)
        if n == 70:
            two = [MAKERS[maker](rng, h, w, colour) for _ in range(2)]
            imgs = np.stack([two[i % 2] for i in range(n)])
        else:
            imgs = np.stack([MAKERS[maker](rng, h, w, colour) for _ in range(n)])
        files = [pil_bytes(im, quality, sub, restart) for im in imgs]
        c = {}
        mine = jpeg.encode_jpegs_host(imgs, quality, sub, restart, counters=c)
        assert mine == files, "%s: the host model does not write PIL's bytes" % name
        for f, im in zip(files, imgs):  # and the project's decoder reads them back as PIL does
            hdr = jpeg.parse_jpeg(f)
            assert hdr["restart_interval"] == (restart or 0)
        per_case[name] = c
        paddings.update(c["padding"])
        for key, v in c.items():
            if key == "padding":
                continue
            total[key] = max(total.get(key, 0), v) if key.startswith("max_") else total.get(key, 0) + v
        cases.append(dict(name=name, quality=quality, subsampling=sub, restart=restart))
        arrays["img_%d" % k] = imgs
        arrays["bytes_%d" % k] = np.frombuffer(b"".join(files), dtype=np.uint8)
        arrays["lens_%d" % k] = np.asarray([len(f) for f in files], dtype=np.int64)
    # what the set must hold
    c = per_case
    assert c["gray_40x24_noise_q100"]["stuffed"] > 0, c["gray_40x24_noise_q100"]
    assert c["gray_40x24_extreme_q100"]["max_dc_category"] == 11 and c["gray_40x24_extreme_q100"]["max_ac_category"] == 10, \
        c["gray_40x24_extreme_q100"]
    assert c["gray_48x64_ramp_q20"]["zrl"] > 0 and c["gray_48x64_ramp_q20"]["zero_blocks"] > 0, c["gray_48x64_ramp_q20"]
    assert c["c420_40x24_ramp_q30"]["zrl"] > 0 and c["c420_40x24_ramp_q30"]["zero_blocks"] > 0, c["c420_40x24_ramp_q30"]
    assert total["no_eob"] > 0 and total["eob"] > 0, total
    assert c["gray_47x33_r3"]["segments"] == 10 and c["gray_47x33_noise_q100_r3"]["segments"] == 10
    assert c["gray_47x33_noise_q100_r3"]["stuffed"] > 0
    assert c["c420_53x37_r1"]["segments"] == 12 and c["c420_53x37_row"]["segments"] == 4
    assert c["gray_17x8_r1000"]["segments"] == 1 and c["c420_16x16_r1000"]["segments"] == 1
    assert c["c422_37x19_q95"]["dummy_blocks"] == 5 and c["c420_53x37_q95"]["dummy_blocks"] == 6 * 8 - 5 * 7, \
        (c["c422_37x19_q95"], c["c420_53x37_q95"])  # a luma grid of 4x5 for 3x5 real blocks; of 6x8 for 5x7
    assert "dummy_blocks" not in c["c420_16x16_q1"] and "dummy_blocks" not in c["gray_37x53_q95"]
    assert {0, 7} <= paddings, paddings
    assert 256 % 7 and (256 // 6) % 4 and 256 % 6  # round ends inside an interval of both large cases, and inside an MCU
    lens = arrays["lens_%d" % [s[0] for s in SPEC].index("batch5_gray_19x30_r2")]
    assert len(set(lens.tolist())) > 1, lens
    arrays["cases"] = np.asarray(json.dumps(cases))
    np.savez_compressed(OUT, **arrays)
    print("wrote %s: %d cases, %d bytes; totals %s; fill bits met %s" % (OUT, len(cases), os.path.getsize(OUT), total, sorted(paddings)))


if __name__ == "__main__":
    main()
