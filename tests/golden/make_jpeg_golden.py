"""Builds tests/golden/jpeg_small.npz with PIL, the judge of DESIGN.md S45-S48: small baseline JPEG files and the pixels
PIL (libjpeg) decodes from them.

    python tests/golden/make_jpeg_golden.py

Per case ``NAME`` the file holds ``jpg_NAME``, the file's bytes as uint8, and ``px_NAME``, PIL's pixels: uint8 ``[3,h,w]``
(planar RGB) or ``[h,w]`` for gray files.  The cases (``cases()``): sizes 16x16, 24x40, 37x53, 19x30 and 8x17 (height x
width) in gray, 4:4:4, 4:2:2 and 4:2:0 with the qualities 20, 75, 95 and 100 dealt round; restart markers every 2 and 3 blocks
next to the same image without them; optimised Huffman tables; copies with their DHT segments removed (the decoder then
takes Annex K's tables, as PIL does); five 24x40 4:2:0 images of three table sets and five that share one (``batch_*``,
``shared_*``); and two targeted images: ``checker``, 16x32 gray of alternating black and white 8x8 blocks at quality 100 (DC
differences of category 11), and ``noise``, 32x32 at quality 100 with the standard tables (uniform noise, one quarter of it
saturated to 0 / 255 and one quarter flat but for one pixel of every block), for which the host decoder's counters must
show a code longer than the device's look-ahead table, ZRL, EOB, and IDCT outputs clipped at 0 and at 255.  The expected pixels are PIL's alone; the package is imported only for those counters.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "jpeg_small.npz")
SIZES = ((16, 16), (24, 40), (37, 53), (19, 30), (8, 17))
FORMATS = (("L", None), ("RGB", 0), ("RGB", 1), ("RGB", 2))  # PIL's subsampling: 0 4:4:4, 1 4:2:2, 2 4:2:0
QUALITIES = (20, 75, 95, 100)


def image(h, w, c, seed):
    """A ramp under noise with one flat patch: u8 [h,w,c]."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w]
    base = np.stack([(xx * 5 + yy * 3 + 40 * i) % 256 for i in range(c)], -1)
    a = (base * 0.6 + rs.randint(0, 256, size=(h, w, c)) * 0.4).astype(np.uint8)
    a[h // 3:h // 2, w // 4:w // 2] = rs.randint(0, 2, size=(1, 1, c)) * 255
    return a


def encode(a, mode, sub, quality, **kw):
    im = Image.fromarray(a[..., 0] if mode == "L" else a, mode)
    buf = io.BytesIO()
    if sub is not None:
        kw["subsampling"] = sub
    im.save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def pil_pixels(data):
    """PIL's decode: u8 [3,h,w] or [h,w]."""
    im = Image.open(io.BytesIO(data))
    a = np.asarray(im.convert("L" if im.mode == "L" else "RGB"))
    return np.ascontiguousarray(a if a.ndim == 2 else a.transpose(2, 0, 1))


def strip_dht(data):
    """The file without its DHT segments."""
    out, p = bytearray(data[:2]), 2
    while True:
        assert data[p] == 0xFF
        m, L = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        if m == 0xDA:
            return bytes(out) + data[p:]
        if m != 0xC4:
            out += data[p:p + 2 + L]
        p += 2 + L


def cases():
    """name -> file bytes."""
    out, k = {}, 0
    for si, (h, w) in enumerate(SIZES):
        for fi, (mode, sub) in enumerate(FORMATS):
            q = QUALITIES[(si + fi) % 4]
            k += 1
            fmt = "gray" if mode == "L" else ("444", "422", "420")[sub]
            out["%s_%dx%d_q%d" % (fmt, h, w, q)] = encode(image(h, w, 1 if mode == "L" else 3, 1000 + k), mode, sub, q)
    # restart markers next to the same image without them
    for tag, (h, w), mode, sub, q, blocks in (("420", (37, 53), "RGB", 2, 95, 3), ("gray", (24, 40), "L", None, 75, 2),
                                              ("422", (19, 30), "RGB", 1, 20, 2), ("444", (8, 17), "RGB", 0, 100, 2)):
        a = image(h, w, 1 if mode == "L" else 3, 2000 + blocks + h)
        out["plain_%s_%dx%d" % (tag, h, w)] = encode(a, mode, sub, q)
        out["restart%d_%s_%dx%d" % (blocks, tag, h, w)] = encode(a, mode, sub, q, restart_marker_blocks=blocks)
    out["optimize_420_37x53_q75"] = encode(image(37, 53, 3, 3000), "RGB", 2, 75, optimize=True)
    out["optimize_gray_19x30_q20"] = encode(image(19, 30, 1, 3001), "L", None, 20, optimize=True)
    out["nodht_420_24x40_q95"] = strip_dht(encode(image(24, 40, 3, 3002), "RGB", 2, 95))
    out["nodht_gray_16x16_q75"] = strip_dht(encode(image(16, 16, 1, 3003), "L", None, 75))
    # one call, three table sets (two quantisation levels and one optimised Huffman set) / one shared set
    for i, (q, kw) in enumerate(((20, {}), (75, {}), (95, {"optimize": True}), (75, {}), (20, {}))):
        out["batch_%d" % i] = encode(image(24, 40, 3, 4000 + i), "RGB", 2, q, **kw)
    for i in range(5):
        out["shared_%d" % i] = encode(image(24, 40, 3, 4100 + i), "RGB", 2, 75)
    yy, xx = np.mgrid[:16, :32]
    checker = ((((yy // 8) + (xx // 8)) % 2) * 255).astype(np.uint8)
    out["checker"] = encode(checker[..., None], "L", None, 100)
    rs = np.random.RandomState(5000)
    noise = rs.randint(0, 256, size=(32, 32, 3)).astype(np.uint8)
    noise[:16, 16:] = rs.randint(0, 2, size=(16, 16, 3)) * 255                      # saturated: the IDCT over- and undershoots
    noise[16:, 16:] = 128                                                            # flat but for one pixel of every block: ZRL, EOB
    noise[19::8, 19::8] = 130
    out["noise"] = encode(noise, "RGB", 0, 100)
    return out


def check_targets(files):
    """The targeted cases reach what they are for (the host decoder's counters)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from video_analytics_amd import jpeg
    c = {}
    jpeg.decode_jpegs_host([files["checker"]], c)
    assert c["max_dc_category"] == 11, c
    c = {}
    jpeg.decode_jpegs_host([files["noise"]], c)
    assert c.get("long_codes", 0) > 0 and c.get("zrl", 0) > 0 and c.get("eob", 0) > 0, c
    assert c.get("clip_low", 0) > 0 and c.get("clip_high", 0) > 0, c
    hdr = jpeg.parse_jpeg(files["noise"])
    assert all(tuple(map(list, hdr["huffman"][k])) == tuple(map(list, jpeg.STD_HUFFMAN[k])) for k in jpeg.STD_HUFFMAN)


def compute():
    files = cases()
    check_targets(files)
    out = {}
    for name, data in files.items():
        out["jpg_" + name] = np.frombuffer(data, dtype=np.uint8)
        out["px_" + name] = pil_pixels(data)
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **compute())
    print(OUT, os.path.getsize(OUT), "bytes")
