"""Baseline JPEG decoding: the frames of a Motion-JPEG AVI, the numbered frame files and the flow images
both datasets read, decoded on the device value for value as PIL (libjpeg's default decompressor) decodes them.

``parse_jpeg`` walks the markers of one file on the host and splits its entropy-coded bytes at the restart markers;
``decode_jpegs`` packs the segments and tables of a batch into one upload and runs ``va_jpeg_decode``: Huffman decode with one
lane per segment, dequantisation + the "islow" integer IDCT, "fancy" chroma upsampling + the fixed-point YCbCr -> RGB.
``decode_jpegs_host`` states the same decoder in numpy and plain Python integers; the tests hold it to PIL and the kernels
to it.  Baseline files only: one Huffman-coded scan of 8-bit samples, gray or YCbCr 4:4:4 / 4:2:2 / 4:2:0; everything else
raises ValueError from ``parse_jpeg``, before anything touches the device.

The domain of "value for value" (DESIGN.md S47).  The decoders here equal libjpeg wherever each block's dequantised
coefficients are the quantised DCT of some 8x8 block of 8-bit samples, which is what an encoder writes; any entropy coding
of them (tables, restarts, runs, ZRL, symbols libjpeg reads as EOB) is inside.  Outside -- coefficients no pixels give -- the
builds of libjpeg do not agree with each other, so there is no value to equal; device and host model then follow the C
"islow" arithmetic with sums that wrap at 32 bits and a clamp to 0..255.  Measured on the host (PIL 12.2.0 with
libjpeg-turbo, x86-64; nothing of it on a GPU), host model against PIL with its SIMD IDCT / against PIL with the SIMD turned
off (``JSIMD_FORCENONE=1``, libjpeg-turbo's C IDCT), pixels that differ: 63 AC coefficients of +1023 at step 1, 4 / 9 of 64;
63 random +-1023 at step 1 in four blocks, 40 / 117 of 256; +-200 at step 8, 78 / 145 of 256; a lone DC of +-2047 at step
4, 0 / 64 of 64; the two builds differ from each other in 11, 121, 165 and 64 of those pixels.  One coefficient of 1023
anywhere agrees with both, sixteen of them with the SIMD build only.  The C IDCT limits its range through a table indexed
by the low 10 bits, which wraps past +-512; the SIMD one is supposed (not verified) to differ through the 16-bit
intermediates of its first pass and its saturating packs.  Every case of tests/golden/jpeg_streams.npz decodes alike under
both builds.

Encoding is the way back: ``encode_jpegs`` runs ``va_jpeg_encode`` -- colour conversion, downsampling,
the "islow" forward DCT and quantisation with one lane per block, then Huffman coding, byte stuffing and restart markers with
one workgroup per image -- and writes PIL's headers around the scans; ``encode_jpegs_host`` states the same encoder in numpy
and plain Python integers.  Both give, byte for byte, the file ``Image.save`` writes: libjpeg's baseline compressor is integer
arithmetic throughout, so there is one value to equal everywhere.
"""
import re
import struct

import numpy as np

LOOK_BITS = 9  # codes of up to this many bits come from the look-ahead table of the device decoder
STATUS_BAD_CODE, STATUS_BAD_RUN, STATUS_OUT_OF_BITS, STATUS_BAD_SEGMENT = 1, 2, 4, 8  # bits of the per-image status
_STATUS_TEXT = ((STATUS_BAD_CODE, "a code that is in no Huffman table"), (STATUS_BAD_RUN, "a run past coefficient 63"),
                (STATUS_OUT_OF_BITS, "the entropy-coded bytes ran out"), (STATUS_BAD_SEGMENT, "a bad segment table"))

# natural index of the k-th coefficient in zigzag order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                   61, 54, 47, 55, 62, 63], dtype=np.int64)

# Annex K.3 of the JPEG standard: the Huffman tables a file without DHT segments uses (ffmpeg's MJPEG), as (bits, values)
STD_HUFFMAN = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
             [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
              0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
              0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
              0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
              0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
              0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
              0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
              0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
              0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
              0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
              0xf9, 0xfa]),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
              0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
              0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
              0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
              0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
              0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
              0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
              0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
              0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
              0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
              0xf9, 0xfa]),
}

_SCAN_END = re.compile(b"\xff[^\x00\xd0-\xd7\xff]")  # the first marker behind a scan that is neither a stuffed FF nor RSTn
_RST = re.compile(b"\xff[\xd0-\xd7]")

MAX_SAMPLES = 2 ** 31 - 1      # MCU-padded samples of one image, all components: the device counts them in 32 bits (include/va.h)
HUFF_BYTES = 1424              # one device Huffman table: look u16[512], maxcode i32[18], valoff i32[18], vals u8[256]
SET_BYTES = 384 + 6 * HUFF_BYTES  # one table set: quant u16[3][64], then (DC, AC) of component 0, 1, 2 (include/va.h)


_TRUNCATED = "parse_jpeg: truncated header"


def _parse(data):
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise ValueError("parse_jpeg: not a JPEG file (no SOI marker)")
    quant, huff = {}, {}
    frame, restart, jfif, adobe = None, 0, False, None
    p = 2
    while True:
        if p < len(data) and data[p] != 0xFF:
            raise ValueError("parse_jpeg: expected a marker at byte %d" % p)
        while p < len(data) and data[p] == 0xFF:  # fill bytes
            p += 1
        if p >= len(data):
            raise ValueError(_TRUNCATED)
        m = data[p]
        p += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise ValueError("parse_jpeg: the file ends before any scan")
        if p + 2 > len(data):
            raise ValueError(_TRUNCATED)
        (L,) = struct.unpack(">H", data[p:p + 2])
        s = data[p + 2:p + L]
        if L < 2 or len(s) != L - 2:
            raise ValueError(_TRUNCATED)
        p += L
        if m == 0xE0 and s[:5] == b"JFIF\x00":
            jfif = True
        elif m == 0xEE and s[:5] == b"Adobe" and len(s) >= 12:
            adobe = s[11]
        elif m == 0xDB:
            i = 0
            while i < len(s):
                pq, tq = s[i] >> 4, s[i] & 15
                if pq != 0:
                    raise ValueError("parse_jpeg: 16-bit quantisation tables are not supported")
                if tq > 3 or len(s) < i + 65:
                    raise ValueError(_TRUNCATED)
                t = np.zeros(64, dtype=np.uint16)
                t[ZIGZAG] = np.frombuffer(s[i + 1:i + 65], dtype=np.uint8)
                quant[tq] = t
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(s):
                tc, th = s[i] >> 4, s[i] & 15
                bits = list(s[i + 1:i + 17])
                n = sum(bits)
                vals = list(s[i + 17:i + 17 + n])
                if tc > 1 or th > 3 or len(bits) != 16 or len(vals) != n:
                    raise ValueError(_TRUNCATED)
                huff[(tc, th)] = (bits, vals)
                i += 17 + n
        elif m == 0xCC or m in (0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise ValueError("parse_jpeg: arithmetic coding is not supported")
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7):
            raise ValueError("parse_jpeg: only baseline files are supported, not SOF%d (%s)"
                             % (m - 0xC0, "progressive" if m == 0xC2 else "extended, lossless or hierarchical"))
        elif m == 0xC0:
            if frame is not None:
                raise ValueError("parse_jpeg: more than one frame header")
            if len(s) < 6:
                raise ValueError(_TRUNCATED)
            prec, h, w, nc = struct.unpack(">BHHB", s[:6])
            if prec != 8:
                raise ValueError("parse_jpeg: %d-bit samples are not supported, only 8-bit" % prec)
            if nc not in (1, 3):
                raise ValueError("parse_jpeg: %d components are not supported, only 1 (gray) and 3 (YCbCr)" % nc)
            if len(s) < 6 + 3 * nc:
                raise ValueError(_TRUNCATED)
            frame = (w, h, [(s[6 + 3 * i], s[7 + 3 * i] >> 4, s[7 + 3 * i] & 15, s[8 + 3 * i]) for i in range(nc)])
        elif m == 0xDD:
            if len(s) < 2:
                raise ValueError(_TRUNCATED)
            (restart,) = struct.unpack(">H", s[:2])
        elif m == 0xDA:
            if frame is None:
                raise ValueError("parse_jpeg: a scan before the frame header")
            break
    w, h, comps = frame
    nc = len(comps)
    if w < 3 or h < 3:
        raise ValueError("parse_jpeg: %dx%d is below the smallest size, 3x3" % (w, h))
    if len(s) < 1:
        raise ValueError(_TRUNCATED)
    if s[0] != nc or len(s) != 4 + 2 * nc:
        raise ValueError("parse_jpeg: more than one scan (the first holds %d of %d components)" % (s[0], nc))
    if (s[1 + 2 * nc], s[2 + 2 * nc], s[3 + 2 * nc]) != (0, 63, 0):
        raise ValueError("parse_jpeg: not a sequential scan of all 64 coefficients")
    if nc == 3:
        ids = tuple(c[0] for c in comps)
        if not jfif and (adobe == 0 or (adobe is None and ids == (0x52, 0x47, 0x42))):
            raise ValueError("parse_jpeg: a 3-component file that is not YCbCr (Adobe transform 0 or component ids R, G, B)")
        if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            raise ValueError("parse_jpeg: sampling %s is not supported, only 4:4:4, 4:2:2 and 4:2:0"
                             % ",".join("%dx%d" % (c[1], c[2]) for c in comps))
    elif (comps[0][1], comps[0][2]) != (1, 1):
        raise ValueError("parse_jpeg: a gray file with sampling %dx%d, not 1x1" % (comps[0][1], comps[0][2]))
    for key in ((0, 0), (0, 1), (1, 0), (1, 1)):  # libjpeg installs the standard table wherever the file defines none
        huff.setdefault(key, STD_HUFFMAN[key])
    components = []
    for i, (cid, ch, cv, tq) in enumerate(comps):
        if s[1 + 2 * i] != cid:
            raise ValueError("parse_jpeg: the scan lists its components in another order than the frame header")
        td, ta = s[2 + 2 * i] >> 4, s[2 + 2 * i] & 15
        if tq not in quant or (0, td) not in huff or (1, ta) not in huff:
            raise ValueError("parse_jpeg: component %d selects a table the file does not define" % i)
        components.append(dict(id=cid, h=ch, v=cv, tq=tq, td=td, ta=ta))
    hs, vs = comps[0][1], comps[0][2]
    mcu_w, mcu_h = -(-w // (8 * hs)), -(-h // (8 * vs))
    mcus = mcu_w * mcu_h
    samples = 64 * mcus * (hs * vs + (2 if nc == 3 else 0))
    if samples > MAX_SAMPLES:
        raise ValueError("parse_jpeg: %dx%d holds %d samples in its MCUs, more than the %d one image may have" % (w, h, samples, MAX_SAMPLES))
    m = _SCAN_END.search(data, p)
    end = m.start() if m else len(data)
    q = end
    while q + 4 <= len(data) and data[q] == 0xFF:  # what follows the scan: another scan is refused
        while q < len(data) and data[q] == 0xFF:
            q += 1
        if q >= len(data) or data[q] == 0xD9:
            break
        if data[q] == 0xDA:
            raise ValueError("parse_jpeg: more than one scan")
        q += 1 + struct.unpack(">H", data[q + 1:q + 3].ljust(2, b"\x00"))[0]
    scan = data[p:end]
    if restart:
        segments = _RST.split(scan)
        if len(segments) != -(-mcus // restart):
            raise ValueError("parse_jpeg: %d restart intervals for %d MCUs at an interval of %d" % (len(segments), mcus, restart))
    else:
        segments = [scan]
    # an FF that ends a segment is a fill byte in front of the marker behind it (a data FF is followed by its 00)
    segments = [seg.rstrip(b"\xff").replace(b"\xff\x00", b"\xff") for seg in segments]
    return dict(width=w, height=h, components=components, quant=quant, huffman=huff, restart_interval=restart,
                segments=segments, mcus=mcus, mcu_w=mcu_w, mcu_h=mcu_h)


def parse_jpeg(data):
    """One baseline JPEG file (bytes) -> its header, a dict: ``width``, ``height``; ``components``, one dict per component of
    ``id``, the sampling factors ``h`` / ``v`` and the table selectors ``tq`` / ``td`` / ``ta``; ``quant`` {selector: uint16
    [64] in natural order}; ``huffman`` {(class, selector): (bits [16], values)}, Annex K's standard tables wherever the file
    defines none; ``restart_interval`` (MCUs, 0 for none); ``mcu_w`` / ``mcu_h`` / ``mcus``, the MCU grid; and ``segments``,
    the entropy-coded bytes split at the ``RSTn`` markers (one entry without restarts), each with ``FF 00`` un-stuffed.

    ValueError names the reason for: a progressive, extended or lossless frame (anything but SOF0), arithmetic coding,
    12-bit samples, 16-bit quantisation tables, more than one scan, 2 or 4 components, a 3-component file PIL would not take
    as YCbCr (Adobe transform 0, or component ids R, G, B without a JFIF marker), sampling other than 1x1 (gray) or luma 1x1 /
    2x1 / 2x2 with both chroma 1x1, a width or height below 3, more than ``MAX_SAMPLES`` MCU-padded samples, a restart count
    that does not fit the MCUs, and a truncated header."""
    return _parse(bytes(data))


def huffman_table(bits, vals, dc=False):
    """(bits [16], values) of one DHT table -> the decoder's form ``(look uint16 [512], maxcode int32 [18], valoff int32 [18],
    vals uint8 [256])``: ``look[c]`` is ``length << 8 | symbol`` for the code of at most ``LOOK_BITS`` bits that the 9 bits
    ``c`` start with (0: a longer code), ``maxcode[l]`` the largest l-bit value that is a code of length l or starts with a
    shorter one (the last code of length l where there is one; it grows with l, and the first l whose ``maxcode`` holds the
    next l bits is the code's length; -1 before the first code) and ``valoff[l]`` the index of that length's first symbol
    minus its first code.  ValueError for counts no prefix code has."""
    look = np.zeros(1 << LOOK_BITS, dtype=np.uint16)
    maxcode = np.full(18, -1, dtype=np.int32)
    valoff = np.zeros(18, dtype=np.int32)
    out = np.zeros(256, dtype=np.uint8)
    if len(bits) != 16 or sum(bits) != len(vals) or len(vals) > 256:
        raise ValueError("parse_jpeg: a Huffman table of %d symbols with counts for %d" % (len(vals), sum(bits)))
    if dc and any(v > 15 for v in vals):
        raise ValueError("parse_jpeg: a DC Huffman table with a category above 15")
    out[:len(vals)] = vals
    code = k = 0
    for l in range(1, 17):
        n = bits[l - 1]
        if code + n > (1 << l):
            raise ValueError("parse_jpeg: a Huffman table with more codes of %d bits than there are" % l)
        if n:
            valoff[l] = k - code
            if l <= LOOK_BITS:
                for j in range(n):
                    lo = (code + j) << (LOOK_BITS - l)
                    look[lo:lo + (1 << (LOOK_BITS - l))] = (l << 8) | vals[k + j]
            code += n
            k += n
        maxcode[l] = code - 1  # without codes of this length: every l-bit value up to here starts with a shorter code
        code <<= 1
    return look, maxcode, valoff, out


def layout(w, h, ncomp, hs, vs):
    """The block grid of one image as the device keeps it -> a dict: ``mcu_w`` / ``mcu_h``; ``blocks_w`` / ``blocks_h``
    per component (MCU-padded; a gray file is one component of 1x1 blocks); ``block_base``, the first block of every
    component (blocks are kept per component in raster order); ``blocks``, their number; and the same counts times 64 as the
    offsets ``plane_off`` and the size ``plane_bytes`` of the MCU-padded component planes, ``8 blocks_w`` samples a row."""
    if ncomp == 1:
        hs = vs = 1
    mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
    bw = [mw * hs] + [mw] * (ncomp - 1)
    bh = [mh * vs] + [mh] * (ncomp - 1)
    base = [0]
    for c in range(ncomp):
        base.append(base[-1] + bw[c] * bh[c])
    return dict(mcu_w=mw, mcu_h=mh, blocks_w=bw, blocks_h=bh, block_base=base[:-1], blocks=base[-1],
                plane_off=[64 * b for b in base[:-1]], plane_bytes=64 * base[-1])


# ------------------------------------------------------------------------------------------------ the decoder on the host

def _int16(v):
    """The low 16 bits of ``v`` as a signed value, the device's ``(short)``: only the sums of a corrupt file reach it."""
    return ((int(v) + 32768) & 0xFFFF) - 32768


def _decode_segment(seg, first, count, geo, comps, tables, coef, counters):
    """The Huffman decode of one segment into ``coef`` int16 [blocks, 64] (natural order), as one lane of the device
    does it -> status bits."""
    big, total, pos = int.from_bytes(seg, "big"), 8 * len(seg), 0
    hs, vs = comps[0]["h"], comps[0]["v"]
    hv = hs * vs
    nb = hv + 2 if len(comps) == 3 else 1

    def peek16():
        rem = total - pos
        return (big >> (rem - 16)) & 0xFFFF if rem >= 16 else (big << (16 - rem)) & 0xFFFF if rem > 0 else 0

    def symbol(tab):
        nonlocal pos
        look, maxcode, valoff, vals = tab
        c16 = peek16()
        e = int(look[c16 >> (16 - LOOK_BITS)])
        if e:
            pos += e >> 8
            return e & 255
        l = LOOK_BITS + 1
        while l <= 16 and (c16 >> (16 - l)) > maxcode[l]:
            l += 1
        if l > 16:
            return -1
        counters["long_codes"] = counters.get("long_codes", 0) + 1
        pos += l
        return int(vals[(int(valoff[l]) + (c16 >> (16 - l))) & 255])

    def value(s):
        nonlocal pos
        v = peek16() >> (16 - s) if s else 0
        pos += s
        return v if s == 0 or v >= (1 << (s - 1)) else v - (1 << s) + 1

    pred = [0, 0, 0]
    for m in range(first, first + count):
        my, mx = divmod(m, geo["mcu_w"])
        for k in range(nb):
            if k < hv:
                ci, by, bx = 0, my * vs + k // hs, mx * hs + k % hs
            else:
                ci, by, bx = k - hv + 1, my, mx
            dst = coef[geo["block_base"][ci] + by * geo["blocks_w"][ci] + bx]
            dc, ac = tables[ci]
            t = symbol(dc)
            if t < 0:
                return STATUS_BAD_CODE
            if t > counters.get("max_dc_category", 0):
                counters["max_dc_category"] = t
            pred[ci] += value(t & 15)
            dst[0] = _int16(pred[ci])
            i = 1
            while i < 64:
                rs = symbol(ac)
                if rs < 0:
                    return STATUS_BAD_CODE
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if r != 15:
                        counters["eob"] = counters.get("eob", 0) + 1
                        break
                    counters["zrl"] = counters.get("zrl", 0) + 1
                    i += 16
                    continue
                i += r
                if i > 63:
                    return STATUS_BAD_RUN
                dst[ZIGZAG[i]] = _int16(value(s))
                i += 1
            if pos > total:
                return STATUS_OUT_OF_BITS
    return 0


def _idct_pass(a, sh):
    """One 8-point pass of libjpeg's jidctint "islow" IDCT along the last axis of an int32 array; the
    arithmetic wraps at 32 bits like the device's, which valid files never reach."""
    a = a.astype(np.int32)
    c = [a[..., k] for k in range(8)]
    with np.errstate(over="ignore"):
        z1 = (c[2] + c[6]) * np.int32(4433)
        t2 = z1 - c[6] * np.int32(15137)
        t3 = z1 + c[2] * np.int32(6270)
        t0 = (c[0] + c[4]) << 13
        t1 = (c[0] - c[4]) << 13
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        o0, o1, o2, o3 = c[7], c[5], c[3], c[1]
        z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
        z5 = (z3 + z4) * np.int32(9633)
        o0, o1, o2, o3 = o0 * np.int32(2446), o1 * np.int32(16819), o2 * np.int32(25172), o3 * np.int32(12299)
        z1, z2 = z1 * np.int32(-7373), z2 * np.int32(-20995)
        z3, z4 = z3 * np.int32(-16069) + z5, z4 * np.int32(-3196) + z5
        o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
        r = np.int32(1 << (sh - 1))
        out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
        return np.stack([(x + r) >> sh for x in out], axis=-1)


def idct_blocks(coef, quant, counters=None):
    """coef int16 [..., 64] (natural order) times quant [64] (or broadcastable) -> uint8 [..., 8, 8]: dequantisation, the
    column pass with a descale by 11 bits, the row pass with a descale by 18, + 128, clamped.  libjpeg's values for the
    quantised DCT of 8-bit samples; beyond those (the module docstring) the sums wrap at 32 bits and the clamp is a true
    clamp, which no build of libjpeg promises."""
    c = (np.asarray(coef).astype(np.int32) * np.asarray(quant).astype(np.int32)).reshape(np.shape(coef)[:-1] + (8, 8))
    ws = np.swapaxes(_idct_pass(np.swapaxes(c, -1, -2), 11), -1, -2)  # per column
    out = _idct_pass(ws, 18) + 128                                    # per row
    if counters is not None:
        counters["clip_low"] = counters.get("clip_low", 0) + int((out < 0).sum())
        counters["clip_high"] = counters.get("clip_high", 0) + int((out > 255).sum())
    return np.clip(out, 0, 255).astype(np.uint8)


def blocks_to_plane(px, bw, bh):
    """uint8 [bw * bh, 8, 8] blocks in raster order -> the plane uint8 [8 bh, 8 bw]."""
    return px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw)


def upsample_h2v1(s):
    """libjpeg's "fancy" 4:2:2 upsampling of a plane [ch, cw] of real samples -> [ch, 2 cw]:
    ``out[2i] = (3 s[i] + s[i-1] + 1) >> 2``, ``out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2``, the neighbours clamped to the row."""
    s = np.asarray(s).astype(np.int64)
    cw = s.shape[-1]
    i = np.arange(cw)
    out = np.empty(s.shape[:-1] + (2 * cw,), dtype=np.int64)
    out[..., 0::2] = (3 * s + s[..., np.maximum(i - 1, 0)] + 1) >> 2
    out[..., 1::2] = (3 * s + s[..., np.minimum(i + 1, cw - 1)] + 2) >> 2
    return out


def upsample_h2v2(s):
    """libjpeg's "fancy" 4:2:0 upsampling of a plane [ch, cw] of real samples -> [2 ch, 2 cw]: ``v = 3 s[y] + s[y']`` with
    y' the row above for even output rows and below for odd ones, clamped to the plane, then ``out[2i] = (3 v[i] + v[i-1] +
    8) >> 4``, ``out[2i+1] = (3 v[i] + v[i+1] + 7) >> 4``, the neighbours clamped to the row."""
    s = np.asarray(s).astype(np.int64)
    ch, cw = s.shape
    y, i = np.arange(ch), np.arange(cw)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    for odd, other in ((0, np.maximum(y - 1, 0)), (1, np.minimum(y + 1, ch - 1))):
        v = 3 * s + s[other]
        out[odd::2, 0::2] = (3 * v + v[:, np.maximum(i - 1, 0)] + 8) >> 4
        out[odd::2, 1::2] = (3 * v + v[:, np.minimum(i + 1, cw - 1)] + 7) >> 4
    return out


def ycc_to_rgb(y, cb, cr):
    """libjpeg's fixed-point YCbCr -> RGB of three planes [h, w] -> uint8 [3, h, w], with ``F(x) = int(x 65536 + 0.5)``."""
    def F(x):
        return int(x * 65536 + 0.5)
    y, cb, cr = (np.asarray(a).astype(np.int64) for a in (y, cb, cr))
    cb, cr = cb - 128, cr - 128
    r = y + ((F(1.402) * cr + 32768) >> 16)
    g = y + ((-F(0.34414) * cb - F(0.71414) * cr + 32768) >> 16)
    b = y + ((F(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b]), 0, 255).astype(np.uint8)


def planes_to_rgb(planes, w, h, hs, vs):
    """The MCU-padded planes (Y, Cb, Cr) of one image -> uint8 [3, h, w]: only the real ``ceil(w / hs) x ceil(h / vs)``
    chroma samples are neighbours, the padding never is."""
    cw, ch = -(-w // hs), -(-h // vs)
    full = [planes[0][:h, :w]]
    for p in planes[1:]:
        p = p[:ch, :cw]
        if hs == 2:
            p = upsample_h2v2(p) if vs == 2 else upsample_h2v1(p)
        full.append(p[:h, :w])
    return ycc_to_rgb(*full)


def _tables_of(hdr):
    """The decoder's tables of one parsed file: per component ``(DC, AC)`` in ``huffman_table``'s form and the quantisation
    table."""
    huff = [(huffman_table(*hdr["huffman"][(0, c["td"])], dc=True), huffman_table(*hdr["huffman"][(1, c["ta"])]))
            for c in hdr["components"]]
    return huff, [hdr["quant"][c["tq"]] for c in hdr["components"]]


def _segment_mcus(hdr):
    """(first MCU, MCUs) of every segment."""
    ri = hdr["restart_interval"] or hdr["mcus"]
    return [(k * ri, min(ri, hdr["mcus"] - k * ri)) for k in range(len(hdr["segments"]))]


def _status_error(who, i, status):
    return ValueError("%s: image %d did not decode: %s" % (who, i, ", ".join(t for bit, t in _STATUS_TEXT if status & bit)))


def decode_jpegs_host(datas, counters=None):
    """The whole decoder on the host, in numpy and plain Python integers: a list of JPEG files (bytes) of one size and format
    -> uint8 ``[n,3,h,w]``, or ``[n,h,w]`` for gray files -- what ``decode_jpegs`` gives, and PIL wherever the coefficients
    are ones 8-bit samples give (the module docstring states that domain and what holds outside it).  ``counters``: a dict that
    collects what the decode met (``long_codes``, codes longer than ``LOOK_BITS``; ``zrl``; ``eob``; ``max_dc_category``;
    ``clip_low`` / ``clip_high``, IDCT outputs below 0 / above 255).  ValueError as ``parse_jpeg`` and ``decode_jpegs``."""
    counters = {} if counters is None else counters
    hdrs, (w, h, nc, hs, vs) = parse_batch(datas, "decode_jpegs_host")
    geo = layout(w, h, nc, hs, vs)
    out = []
    for i, hdr in enumerate(hdrs):
        huff, quant = _tables_of(hdr)
        coef = np.zeros((geo["blocks"], 64), dtype=np.int16)
        status = 0
        for seg, (first, count) in zip(hdr["segments"], _segment_mcus(hdr)):
            status |= _decode_segment(seg, first, count, geo, hdr["components"], huff, coef, counters)
        if status:
            raise _status_error("decode_jpegs_host", i, status)
        planes = []
        for c in range(nc):
            b0, bw, bh = geo["block_base"][c], geo["blocks_w"][c], geo["blocks_h"][c]
            planes.append(blocks_to_plane(idct_blocks(coef[b0:b0 + bw * bh], quant[c], counters), bw, bh))
        out.append(planes[0][:h, :w] if nc == 1 else planes_to_rgb(planes, w, h, hs, vs))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ the decoder on the device

def parse_batch(datas, who):
    """Parse every file of one call -> (headers, (w, h, ncomp, hs, vs)); ValueError unless all share the size, the component
    count and the sampling."""
    datas = list(datas)
    if not datas:
        raise ValueError("%s: no images" % who)
    hdrs = [d if isinstance(d, dict) else parse_jpeg(d) for d in datas]  # a header parse_jpeg gave stands for its file

    def shape(hdr):
        c = hdr["components"]
        return hdr["width"], hdr["height"], len(c), c[0]["h"], c[0]["v"]
    for i, hdr in enumerate(hdrs):
        if shape(hdr) != shape(hdrs[0]):
            raise ValueError("%s: image %d is %dx%d with %d components and luma sampling %dx%d, image 0 is %dx%d with %d and "
                             "%dx%d: one call takes one size and format" % ((who, i) + shape(hdr) + shape(hdrs[0])))
    return hdrs, shape(hdrs[0])


def _table_set(hdr):
    """The device form of one file's tables (include/va.h): ``SET_BYTES`` bytes."""
    huff, quant = _tables_of(hdr)
    parts = [np.zeros(192, dtype=np.uint16)]
    for c, q in enumerate(quant):
        parts[0][64 * c:64 * c + 64] = q
    for c in range(3):
        for tab in (huff[c] if c < len(huff) else ((), ())):
            parts.extend(tab)
        if c >= len(huff):
            parts.append(np.zeros(2 * HUFF_BYTES, dtype=np.uint8))
    blob = b"".join(np.ascontiguousarray(p).tobytes() for p in parts)
    assert len(blob) == SET_BYTES
    return blob


def pack_jpegs(hdrs):
    """The one upload of a call (include/va.h, ``va_jpeg_decode``) -> ``(bytes, n_segments, n_sets)``: the image table, the
    segment table, the table sets -- identical ones are kept once -- and the segments' bytes, each from a multiple of 4."""
    sets, set_of, img_rows, seg_rows, chunks, off = [], {}, [], [], [], 0
    for i, hdr in enumerate(hdrs):
        key = tuple((hdr["quant"][c["tq"]].tobytes(), bytes(hdr["huffman"][(0, c["td"])][0]), bytes(hdr["huffman"][(0, c["td"])][1]),
                     bytes(hdr["huffman"][(1, c["ta"])][0]), bytes(hdr["huffman"][(1, c["ta"])][1])) for c in hdr["components"])
        if key not in set_of:  # the tables of a video's frames are built once
            set_of[key] = len(sets)
            sets.append(_table_set(hdr))
        img_rows.append((set_of[key], len(seg_rows), len(hdr["segments"]), 0))
        for seg, (first, count) in zip(hdr["segments"], _segment_mcus(hdr)):
            seg_rows.append((i, off, len(seg), first, count, 0, 0, 0))
            pad = -len(seg) % 4
            chunks.append(seg + b"\x00" * pad)
            off += len(seg) + pad
    head = np.asarray(img_rows, dtype=np.int32).tobytes()
    head += b"\x00" * (-len(head) % 16)
    packed = b"".join([head, np.asarray(seg_rows, dtype=np.int32).tobytes()] + sets + chunks)
    if len(packed) >= 1 << 31:
        raise ValueError("decode_jpegs: %d bytes in one call, the limit is 2**31" % len(packed))
    return packed, len(seg_rows), len(sets)


def upload(packed, device):
    """``pack_jpegs``'s bytes -> a uint8 tensor on ``device``: one pinned staging buffer, one copy on the current stream."""
    import torch
    staging = torch.empty(len(packed), dtype=torch.uint8, pin_memory=True)
    staging.numpy()[:] = np.frombuffer(packed, dtype=np.uint8)
    return staging.to(device, non_blocking=True)


def launch(packed, shape, nseg, nsets, out, status):
    """``va_jpeg_decode`` on the current stream: ``packed`` as ``upload`` gives it, ``shape = (n, w, h, ncomp, hs, vs)``,
    ``out`` and ``status`` the tensors to fill.  The workspace is this call's own, stream-ordered."""
    import torch
    from . import _ffi
    L = _ffi.lib()
    device = packed.device
    nbytes = int(L.va_jpeg_decode_workspace_bytes(*shape))
    work = torch.empty(nbytes, dtype=torch.uint8, device=device)
    _ffi.check(L.va_jpeg_decode(_ffi.ctx(device.index), _ffi.ptr(packed), packed.numel(), *shape, nseg, nsets, _ffi.ptr(out),
                                _ffi.ptr(status), _ffi.ptr(work), nbytes, _ffi.stream_ptr(device)))


def decode_jpegs(datas, device, out=None, check=True):
    """A list of baseline JPEG files (bytes) -> ``(pixels, status)`` on ``device``: pixels uint8 ``[n,3,h,w]`` planar RGB, or
    ``[n,h,w]`` for gray files, PIL's values bit for bit for every file whose blocks hold the quantised DCT
    of 8-bit samples -- any file an encoder wrote; for coefficients outside that, where libjpeg's builds differ among
    themselves, the values of ``decode_jpegs_host`` (the module docstring); status int32 ``[n]``, 0 for every image that
    decoded (the bits: ``STATUS_*``).  All images of one call share the size, the component count and the sampling; their
    tables may differ.  One pinned staging buffer and one upload carry everything; the call is ordered on the current stream.

    ``out``: a contiguous uint8 tensor of the result's shape on ``device`` to write into.  ``check=True`` reads the status (one
    synchronisation) and raises ValueError naming the first image that did not decode; with ``check=False`` nothing waits
    and the status is the caller's to read.  ValueError from ``parse_jpeg`` for every file outside the subset, for mixed
    sizes or formats and for a wrong ``out``, before anything touches the device."""
    import torch
    hdrs, (w, h, nc, hs, vs) = parse_batch(datas, "decode_jpegs")
    n = len(hdrs)
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("decode_jpegs: device must be a CUDA device, got %s" % device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    shape = (n, 3, h, w) if nc == 3 else (n, h, w)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape
                            or not out.is_contiguous() or out.device != device):
        raise ValueError("decode_jpegs: out must be a contiguous uint8 tensor of shape %s on %s" % (shape, device))
    packed, nseg, nsets = pack_jpegs(hdrs)
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=device)
        status = torch.empty(n, dtype=torch.int32, device=device)
        launch(upload(packed, device), (n, w, h, nc, hs, vs), nseg, nsets, out, status)
    if check:
        bad = status.cpu().numpy()
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise _status_error("decode_jpegs", i, int(bad[i]))
    return out, status


def idct_planes(coef, quant, w, h, ncomp, hs, vs):
    """The second launch alone (``va_jpeg_idct``, a testing entry point): coef int16 ``[n, blocks, 64]`` on the device in
    ``layout``'s block order and quant uint16 ``[ncomp, 64]`` -> the planes uint8 ``[n, plane_bytes]``, or ``[n,h,w]`` for
    ``ncomp = 1``."""
    import torch
    from . import _ffi
    geo = layout(w, h, ncomp, hs, vs)
    n = int(coef.shape[0])
    if (coef.dtype != torch.int16 or tuple(coef.shape) != (n, geo["blocks"], 64) or not coef.is_contiguous()
            or quant.dtype != torch.int16 or tuple(quant.shape) != (ncomp, 64) or not quant.is_contiguous()):
        raise ValueError("idct_planes: coef must be int16 [n,%d,64] and quant int16 (the uint16 bits) [%d,64]" % (geo["blocks"], ncomp))
    dst = torch.empty((n, h, w) if ncomp == 1 else (n, geo["plane_bytes"]), dtype=torch.uint8, device=coef.device)
    _ffi.check(_ffi.lib().va_jpeg_idct(_ffi.ctx(coef.device.index), _ffi.ptr(coef), _ffi.ptr(quant), n, w, h, ncomp, hs, vs,
                                       _ffi.ptr(dst), _ffi.stream_ptr(coef.device)))
    return dst


def upsample_planes(planes, w, h, hs, vs):
    """The third launch alone (``va_jpeg_upsample``, a testing entry point): planes uint8 ``[n, plane_bytes]`` on the device
    (Y, Cb, Cr, MCU-padded: ``layout``) -> uint8 ``[n,3,h,w]``."""
    import torch
    from . import _ffi
    geo = layout(w, h, 3, hs, vs)
    n = int(planes.shape[0])
    if planes.dtype != torch.uint8 or tuple(planes.shape) != (n, geo["plane_bytes"]) or not planes.is_contiguous():
        raise ValueError("upsample_planes: planes must be uint8 [n,%d]" % geo["plane_bytes"])
    out = torch.empty((n, 3, h, w), dtype=torch.uint8, device=planes.device)
    _ffi.check(_ffi.lib().va_jpeg_upsample(_ffi.ctx(planes.device.index), _ffi.ptr(planes), n, w, h, hs, vs, _ffi.ptr(out),
                                           _ffi.stream_ptr(planes.device)))
    return out


# ------------------------------------------------------------------------------------------------ the encoder on the host

# Annex K.1 of the JPEG standard in natural order: the tables libjpeg scales by the quality
STD_QUANT = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
     100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99))

ENC_STATUS_RANGE, ENC_STATUS_FIT = 1, 2  # bits of the encoder's per-image status
_ENC_STATUS_TEXT = ((ENC_STATUS_RANGE, "a coefficient outside the baseline categories (DC difference above 11 bits, AC above 10)"),
                    (ENC_STATUS_FIT, "the scan did not fit the output buffer"))
ENC_TABLE_BYTES = 384 + 2 * (16 + 256) * 4  # quant u16[3][64]; then (DC u32[16], AC u32[256]) of luma and of chroma (include/va.h)
BLOCK_BITS = 20 + 63 * 26                   # the most one block codes to: a DC code + value, 63 AC codes + values
_SUBSAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}  # PIL's keyword -> the luma sampling factors


def quant_tables(quality):
    """libjpeg's ``jpeg_set_quality(quality, force_baseline=TRUE)`` -> ``(luma, chroma)``, uint16 [64] in natural order:
    Annex K's tables times ``5000 / q`` percent below 50 and ``200 - 2 q`` from there, each entry ``(base * scale + 50) / 100``
    clamped to 1..255.  ValueError outside 1..100."""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError("quant_tables: quality must be an integer in 1..100, got %r" % (quality,))
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(t, dtype=np.int64) * scale + 50) // 100, 1, 255).astype(np.uint16) for t in STD_QUANT)


def huffman_codes(bits, vals):
    """(bits [16], values) of one DHT table -> uint32 [256] indexed by symbol: ``length << 16 | code``, 0 for a symbol the
    table does not hold."""
    out = np.zeros(256, dtype=np.uint32)
    code = k = 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[k]] = (l << 16) | code
            code, k = code + 1, k + 1
        code <<= 1
    return out


def encode_tables(quant, huffman=STD_HUFFMAN):
    """The encoder's one table block on the device (include/va.h), ``ENC_TABLE_BYTES`` bytes: ``quant`` (luma, chroma) as
    u16 [3][64] per component, then the codes of the (DC, AC) tables of luma and of chroma, ``huffman_codes``'s form."""
    q = np.stack([quant[0], quant[1], quant[1]]).astype(np.uint16)
    parts = [q.tobytes()]
    for th in (0, 1):
        parts.append(huffman_codes(*huffman[(0, th)])[:16].tobytes())
        parts.append(huffman_codes(*huffman[(1, th)]).tobytes())
    blob = b"".join(parts)
    assert len(blob) == ENC_TABLE_BYTES
    return blob


def rgb_to_ycc(rgb):
    """jccolor.c's 16-bit fixed point: uint8 [3, h, w] -> int64 [3, h, w] (Y, Cb, Cr)."""
    r, g, b = (rgb[c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.stack([y, cb, cr])


def _clamp_take(a, rows, cols):
    """``a`` [h, w] extended to ``rows`` x ``cols`` by repeating its last row and column."""
    return a[np.minimum(np.arange(rows), a.shape[0] - 1)][:, np.minimum(np.arange(cols), a.shape[1] - 1)]


def component_plane(full, hs, vs, chroma):
    """One component at full resolution int64 [h, w] -> its samples on the grid of its real blocks, [8 hb, 8 wb]: columns
    repeated at full resolution up to the blocks' width, rows only up to a multiple of ``vs``; then the downsampling
    (h2v1 with bias 0, 1, ..., h2v2 with 1, 2, ... along every output row); then the last downsampled row repeated."""
    h, w = full.shape
    fh, fv = (hs, vs) if chroma else (1, 1)
    wb, hb = -(-w // (8 * fh)), -(-h // (8 * fv))
    a = _clamp_take(full, -(-h // fv) * fv, wb * 8 * fh)
    if fh == 2:
        x = np.arange(wb * 8)
        if fv == 2:
            a = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 1 + (x & 1)) >> 2
        else:
            a = (a[:, 0::2] + a[:, 1::2] + (x & 1)) >> 1
    return _clamp_take(a, hb * 8, a.shape[1])


def _fdct_pass(d, first):
    """One 8-point pass of jfdctint's "islow" forward DCT along the last axis of an int64 array."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 11 if first else 15

    def ds(x, n):
        return (x + (1 << (n - 1))) >> n
    o = [None] * 8
    o[0], o[4] = ((t10 + t11) << 2, (t10 - t11) << 2) if first else (ds(t10 + t11, 2), ds(t10 - t11, 2))
    z1 = (t12 + t13) * 4433
    o[2], o[6] = ds(z1 + t13 * 6270, sh), ds(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = ds(t4 + z1 + z3, sh), ds(t5 + z2 + z4, sh), ds(t6 + z2 + z3, sh), ds(t7 + z1 + z4, sh)
    return np.stack(o, axis=-1)


def fdct_blocks(px, quant):
    """Samples [..., 8, 8] -> the quantised coefficients int64 [..., 64] in natural order: ``jfdct_islow`` on samples - 128
    (rows, then columns; the output is scaled by 8), divided by ``8 q`` rounding half away from zero."""
    d = _fdct_pass(np.asarray(px).astype(np.int64) - 128, True)
    d = np.swapaxes(_fdct_pass(np.swapaxes(d, -1, -2), False), -1, -2)
    c = d.reshape(d.shape[:-2] + (64,))
    q = np.asarray(quant).astype(np.int64)
    return np.sign(c) * ((np.abs(c) + 4 * q) // (8 * q))


def _scan_order(geo, hs, vs, ncomp, m):
    """(component, block index within ``layout``'s array) of the blocks of MCU ``m``, in the order they are coded."""
    my, mx = divmod(m, geo["mcu_w"])
    if ncomp == 1:
        return [(0, m)]
    out = [(0, (my * vs + v) * geo["blocks_w"][0] + mx * hs + u) for v in range(vs) for u in range(hs)]
    return out + [(c, geo["block_base"][c] + m) for c in (1, 2)]


def encode_coefficients(img, quant, hs, vs, counters=None):
    """One image uint8 [h, w] or [3, h, w] -> int16 [blocks, 64] in ``layout``'s order, the quantised coefficients libjpeg
    codes: colour conversion, edge padding, downsampling, forward DCT, quantisation; a dummy block (on the MCU-padded grid
    but outside the component's real blocks) holds zero AC and the DC of the block before it in the MCU's own order."""
    nc = 1 if img.ndim == 2 else 3
    h, w = img.shape[-2:]
    geo = layout(w, h, nc, hs, vs)
    comps = [img.astype(np.int64)] if nc == 1 else list(rgb_to_ycc(img))
    coef = np.zeros((geo["blocks"], 64), dtype=np.int64)
    for c, full in enumerate(comps):
        p = component_plane(full, hs, vs, c > 0)
        hb, wb = p.shape[0] // 8, p.shape[1] // 8
        blk = fdct_blocks(p.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3), quant[min(c, 1)])
        grid = coef[geo["block_base"][c]:geo["block_base"][c] + geo["blocks_w"][c] * geo["blocks_h"][c]]
        grid.reshape(geo["blocks_h"][c], geo["blocks_w"][c], 64)[:hb, :wb] = blk
        if c == 0 and (wb < geo["blocks_w"][0] or hb < geo["blocks_h"][0]):
            for m in range(geo["mcu_w"] * geo["mcu_h"]):
                order = _scan_order(geo, hs, vs, nc, m)[:hs * vs]
                for k, (_, at) in enumerate(order):
                    by, bx = divmod(at, geo["blocks_w"][0])
                    if bx >= wb or by >= hb:
                        coef[at] = 0
                        coef[at, 0] = coef[order[k - 1][1], 0]
                        if counters is not None:
                            counters["dummy_blocks"] = counters.get("dummy_blocks", 0) + 1
    return coef.astype(np.int16)


def _category(v):
    return int(abs(int(v))).bit_length()


def entropy_encode_host(coef, w, h, ncomp, hs, vs, restart=0, huffman=STD_HUFFMAN, counters=None):
    """int16 [blocks, 64] (``layout``'s order) -> the scan's bytes: Huffman coding in MCU order with the DC predictors reset at
    every restart interval, every interval filled up to a whole byte with 1-bits, FF stuffed to FF 00, ``RSTm`` between
    intervals.  ValueError for a coefficient outside the baseline categories."""
    counters = {} if counters is None else counters
    geo = layout(w, h, ncomp, hs, vs)
    codes = {key: huffman_codes(*spec) for key, spec in huffman.items()}
    mcus = geo["mcu_w"] * geo["mcu_h"]
    interval = restart or mcus
    out = bytearray()
    for first in range(0, mcus, interval):
        acc = nbits = 0
        pred = [0, 0, 0]

        def put(cls, th, sym, value, size):
            nonlocal acc, nbits
            e = int(codes[(cls, th)][sym])
            if e == 0:
                raise ValueError("encode_jpegs_host: " + _ENC_STATUS_TEXT[0][1])
            v = value if value >= 0 else value + (1 << size) - 1
            acc = (((acc << (e >> 16)) | (e & 0xFFFF)) << size) | v
            nbits += (e >> 16) + size
        for m in range(first, min(first + interval, mcus)):
            for c, at in _scan_order(geo, hs, vs, ncomp, m):
                th = min(c, 1)
                zz = [int(v) for v in coef[at][ZIGZAG]]
                diff = zz[0] - pred[c]
                pred[c] = zz[0]
                s = _category(diff)
                if s > 11:
                    raise ValueError("encode_jpegs_host: " + _ENC_STATUS_TEXT[0][1])
                counters["max_dc_category"] = max(counters.get("max_dc_category", 0), s)
                put(0, th, s, diff, s)
                run = 0
                for k in range(1, 64):
                    if zz[k] == 0:
                        run += 1
                        continue
                    while run > 15:
                        put(1, th, 0xF0, 0, 0)
                        counters["zrl"] = counters.get("zrl", 0) + 1
                        run -= 16
                    s = _category(zz[k])
                    if s > 10:
                        raise ValueError("encode_jpegs_host: " + _ENC_STATUS_TEXT[0][1])
                    counters["max_ac_category"] = max(counters.get("max_ac_category", 0), s)
                    put(1, th, run << 4 | s, zz[k], s)
                    run = 0
                if run:
                    put(1, th, 0, 0, 0)
                    counters["eob"] = counters.get("eob", 0) + 1
                    if run == 63 and diff == 0:
                        counters["zero_blocks"] = counters.get("zero_blocks", 0) + 1
                else:
                    counters["no_eob"] = counters.get("no_eob", 0) + 1
        pad = -nbits % 8
        plain = (((acc << pad) | ((1 << pad) - 1)).to_bytes((nbits + pad) // 8, "big"))
        counters["segments"] = counters.get("segments", 0) + 1
        counters.setdefault("padding", []).append(pad)
        counters["stuffed"] = counters.get("stuffed", 0) + plain.count(b"\xff")
        if first:
            out += bytes([0xFF, 0xD0 + (first // interval - 1) % 8])
        out += plain.replace(b"\xff", b"\xff\x00")
    return bytes(out)


def jpeg_header(w, h, ncomp, hs, vs, quant, restart=0, huffman=STD_HUFFMAN):
    """Everything PIL writes in front of the scan: SOI, APP0 "JFIF" 1.01 (units 0, density 1x1, no thumbnail), one DQT per
    table, SOF0, one DHT per table in the order DC0, AC0, DC1, AC1, DRI when ``restart`` is not 0, SOS."""
    def seg(m, payload):
        return bytes([0xFF, m]) + struct.pack(">H", len(payload) + 2) + payload
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(1 if ncomp == 1 else 2):
        out += seg(0xDB, bytes([t]) + bytes(int(v) for v in np.asarray(quant[t])[ZIGZAG]))
    sof = struct.pack(">BHHB", 8, h, w, ncomp)
    for c in range(ncomp):
        sof += bytes([c + 1, (hs << 4 | vs) if c == 0 and ncomp == 3 else 0x11, min(c, 1)])
    out += seg(0xC0, sof)
    for th in range(1 if ncomp == 1 else 2):
        for cls in (0, 1):
            bits, vals = huffman[(cls, th)]
            out += seg(0xC4, bytes([cls << 4 | th]) + bytes(bits) + bytes(vals))
    if restart:
        out += seg(0xDD, struct.pack(">H", restart))
    sos = bytes([ncomp]) + b"".join(bytes([c + 1, min(c, 1) * 0x11]) for c in range(ncomp)) + b"\x00\x3f\x00"
    return out + seg(0xDA, sos)


def _encode_args(who, shape, quality, subsampling, restart_blocks):
    """The checks every encoder shares -> ``(n, w, h, ncomp, hs, vs, restart, quant)``; ValueError for a rank other than 3 or
    4, a size below 3x3 or above 65535, a bad quality or subsampling and a restart interval outside 0..65535."""
    if len(shape) not in (3, 4) or (len(shape) == 4 and shape[1] != 3) or shape[0] < 1:
        raise ValueError("%s: images must be [n,h,w] (gray) or [n,3,h,w] (RGB) with n >= 1, got %s" % (who, list(shape)))
    h, w = int(shape[-2]), int(shape[-1])
    if not (3 <= w <= 65535 and 3 <= h <= 65535):
        raise ValueError("%s: %dx%d is outside the sizes 3x3 .. 65535x65535" % (who, w, h))
    quant = quant_tables(quality)
    ncomp = 1 if len(shape) == 3 else 3
    if isinstance(subsampling, bool) or subsampling not in _SUBSAMPLING:
        raise ValueError("%s: subsampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), got %r" % (who, subsampling))
    hs, vs = _SUBSAMPLING[subsampling] if ncomp == 3 else (1, 1)
    restart = 0 if restart_blocks is None else restart_blocks
    if isinstance(restart, bool) or not isinstance(restart, (int, np.integer)) or not 0 <= restart <= 65535:
        raise ValueError("%s: restart_blocks must be an integer of at most 65535 MCUs per interval, got %r" % (who, restart_blocks))
    geo = layout(w, h, ncomp, hs, vs)
    if geo["plane_bytes"] > MAX_SAMPLES:
        raise ValueError("%s: %dx%d holds %d samples in its MCUs, more than the %d one image may have"
                         % (who, w, h, geo["plane_bytes"], MAX_SAMPLES))
    return int(shape[0]), w, h, ncomp, hs, vs, int(restart), quant


def encode_jpegs_host(images, quality=95, subsampling=2, restart_blocks=None, counters=None):
    """The whole encoder on the host, in numpy and plain Python integers: uint8 ``[n,h,w]`` (gray) or ``[n,3,h,w]`` (planar
    RGB) -> a list of n files (bytes), byte for byte what ``Image.fromarray(...).save(f, "JPEG", quality=, subsampling=,
    restart_marker_blocks=)`` writes and what ``encode_jpegs`` gives.  ``counters``: a dict that collects what the encode met:
    ``stuffed`` (FF bytes), ``zrl``, ``eob``, ``no_eob`` (blocks whose coefficient 63 is not zero), ``zero_blocks`` (blocks of
    a DC difference of 0 and no AC), ``max_dc_category``, ``max_ac_category``, ``segments`` (restart intervals),
    ``dummy_blocks`` and ``padding``, the fill bits of every interval.  ValueError as ``encode_jpegs``."""
    images = np.asarray(images)
    if images.dtype != np.uint8:
        raise ValueError("encode_jpegs_host: images must be uint8, got %s" % images.dtype)
    n, w, h, nc, hs, vs, restart, quant = _encode_args("encode_jpegs_host", images.shape, quality, subsampling, restart_blocks)
    head = jpeg_header(w, h, nc, hs, vs, quant, restart)
    return [head + entropy_encode_host(encode_coefficients(images[i], quant, hs, vs, counters), w, h, nc, hs, vs, restart,
                                       counters=counters) + b"\xff\xd9" for i in range(n)]


# ------------------------------------------------------------------------------------------------ the encoder on the device

def scan_bound(w, h, ncomp, hs, vs, restart=0):
    """The most bytes the scan of one image takes (include/va.h): every block at ``BLOCK_BITS``, one byte of fill per
    interval, all of it stuffed, and two bytes of ``RSTm`` between intervals."""
    geo = layout(w, h, ncomp, hs, vs)
    mcus = geo["mcu_w"] * geo["mcu_h"]
    intervals = -(-mcus // restart) if restart else 1
    return 2 * (-(-geo["blocks"] * BLOCK_BITS // 8) + intervals) + 2 * (intervals - 1)


def _enc_status_error(who, i, status):
    return ValueError("%s: image %d did not encode: %s" % (who, i, ", ".join(t for bit, t in _ENC_STATUS_TEXT if status & bit)))


def _enc_workspace(shape, restart, device):
    import torch
    from . import _ffi
    nbytes = int(_ffi.lib().va_jpeg_encode_workspace_bytes(*shape, restart))
    if nbytes == 0:
        raise ValueError("encode_jpegs: %d images of %dx%d are more than one call encodes" % shape[:3])
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _scans(out, lengths, status, who, check):
    """One synchronisation for the lengths (and the status), one download of the bytes in use -> a list of scans."""
    ls = lengths.cpu().numpy().astype(np.int64)
    bad = status.cpu().numpy()
    if check and bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise _enc_status_error(who, i, int(bad[i]))
    ends = np.cumsum(ls)
    data = out[:int(ends[-1])].cpu().numpy().tobytes()
    return [b"" if bad[i] & ENC_STATUS_FIT else data[int(e - l):int(e)] for i, (l, e) in enumerate(zip(ls, ends))]


def encode_buffers(shape, restart, device):
    """What one ``va_jpeg_encode`` call of ``shape = (n, w, h, ncomp, hs, vs)`` fills -> ``(out, lengths, status, work)``:
    the output sized by ``scan_bound``, so that nothing is ever cut short, and the call's own workspace."""
    import torch
    n = shape[0]
    work, _ = _enc_workspace(shape, restart, device)
    return (torch.empty(n * scan_bound(*shape[1:], restart), dtype=torch.uint8, device=device),
            torch.empty(n, dtype=torch.int32, device=device), torch.empty(n, dtype=torch.int32, device=device), work)


def encode_launch(images, shape, restart, tables, out, lengths, status, work):
    """``va_jpeg_encode`` on the current stream: two memsets and four launches, nothing waits."""
    from . import _ffi
    device = images.device
    _ffi.check(_ffi.lib().va_jpeg_encode(_ffi.ctx(device.index), _ffi.ptr(images), *shape, restart, _ffi.ptr(tables), _ffi.ptr(out),
                                         out.numel(), _ffi.ptr(lengths), _ffi.ptr(status), _ffi.ptr(work), work.numel(),
                                         _ffi.stream_ptr(device)))


def encode_jpegs(images, quality=95, subsampling=2, restart_blocks=None, check=True):
    """A contiguous CUDA uint8 tensor ``[n,h,w]`` (gray) or ``[n,3,h,w]`` (planar RGB), the shapes ``decode_jpegs`` returns ->
    a list of n baseline JPEG files (bytes), byte for byte what ``Image.fromarray(...).save(f, "JPEG", quality=,
    subsampling=, restart_marker_blocks=)`` writes.  ``subsampling``: PIL's 0 / 1 / 2 for 4:4:4, 4:2:2,
    4:2:0, ignored for gray (a gray file is the one PIL writes without the keyword); ``restart_blocks``: PIL's
    ``restart_marker_blocks``, the restart interval in MCUs (None or 0: none).  Standard Huffman tables, no ``optimize``, no progressive files, no custom tables, density or comments.

    The tables go up in one block, the kernels run on the current stream into a buffer sized by the bound of the shape (nothing
    is ever cut short), one synchronisation reads the lengths and one download brings every scan; the host writes the headers
    around them.  ``check=True`` raises ValueError naming the first image whose status is not 0 (``ENC_STATUS_*``: pixels
    give no such image); with ``check=False`` such an image comes back as it is.  ValueError before anything touches the
    device for a tensor that is not a contiguous CUDA uint8 one of those shapes, a size below 3x3 or above 65535, a bad
    quality or subsampling and more than 65535 MCUs per interval."""
    import torch
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8:
        raise ValueError("encode_jpegs: images must be a uint8 tensor, got %s"
                         % (images.dtype if isinstance(images, torch.Tensor) else type(images).__name__))
    n, w, h, nc, hs, vs, restart, quant = _encode_args("encode_jpegs", tuple(images.shape), quality, subsampling, restart_blocks)
    if images.device.type != "cuda" or not images.is_contiguous():
        raise ValueError("encode_jpegs: images must be contiguous and on a CUDA device, got %s on %s"
                         % ("a contiguous tensor" if images.is_contiguous() else "a strided view", images.device))
    device, shape = images.device, (n, w, h, nc, hs, vs)
    with torch.cuda.device(device):
        bufs = encode_buffers(shape, restart, device)
        encode_launch(images, shape, restart, upload(encode_tables(quant), device), *bufs)
        scans = _scans(*bufs[:3], "encode_jpegs", check)
    head = jpeg_header(w, h, nc, hs, vs, quant, restart)
    return [head + s + b"\xff\xd9" for s in scans]


def fdct_coefficients(images, quant, hs=1, vs=1):
    """The first launch alone (``va_jpeg_fdct``, a testing entry point): images as ``encode_jpegs`` takes them and ``quant``
    (luma, chroma) -> coef int16 ``[n, blocks, 64]`` on the device in ``layout``'s order, dummy blocks included."""
    import torch
    from . import _ffi
    n, w, h, nc, hs, vs, _, _ = _encode_args("fdct_coefficients", tuple(images.shape), 50, {(1, 1): 0, (2, 1): 1, (2, 2): 2}.get((hs, vs)), None)
    if images.dtype != torch.uint8 or not images.is_contiguous() or images.device.type != "cuda":
        raise ValueError("fdct_coefficients: images must be a contiguous CUDA uint8 tensor")
    device = images.device
    with torch.cuda.device(device):
        tables = upload(encode_tables(quant), device)
        coef = torch.empty((n, layout(w, h, nc, hs, vs)["blocks"], 64), dtype=torch.int16, device=device)
        _ffi.check(_ffi.lib().va_jpeg_fdct(_ffi.ctx(device.index), _ffi.ptr(images), _ffi.ptr(tables), n, w, h, nc, hs, vs,
                                           _ffi.ptr(coef), _ffi.stream_ptr(device)))
    return coef


def entropy_encode(coef, w, h, ncomp, hs, vs, restart=0, huffman=STD_HUFFMAN, check=True, out_bytes=None):
    """The entropy stage alone (``va_jpeg_entropy_encode``, a testing entry point): coef int16 ``[n, blocks, 64]`` on the
    device in ``layout``'s order, whatever it holds -> ``(scans, status)``, the list of n scans (bytes; empty for an image
    that did not fit) and the status as a numpy array.  ``out_bytes``: the size of the output buffer, by default n times
    ``scan_bound``."""
    import torch
    from . import _ffi
    geo = layout(w, h, ncomp, hs, vs)
    n = int(coef.shape[0])
    if coef.dtype != torch.int16 or tuple(coef.shape) != (n, geo["blocks"], 64) or not coef.is_contiguous() or n < 1:
        raise ValueError("entropy_encode: coef must be int16 [n,%d,64]" % geo["blocks"])
    device, shape = coef.device, (n, w, h, ncomp, hs, vs)
    dummy = (np.ones(64, dtype=np.uint16),) * 2
    with torch.cuda.device(device):
        work, nbytes = _enc_workspace(shape, restart, device)
        tables = upload(encode_tables(dummy, huffman), device)
        out = torch.empty(n * scan_bound(w, h, ncomp, hs, vs, restart) if out_bytes is None else int(out_bytes), dtype=torch.uint8, device=device)
        lengths = torch.empty(n, dtype=torch.int32, device=device)
        status = torch.empty(n, dtype=torch.int32, device=device)
        _ffi.check(_ffi.lib().va_jpeg_entropy_encode(_ffi.ctx(device.index), _ffi.ptr(coef), _ffi.ptr(tables), *shape, restart,
                                                     _ffi.ptr(out), out.numel(), _ffi.ptr(lengths), _ffi.ptr(status), _ffi.ptr(work),
                                                     nbytes, _ffi.stream_ptr(device)))
        scans = _scans(out, lengths, status, "entropy_encode", check)
    return scans, status.cpu().numpy()
