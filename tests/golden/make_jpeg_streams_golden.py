"""Builds tests/golden/jpeg_streams.npz: baseline JPEG files written bit by bit with tests/jpeg_writer.py, and the pixels PIL
(libjpeg) decodes from them -- the judge of DESIGN.md S45-S48 on streams its own encoder never writes.

    python tests/golden/make_jpeg_streams_golden.py

Per case ``NAME`` the file holds ``jpg_NAME``, the file's bytes as uint8, and ``px_NAME``, PIL's pixels: uint8 ``[3,h,w]`` or
``[h,w]``.  ``cases()`` builds every case and asserts, from the writer's ``stats`` alone, that it reaches what it is for (each
builder's docstring says what); the names carry height x width like those of jpeg_small.npz.  ``basis_*`` are the only files
PIL encodes: the 64 DCT basis sign patterns, the largest coefficients 8-bit pixels give.  ``status_streams()`` builds the
files that must NOT decode, with the one status bit each sets by construction; PIL is no judge of those and they are not
recorded.  Nothing of the package is imported here.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_writer as W  # noqa: E402

OUT = os.path.join(HERE, "jpeg_streams.npz")
ONES = np.ones(64, dtype=np.int64)
ALL32 = set(range(32))

# category c in c + 1 bits: '0' is category 0, so the zero bits behind a segment's end decode as "no difference"
DC_ALL = W.huffman_from_lengths(range(12), range(1, 13))
# '0' is EOB; the all-ones code of 16 bits (and every code that starts with six ones) is in no table
AC_SMALL = W.huffman_from_lengths([0x00, 0x01, 0x08, 0xF0, 0xC8, 0xF1], [1, 2, 3, 4, 5, 6])


def pil_pixels(data):
    """PIL's decode: u8 [3,h,w] or [h,w]."""
    im = Image.open(io.BytesIO(data))
    a = np.asarray(im.convert("L" if im.mode == "L" else "RGB"))
    return np.ascontiguousarray(a if a.ndim == 2 else a.transpose(2, 0, 1))


def zz_block(dc, ac=None):
    """DC and {zigzag index: value} -> 64 coefficients in natural order."""
    c = np.zeros(64, dtype=np.int64)
    c[0] = dc
    for k, v in (ac or {}).items():
        assert 1 <= k <= 63 and c[W.ZIGZAG[k]] == 0
        c[W.ZIGZAG[k]] = v
    return c


def _dct_matrix():
    k, x = np.mgrid[:8, :8]
    m = np.cos((2 * x + 1) * k * np.pi / 16) / 2
    m[0] /= np.sqrt(2)
    return m


DCT = _dct_matrix()


def quantised(plane, q):
    """A plane u8 [8 bh, 8 bw] -> its blocks' quantised DCT [bh * bw, 64], natural order: coefficients that 8-bit samples
    give, which is the domain of the bit-for-bit claim."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).astype(np.float64) - 128
    c = np.einsum("ux,nmxy,vy->nmuv", DCT, b, DCT).reshape(bh * bw, 64)
    return np.rint(c / np.asarray(q).reshape(1, 64)).astype(np.int64)


def textured(h, w, seed):
    """u8 [h,w]: 8x8 blocks of alternating dark and bright means (large DC differences, so that a predictor that is not
    reset at a restart shows in the next block) under a ramp and noise."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w]
    mean = np.where(((yy // 8) * 3 + (xx // 8)) % 2 == 0, 40, 215) + rs.randint(-30, 31, size=(h // 8 + 1, w // 8 + 1))[yy // 8, xx // 8]
    return np.clip(mean + (xx % 8) * 3 - (yy % 8) * 2 + rs.randint(-15, 16, size=(h, w)), 0, 255).astype(np.uint8)


def steps(seed, lo=6, hi=30):
    return np.random.RandomState(seed).randint(lo, hi + 1, size=64)


def table_set(seed):
    """A DC and an AC spec of their own shape: every category / every (run, size) up to size 10, lengths shuffled by
    ``seed``, codes of 2..16 bits."""
    rs = np.random.RandomState(seed)
    dc_sym = list(rs.permutation(12))
    dc = W.huffman_from_lengths(dc_sym, [2, 3, 3, 3, 4, 4, 5, 6, 7, 8, 9, 10])
    ac_sym = [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x12, 0x21, 0xF0] + [int(s) for s in rs.permutation(
        [r << 4 | s for r in range(16) for s in range(1, 11) if (r << 4 | s) not in (0x01, 0x02, 0x03, 0x11, 0x04, 0x12, 0x21)])]
    lengths = [2, 3, 3, 4, 4, 5, 5, 6, 6] + [7] * 8 + [8] * 12 + [9] * 16 + [10] * 20 + [11] * 24 + [12] * 20 + [14] * 20 + [16] * 33
    assert len(lengths) == len(ac_sym) == 162
    return dc, W.huffman_from_lengths(ac_sym, lengths)


def _all_ends(stats, key, lengths):
    """Every one of ``lengths`` had its first and its last code emitted from table ``key``."""
    return all(stats["first_last"][key].get(l) == [True, True] for l in lengths)


# ------------------------------------------------------------------------------------------------------ the cases

def case_lengths():
    """Gray 24x32, twelve blocks (one DC code a block): a DC table with one code of each length 1..12 and an AC table with
    one of each length 1..16; every code is emitted."""
    ac = W.huffman_from_lengths([0x00, 0x01, 0x02, 0x11, 0x03, 0x21, 0x04, 0x12, 0x31, 0xF0, 0x05, 0x41, 0x06, 0x51, 0x07, 0x0A],
                                range(1, 17))
    levels = [0, 1, -2, 5, -10, 21, -42, 85, -170, 341, -682, 1016]  # differences of category 0, 1, ..., 11
    acs = [{1: 1, 2: 2, 4: 1}, {1: 5, 4: -1, 5: 9, 7: 3, 11: 1}, {1: -20, 6: 1, 7: 40, 13: -1, 14: 100, 15: -600, 32: 1}]
    blocks = [zz_block(d, acs[i] if i < 3 else {3: (-1) ** i}) for i, d in enumerate(levels)]
    q = ONES * 8  # the small values show in the pixels; the large ones and the DC keep the step 1
    q[[W.ZIGZAG[k] for k in (0, 7, 14, 15)]] = 1
    data, st = W.write_jpeg(32, 24, [blocks], {0: q}, {0: DC_ALL}, {0: ac})
    assert st["codes"][("dc", 0)][1:13] == [1] * 12 and all(n >= 1 for n in st["codes"][("ac", 0)][1:])
    assert _all_ends(st, ("dc", 0), range(1, 13)) and _all_ends(st, ("ac", 0), range(1, 17))
    return {"lengths_gray_24x32": (data, st)}


def _pack(symbols):
    """Blocks (coefficients) that emit every one of ``symbols`` (run << 4 | size) once, in order, as many a block as fit."""
    blocks, ac, i = [], {}, 1
    for n, sym in enumerate(symbols):
        r, s = sym >> 4, sym & 15
        if i + r > 63:
            blocks.append(ac)
            ac, i = {}, 1
        ac[i + r] = (-1) ** n * ((1 << s) - 1 if n % 3 else 1 << (s - 1))
        i += r + 1
    return blocks + [ac]


def case_full_lengths():
    """Gray 16x16: an AC table with codes of 1, 2 and 9 bits, none of 3..8, and three of every length 10..16; the first and
    the last code of every populated length is emitted.  The last code of a length IS that length's maxcode, and the lengths
    without codes are the ones the host fills in."""
    sym = [0x00, 0x01, 0x11, 0x21] + [r << 4 | s for s in (2, 3, 4) for r in range(7)]
    lengths = [1, 2, 9, 9] + [l for l in range(10, 17) for _ in range(3)]
    ac = W.huffman_from_lengths(sym, lengths)
    assert ac[0][2:8] == [0] * 6 and ac[0][9:] == [3] * 7
    order = [s for s in ac[1] if s != 0]
    acs = _pack(order + order[::-1])  # twice, the second time with the other value of each size
    assert len(acs) <= 4
    blocks = [zz_block(60 * (-1) ** i, acs[i] if i < len(acs) else {}) for i in range(4)]
    data, st = W.write_jpeg(16, 16, [blocks], {0: ONES * 8}, {0: DC_ALL}, {0: ac})
    assert _all_ends(st, ("ac", 0), [1, 2, 9] + list(range(10, 17))) and sorted(st["first_last"][("ac", 0)]) == [1, 2, 9] + list(range(10, 17))
    assert all(st["codes"][("ac", 0)][l] >= 6 for l in range(10, 17)) and st["symbols"][("ac", 0)] == set(sym)
    return {"full_gray_16x16": (data, st)}


def case_ac256():
    """Gray 8x16: an AC table of all 256 symbols, eight codes of 1..8 bits and 248 of 16: valoff[16] is negative and the
    index into vals is taken modulo 256; vals[0], vals[8] (the first 16-bit code) and vals[255] (the last) are emitted."""
    head = [0x00, 0x01, 0x02, 0x11, 0x03, 0x21, 0x12, 0x31]
    rest = [s for s in range(256) if s not in head and s not in (0x04, 0x22)]
    vals = head + [0x04] + rest + [0x22]
    ac = W.huffman_from_lengths(vals, [1, 2, 3, 4, 5, 6, 7, 8] + [16] * 248)
    assert ac[1] == vals and ac[0][15] == 248 and W.code_table(ac)[0x04][0] > 8  # first 16-bit code > its index: valoff < 0
    blocks = [zz_block(-30, {1: 9, 2: 1, 4: 2, 5: -3}), zz_block(25, {1: -15, 3: -2, 4: 1})]  # 0x04, 0x01, 0x12, 0x02 | 0x04, 0x12, 0x01
    blocks[0][W.ZIGZAG[9]] = 3                                                               # run 3: 0x32 is a 16-bit code too
    blocks[1][W.ZIGZAG[7]] = -2                                                              # run 2, size 2: 0x22, vals[255]
    data, st = W.write_jpeg(16, 8, [blocks], {0: ONES * 8}, {0: DC_ALL}, {0: ac})
    assert {vals[0], vals[8], vals[255]} <= st["symbols"][("ac", 0)] and st["first_last"][("ac", 0)][16] == [True, True]
    return {"ac256_gray_8x16": (data, st)}


def _shift(d):
    """(a, b), the fewest symbols 0x01 (3 bits with their value) and 0x02 (5 bits) that move the bit position by d mod 32."""
    return min(((a, b) for a in range(12) for b in range(12) if (3 * a + 5 * b) % 32 == d % 32), key=sum)


def case_phases():
    """Gray 32x64, 32 blocks.  Every block starts with a 16-bit DC code and its 11-bit value, then holds the 16-bit AC code
    of symbol 0x0A with its 10-bit value and the 10-bit code of symbol 0x09; short symbols in between place the DC code at
    bit offset b mod 32 and the AC code at 5 b + 3 mod 32 in block b, so each of the three begins at all 32 offsets, and the
    16-bit codes cross a word boundary with their value at every offset that can (7..31 / 6..31: all eight byte phases)."""
    dc = W.huffman_from_lengths([0, 1, 2, 11], [1, 2, 3, 16])
    ac = W.huffman_from_lengths([0x00, 0x01, 0x02, 0x09, 0x0A], [1, 2, 3, 10, 16])
    blocks, pos, pred = [], 0, 0
    for b in range(32):
        level = -1024 if b % 2 == 0 else 1016
        items, i = [(11, level - pred)], 1
        pred = level
        pos += 27
        tail = lambda a, c: [(0x01, (-1) ** (b + j)) for j in range(a)] + [(0x02, 2 + (j + b) % 2) for j in range(c)]  # noqa: E731
        a, c = _shift(5 * b + 3 - pos)
        items += tail(a, c) + [(0x0A, (-1) ** b * (1023 - 7 * b)), (0x09, (-1) ** (b // 2) * (511 - 5 * b))]
        pos += 3 * a + 5 * c + 26 + 19
        a, c = _shift(b + 1 - pos - 1)  # then EOB, one bit, and the next block's DC code
        items += tail(a, c) + [(W.EOB, 0)]
        pos += 3 * a + 5 * c + 1
        blocks.append(items)
    data, st = W.write_jpeg(64, 32, [blocks], {0: ONES}, {0: dc}, {0: ac})
    by = st["long_code_offsets_by_length"]
    assert st["long_code_offsets"] == ALL32 and by[16] == ALL32 and by[10] == ALL32, st
    assert st["crossings"] == set(range(6, 32)) and {o % 8 for o in st["crossings"]} == set(range(8))
    assert st["codes"][("dc", 0)][16] == 32 and st["codes"][("ac", 0)][16] == 32
    return {"phases_gray_32x64": (data, st)}


def _tail_blocks(ends_ff, n, k):
    """One block of 2 + 3 n bits (category 0, n times symbol 0x01, EOB), or one that ends in eight 1-bits on a byte boundary:
    two 0x01, three ZRL, then run 12 to coefficient 63 with the 8-bit value 255 and no EOB."""
    if ends_ff:
        return [(0, 0), (0x01, 1), (0x01, -1), (W.ZRL, 0), (W.ZRL, 0), (W.ZRL, 0), (0xC8, 255)]
    return [(0, 0)] + [(0x01, (-1) ** (j + k)) for j in range(n)] + [(W.EOB, 0)]


def case_tails():
    """Gray 8x64 with a restart marker per MCU: segments of 1, 3, 2, 4, 4, 4, 1 and 4 bytes (every length modulo 4), with 0
    and with 7 padding bits, three that end in a stuffed FF 00 -- one in front of its marker, one with a fill FF in between,
    one in front of two fill bytes and EOI -- and one of 2 bytes with two fill bytes behind it."""
    plan = [(False, 2), (False, 5), (False, 3), (False, 10), (True, 0), (True, 0), (False, 0), (True, 0)]
    blocks = [_tail_blocks(ff, n, k) for k, (ff, n) in enumerate(plan)]
    q = ONES * 16
    q[63] = 1  # the 8-bit value 255 sits at coefficient 63
    data, st = W.write_jpeg(64, 8, [blocks], {0: q}, {0: DC_ALL}, {0: AC_SMALL}, restart=1, rst_fill={2: 2, 4: 1}, eoi_fill=2)
    seg = st["segments"]
    assert [s["bytes"] for s in seg] == [1, 3, 2, 4, 4, 4, 1, 4] and {s["bytes"] % 4 for s in seg} == {0, 1, 2, 3}
    assert {0, 7} <= {s["padding"] for s in seg} and seg[0]["padding"] == 0 and seg[1]["padding"] == 7
    assert [s["ends_stuffed"] for s in seg] == [False] * 4 + [True, True, False, True] and st["stuffed"] == 3
    assert [s["fill"] for s in seg] == [0, 0, 2, 0, 1, 0, 0, 0] and b"\xff\x00\xff\xff\xd4" in data and b"\xff\x00\xff\xd5" in data
    assert data.endswith(b"\xff\x00\xff\xff\xff\xd9") and st["end63"] == 3
    return {"tails_gray_8x64": (data, st)}


def case_marker_wrap():
    """Gray 16x40 with a restart marker per MCU: ten segments, so the markers run RST0..RST7 and start again at RST0."""
    blocks = [_tail_blocks(k % 4 == 3, 1 + k, k) for k in range(10)]
    q = ONES * 16
    q[63] = 1
    data, st = W.write_jpeg(40, 16, [blocks], {0: q}, {0: DC_ALL}, {0: AC_SMALL}, restart=1)
    assert len(st["segments"]) == 10 and data.count(b"\xff\xd0") == 2 and data.count(b"\xff\xd7") == 1 and b"\xff\xd1" in data
    return {"wrap_gray_16x40": (data, st)}


def case_magnitudes():
    """Gray 48x64, 48 blocks, quantiser 1.  AC: every size 1..10 at +-(2^s - 1) and +-2^(s-1), one such coefficient a block, at
    a position that moves through the block.  DC: differences of every category 0..11 at both signs of 2^s - 1 and 2^(s-1);
    for category 11 they are +-1024 and +-2040, the walk from one end of the levels 8-bit samples give (-1024..1016) to the
    other and back.  One large coefficient in a block stays where every libjpeg build agrees."""
    ac_sym = [0x00, 0xF0] + [r << 4 | s for s in range(1, 11) for r in range(16)]
    ac = W.huffman_from_lengths(ac_sym, [3, 8] + [4 + (s + 1) // 2 + (r > 0) * 3 + (r > 7) * 3 for s in range(1, 11) for r in range(16)])
    diffs = [0]
    for s in range(1, 11):
        diffs += [-((1 << s) - 1), (1 << s) - 1, -(1 << (s - 1)), 1 << (s - 1)]  # down first: 1023 is past the brightest level
    diffs += [-1024, 2040, -2040, 1024, 0, 0, 0]
    assert len(diffs) == 48
    values = [v for s in range(1, 11) for v in ((1 << s) - 1, -((1 << s) - 1), 1 << (s - 1), -(1 << (s - 1)))]
    blocks, level = [], 0
    for i, d in enumerate(diffs):
        level += d
        assert -1024 <= level <= 1016
        blocks.append(zz_block(level, {1 + (i * 11) % 63: values[i]} if i < 40 else {}))
    data, st = W.write_jpeg(64, 48, [blocks], {0: ONES}, {0: DC_ALL}, {0: ac})
    assert st["codes"][("dc", 0)][1:13] == [4] + [4] * 10 + [4]
    assert {s & 15 for s in st["symbols"][("ac", 0)]} == set(range(11))
    return {"magnitudes_gray_48x64": (data, st)}


def case_runs():
    """Gray 32x56, 28 blocks: every run 0..15 in front of a value; one, two and three ZRLs and then a value; a value at
    coefficient 63 and no EOB; a block of 63 nonzero ACs; and by escape four ZRLs (the index passes 64 and nothing is
    written), ZRL and then EOB, and the fourteen symbols 0x10..0xE0, on which libjpeg ends the block."""
    odd = [r << 4 for r in range(1, 15)]
    ac_sym = [0x00, 0x01] + [r << 4 | 1 for r in range(1, 16)] + [0x02, 0x12, 0xE2, 0xF0] + odd
    ac = W.huffman_from_lengths(ac_sym, [2, 3] + [6] * 15 + [6, 6, 6, 6] + [11] * 14)
    acs = _pack([r << 4 | 1 for r in range(16)])
    assert len(acs) == 3
    acs += [{17: 1}, {33: -1}, {49: 1}, {23: -1, 40: 1}, {63: 2}, {k: (-1) ** k * (1 + k % 2) for k in range(1, 64)}]
    blocks = [zz_block(12 * (-1) ** i, a) for i, a in enumerate(acs)]
    blocks.append([(3, 5)] + [(W.ZRL, 0)] * 4)
    blocks.append([(3, -5), (0x01, 1), (W.ZRL, 0), (W.EOB, 0)])
    blocks += [[(2, 3 * (-1) ** r), (0x01, (-1) ** r), (r << 4, 0)] for r in range(1, 15)]
    blocks += [zz_block(12, {2: 1})] * (28 - len(blocks))
    data, st = W.write_jpeg(56, 32, [blocks], {0: ONES * 6}, {0: DC_ALL}, {0: ac})
    assert st["symbols"][("ac", 0)] >= set(r << 4 | 1 for r in range(16)) | set(odd) | {W.ZRL, W.EOB}
    assert st["zrl"] == 1 + 2 + 3 + 2 + 3 + 4 + 1 and st["end63"] == 2 and st["eob"] == 28 - 2 - 1 - 14
    return {"runs_gray_32x56": (data, st)}


def _colour_blocks(h, w, sampling, seed, quants):
    """The quantised blocks of a textured image in Y, Cb, Cr on the MCU-padded grid."""
    mw, mh, grid = W.block_grid(w, h, sampling)
    return [list(quantised(textured(8 * bh, 8 * bw, seed + c), q)) for c, ((bw, bh), q) in enumerate(zip(grid, quants))]


def case_restarts():
    """4:2:0, 19x30: four MCUs of six blocks, two a row.  Restart intervals of 1 MCU, of one MCU row (2), of 3 (the first
    segment spans both rows, the last is short) and of 7 (a DRI, no marker).  The blocks alternate dark and bright, so the
    first DC of every segment is large and a predictor that is not reset shows.  One image, four files: equal pixels."""
    dc, ac = table_set(11)
    q = [steps(1), steps(2), steps(3)]
    blocks = _colour_blocks(19, 30, (2, 2), 50, q)
    assert all(abs(int(comp[i][0]) * int(qq[0])) >= 300 for comp, qq in zip(blocks, q) for i in range(len(comp)))
    out = {}
    for ri, nseg in ((1, 4), (2, 2), (3, 2), (7, 1)):
        data, st = W.write_jpeg(30, 19, blocks, dict(enumerate(q)), {0: dc, 1: dc}, {0: ac, 1: ac}, sampling=(2, 2), restart=ri,
                                selectors=[(0, 0, 0), (1, 1, 1), (2, 1, 1)])
        assert len(st["segments"]) == nseg and [s["mcus"] for s in st["segments"]] == {1: [1] * 4, 2: [2, 2], 3: [3, 1], 7: [4]}[ri]
        assert (b"\xff\xd0" in data) == (ri < 4) and b"\xff\xdd\x00\x04" + bytes([0, ri]) in data
        out["restart%d_420_19x30" % ri] = (data, st)
    return out


def case_layouts():
    """4:4:4, 8x16, header layouts: every component on table 0; four selectors with the chroma components on 2 and 3 (and 1
    defined, unused); tables 0 defined twice, the later definition being the one the data was coded with, with fill bytes in
    front of every marker and COM / APP5 segments in between; and all tables in one DQT and one DHT segment."""
    sets = [table_set(20 + i) for i in range(4)]
    q = [steps(30 + i) for i in range(4)]
    out = {}

    def build(name, sel, tabs, **kw):
        blocks = _colour_blocks(8, 16, (1, 1), 60, [q[s[0]] for s in sel])
        data, st = W.write_jpeg(16, 8, blocks, {k: q[k] for k in tabs}, {k: sets[k][0] for k in tabs}, {k: sets[k][1] for k in tabs},
                                sampling=(1, 1), selectors=sel, **kw)
        out[name] = (data, st)
        return data
    build("layout_table0_444_8x16", [(0, 0, 0)] * 3, [0])
    data = build("layout_four_444_8x16", [(0, 0, 0), (2, 2, 2), (3, 3, 3)], [0, 1, 2, 3])
    assert data.count(b"\xff\xdb") == 4 and data.count(b"\xff\xc4") == 8
    data = build("layout_redefined_444_8x16", [(0, 0, 0), (1, 1, 1), (1, 1, 1)], [0, 1], fill=2,
                 dqt_layout=[[(0, q[3])], [1], [0]], dht_layout=[[("dc", 0, sets[3][0])], [("ac", 0, sets[2][1]), ("ac", 1)], [("dc", 1)],
                                                                 [("dc", 0), ("ac", 0)]],
                 extra=[("soi", 0xFE, b"a comment"), ("dqt", 0xE5, b"\xff\xd8 not a marker"), ("dht", 0xFE, b"")])
    assert data.count(b"\xff\xff\xff\xdb") == 3 and data.count(b"\xff\xff\xff\xc4") == 4 and b"\xff\xff\xff\xda" in data
    data = build("layout_merged_444_8x16", [(0, 0, 0), (1, 1, 1), (1, 1, 1)], [0, 1], dqt_layout=[[0, 1]],
                 dht_layout=[[("dc", 0), ("ac", 0), ("dc", 1), ("ac", 1)]])
    assert data.count(b"\xff\xdb") == 1 and data.count(b"\xff\xc4") == 1
    return out


def case_batches():
    """4:2:0, 19x30, two batches of three: ``sets_i`` with three table sets of their own, ``one_i`` sharing one; in both the
    images have different restart intervals (1, 3 and none / 2, none and 1)."""
    out = {}
    for i, ri in enumerate((1, 3, 0)):
        dc, ac = table_set(40 + i)
        q = [steps(41 + i), steps(44 + i), steps(47 + i)]
        blocks = _colour_blocks(19, 30, (2, 2), 70 + 3 * i, q)
        out["sets_%d" % i] = W.write_jpeg(30, 19, blocks, dict(enumerate(q)), {0: dc, 1: DC_ALL}, {0: ac, 1: table_set(50 + i)[1]},
                                          sampling=(2, 2), restart=ri, selectors=[(0, 0, 0), (1, 1, 1), (2, 1, 1)])
    dc, ac = table_set(60)
    q = [steps(61), steps(62)]
    for i, ri in enumerate((2, 0, 1)):
        blocks = _colour_blocks(19, 30, (2, 2), 80 + 3 * i, [q[0], q[1], q[1]])
        out["one_%d" % i] = W.write_jpeg(30, 19, blocks, dict(enumerate(q)), {0: dc, 1: DC_ALL}, {0: ac, 1: ac}, sampling=(2, 2), restart=ri)
    assert [len(out["sets_%d" % i][1]["segments"]) for i in range(3)] == [4, 2, 1]
    assert [len(out["one_%d" % i][1]["segments"]) for i in range(3)] == [2, 1, 4]
    return out


def basis_image():
    """u8 [64,64]: block (v, u) is the sign pattern of DCT basis function (v, u): 255 where it is positive, else 0."""
    k, x = np.mgrid[:8, :8]
    c = np.cos((2 * x + 1) * k * np.pi / 16)  # [k, x]
    img = np.zeros((64, 64), dtype=np.uint8)
    for v in range(8):
        for u in range(8):
            img[8 * v:8 * v + 8, 8 * u:8 * u + 8] = np.where(np.outer(c[v], c[u]) > 0, 255, 0)
    return img


def case_basis():
    """The basis sign image and its negative, encoded by PIL at quality 100, 95 and 50 in gray, 4:4:4, 4:2:2 and 4:2:0 (the
    colour files carry the image in R and B and its negative in G: magenta against green, so the chroma planes are as extreme)."""
    out = {}
    pos = basis_image()
    for tag, a in (("pos", pos), ("neg", 255 - pos)):
        rgb = np.stack([a, 255 - a, a], -1)
        for q in (100, 95, 50):
            for fmt, sub in (("gray", None), ("444", 0), ("422", 1), ("420", 2)):
                buf = io.BytesIO()
                kw = {} if sub is None else {"subsampling": sub}
                Image.fromarray(np.ascontiguousarray(a if sub is None else rgb)).save(buf, "JPEG", quality=q, optimize=True, **kw)
                out["basis_%s_%s_64x64_q%d" % (tag, fmt, q)] = (buf.getvalue(), None)
    return out


def cases():
    """name -> (file bytes, the writer's stats; None for the files PIL encoded)."""
    out = {}
    for build in (case_lengths, case_full_lengths, case_ac256, case_phases, case_tails, case_marker_wrap, case_magnitudes, case_runs, case_restarts,
                  case_layouts, case_batches, case_basis):
        out.update(build())
    return out


# ------------------------------------------------------------------------------------------------------ streams that fail

BAD_CODE, BAD_RUN, OUT_OF_BITS = 1, 2, 4  # the status bits of include/va.h, written down here: nothing is imported


def _gray(w, h, blocks, **kw):
    return W.write_jpeg(w, h, [blocks], {0: ONES * 4}, {0: DC_ALL}, {0: AC_SMALL}, **kw)[0]


def _good_block(k):
    return [(3, 5 - k), (0x01, 1), (0x01, -1), (W.EOB, 0)]


def status_streams():
    """name -> (file bytes, the status by construction).  The tables give category 0 and EOB the code '0', so the zero bits
    the bit reader supplies behind a segment's end decode cleanly and only the intended bit can be set.  Gray 8x16, two
    blocks: ``bad_code`` has sixteen 1-bits where the second block's first AC code is due (no code of AC_SMALL starts with
    six ones), ``bad_code_dc`` where its DC code is due; ``bad_run`` three ZRLs and then run 15, size 1: coefficient 64;
    ``exact`` ends its last block on the last bit of its last byte (status 0) and ``short`` is ``exact`` without that byte.
    ``rows_*`` are gray 24x24 with a restart per MCU row; in ``rows_bad_*`` the middle segment alone is corrupt."""
    out = {}
    out["bad_code"] = (_gray(16, 8, [_good_block(0), [(2, 3), "1" * 16]]), BAD_CODE)
    out["bad_code_dc"] = (_gray(16, 8, [_good_block(0), ["1" * 16]]), BAD_CODE)
    out["bad_run"] = (_gray(16, 8, [_good_block(0), [(2, -3)] + [(W.ZRL, 0)] * 3 + [(0xF1, 1)]]), BAD_RUN)
    # 7 + 6 + 1 bits, then 3 + 11 + 3 + 1: the second block ends on the last bit of byte 4
    exact, st = W.write_jpeg(16, 8, [[_good_block(0), [(1, 1), (0x08, 77), (0x01, -1), (W.EOB, 0)]]], {0: ONES * 4},
                             {0: DC_ALL}, {0: AC_SMALL})
    assert st["segments"][0]["padding"] == 0 and st["segments"][0]["bytes"] == 4 and not st["segments"][0]["stuffed"]
    assert exact[-3] not in (0x00, 0xFF) and exact[-4] != 0xFF
    out["exact"] = (exact, 0)
    out["short"] = (exact[:-3] + exact[-2:], OUT_OF_BITS)
    rows = [[(3, 4 + (i % 3)) if i % 3 == 0 else (2, -2), (0x01, (-1) ** i), (0x08, 100 + 10 * i), (W.EOB, 0)] for i in range(9)]
    out["rows_good"] = (_gray(24, 24, rows, restart=3), 0)
    for name, bad, bit in (("rows_bad_code", [(2, 3), (0x01, 1), "1" * 16], BAD_CODE),
                           ("rows_bad_run", [(2, 3)] + [(W.ZRL, 0)] * 3 + [(0xF1, -1)], BAD_RUN)):
        out[name] = (_gray(24, 24, rows[:4] + [bad] + rows[5:], restart=3), bit)
    return out


def compute():
    out = {}
    for name, (data, _) in cases().items():
        out["jpg_" + name] = np.frombuffer(data, dtype=np.uint8)
        out["px_" + name] = pil_pixels(data)
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **compute())
    print(OUT, os.path.getsize(OUT), "bytes")
