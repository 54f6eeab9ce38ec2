"""Baseline JPEG decoding on the host: jpeg.decode_jpegs_host, the numpy statement of the device decoder,
against PIL on the recorded fixtures (tests/golden/jpeg_small.npz), on PIL's decode of the same files here and on fresh PIL
encodes; every rejection of jpeg.parse_jpeg; segment splitting and un-stuffing; the packed upload; utils.videoJpegs on an AVI
built by hand; and utils.loadFlowImages / saveFlowImages, whose defaults keep their bytes."""
import importlib.util
import inspect
import io
import os
import struct

import numpy as np
import pytest
from PIL import Image

from video_analytics_amd import jpeg, utils

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_jpeg_golden", os.path.join(HERE, "golden", "make_jpeg_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


GEN = _generator()


def load_golden():
    """name -> (file bytes, PIL's pixels as recorded)."""
    z = np.load(GEN.OUT)
    return {k[4:]: (z[k].tobytes(), z["px_" + k[4:]]) for k in z.files if k.startswith("jpg_")}


GOLDEN = load_golden()


def test_the_fixture_file_is_small_and_complete():
    assert os.path.getsize(GEN.OUT) < 256 * 1024
    fresh = GEN.cases()
    assert sorted(fresh) == sorted(GOLDEN) and len(GOLDEN) >= 40
    for size in ("16x16", "24x40", "37x53", "19x30", "8x17"):
        for fmt in ("gray", "444", "422", "420"):
            assert any(n.startswith("%s_%s_q" % (fmt, size)) for n in GOLDEN), (fmt, size)
    assert {n.rsplit("_q", 1)[1] for n in GOLDEN if "_q" in n} >= {"20", "75", "95", "100"}
    assert any(n.startswith("restart2") for n in GOLDEN) and any(n.startswith("restart3") for n in GOLDEN)
    for n in GOLDEN:
        if n.startswith("nodht"):
            assert b"\xff\xc4" not in GOLDEN[n][0][:GOLDEN[n][0].index(b"\xff\xda")]
    GEN.check_targets({n: d for n, (d, _) in GOLDEN.items()})  # category 11, a long code, ZRL, EOB, both clips


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_host_decoder_equals_pil(name):
    data, want = GOLDEN[name]
    got = jpeg.decode_jpegs_host([data])[0]
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), "%d values differ from the recorded pixels" % int((got != want).sum())
    assert np.array_equal(got, GEN.pil_pixels(data)), "differs from this machine's PIL"


def test_host_decoder_equals_pil_on_fresh_encodes():
    """What this machine's PIL writes today (the bytes may differ from the recorded files) decodes to what it reads."""
    for name, data in GEN.cases().items():
        assert np.array_equal(jpeg.decode_jpegs_host([data])[0], GEN.pil_pixels(data)), name


def test_a_batch_decodes_image_by_image_and_mixed_batches_raise():
    datas = [GOLDEN["batch_%d" % i][0] for i in range(5)]
    got = jpeg.decode_jpegs_host(datas)
    assert got.shape == (5, 3, 24, 40)
    for i in range(5):
        assert np.array_equal(got[i], GOLDEN["batch_%d" % i][1])
    for other in ("gray_24x40_q75", "444_24x40_q95", "420_16x16_q95"):
        name = [n for n in GOLDEN if n.startswith(other.rsplit("_q", 1)[0] + "_q")][0]
        with pytest.raises(ValueError, match="one call takes one size and format"):
            jpeg.decode_jpegs_host([datas[0], GOLDEN[name][0]])
    with pytest.raises(ValueError, match="no images"):
        jpeg.decode_jpegs_host([])


def test_standard_tables_are_the_ones_pil_writes():
    hdr = jpeg.parse_jpeg(GOLDEN["batch_0"][0])
    for key, (bits, vals) in jpeg.STD_HUFFMAN.items():
        assert (list(hdr["huffman"][key][0]), list(hdr["huffman"][key][1])) == (list(bits), list(vals)), key
    bare = jpeg.parse_jpeg(GOLDEN["nodht_420_24x40_q95"][0])
    assert bare["huffman"] == jpeg.STD_HUFFMAN


# ---- parse_jpeg: the header and every rejection ----

def _segment(data, marker, start=2):
    """(offset of the marker's FF, segment length incl. the length field) of the first ``marker`` segment."""
    p = start
    while True:
        assert data[p] == 0xFF
        m, L = data[p + 1], struct.unpack(">H", data[p + 2:p + 4])[0]
        if m == marker:
            return p, L
        assert m != 0xDA
        p += 2 + L


def _edit(data, at, value):
    b = bytearray(data)
    b[at] = value
    return bytes(b)


def _pil(mode="RGB", size=(40, 24), **kw):
    a = GEN.image(size[1], size[0], 1 if mode == "L" else 3, 7)
    buf = io.BytesIO()
    Image.fromarray(a[..., 0] if mode == "L" else a, mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_parse_jpeg_reads_the_header():
    hdr = jpeg.parse_jpeg(GOLDEN["restart3_420_37x53"][0])
    assert (hdr["width"], hdr["height"]) == (53, 37) and (hdr["mcu_w"], hdr["mcu_h"], hdr["mcus"]) == (4, 3, 12)
    assert [(c["h"], c["v"]) for c in hdr["components"]] == [(2, 2), (1, 1), (1, 1)]
    assert [(c["tq"], c["td"], c["ta"]) for c in hdr["components"]] == [(0, 0, 0), (1, 1, 1), (1, 1, 1)]
    # PIL counts restart_marker_blocks in MCUs
    assert hdr["restart_interval"] == 3 and len(hdr["segments"]) == 4
    assert hdr["quant"][0].dtype == np.uint16 and hdr["quant"][0].shape == (64,)
    # natural order: PIL's own tables are in zigzag order
    im = Image.open(io.BytesIO(GOLDEN["restart3_420_37x53"][0]))
    zz = np.asarray(im.quantization[0])
    natural = np.zeros(64, dtype=np.int64)
    natural[jpeg.ZIGZAG] = zz
    assert np.array_equal(hdr["quant"][0], natural) or np.array_equal(hdr["quant"][0], zz)  # older PILs hand them over de-zigzagged
    gray = jpeg.parse_jpeg(GOLDEN["checker"][0])
    assert len(gray["components"]) == 1 and gray["restart_interval"] == 0 and len(gray["segments"]) == 1 and gray["mcus"] == 8


def _rejections():
    good, gray = _pil(quality=90, subsampling=2), _pil("L", quality=90)
    sof, _ = _segment(good, 0xC0)
    dqt, _ = _segment(good, 0xDB)
    sos, sos_len = _segment(good, 0xDA)
    app0, app0_len = _segment(good, 0xE0)
    gsof, _ = _segment(gray, 0xC0)
    cases = {
        "progressive": (_pil(quality=90, progressive=True), "progressive"),
        "extended": (_edit(good, sof + 1, 0xC1), "SOF1"),
        "arithmetic": (_edit(good, sof + 1, 0xC9), "arithmetic"),
        "12-bit": (_edit(good, sof + 4, 12), "12-bit"),
        "16-bit quant": (_edit(good, dqt + 4, 0x10), "16-bit quantisation"),
        "two scans (first holds one component)": (_edit(good, sos + 4, 1), "more than one scan"),
        "two scans (a second SOS)": (good[:-2] + good[sos:sos + 2 + sos_len] + b"\x00\xff\xd9", "more than one scan"),
        "2 components": (_edit(good, sof + 9, 2), "2 components"),
        "4 components": (_pil_cmyk(), "4 components"),
        "adobe transform 0": (good[:app0] + _adobe(0) + good[app0 + 2 + app0_len:], "not YCbCr"),
        "ids RGB without JFIF": (_rgb_ids(good, app0, app0_len, sof, sos), "not YCbCr"),
        "luma 1x2": (_edit(good, sof + 11, 0x12), "sampling"),
        "chroma 2x1": (_edit(good, sof + 14, 0x21), "sampling"),
        "gray 2x2": (_edit(gray, gsof + 11, 0x22), "sampling"),
        "width 2": (_edit(_edit(good, sof + 7, 0), sof + 8, 2), "below the smallest size"),
        "height 2": (_edit(_edit(good, sof + 5, 0), sof + 6, 2), "below the smallest size"),
        "truncated in a segment": (good[:sof + 6], "truncated header"),
        "truncated before the scan": (good[:sos], "truncated header"),
        "not a JPEG": (b"RIFF" + good[4:], "not a JPEG"),
    }
    return cases


def _adobe(transform):
    return b"\xff\xee" + struct.pack(">H", 14) + b"Adobe" + struct.pack(">HHHB", 100, 0, 0, transform)


def _pil_cmyk():
    buf = io.BytesIO()
    Image.new("CMYK", (16, 16), (10, 20, 30, 40)).save(buf, "JPEG")
    return buf.getvalue()


def _rgb_ids(good, app0, app0_len, sof, sos):
    b = bytearray(good)
    for i, cid in enumerate(b"RGB"):
        b[sof + 10 + 3 * i] = cid
        b[sos + 5 + 2 * i] = cid
    return bytes(b[:app0] + b[app0 + 2 + app0_len:])


REJECTIONS = _rejections()


@pytest.mark.parametrize("case", sorted(REJECTIONS))
def test_parse_jpeg_rejects(case):
    data, reason = REJECTIONS[case]
    with pytest.raises(ValueError, match=reason):
        jpeg.parse_jpeg(data)
    with pytest.raises(ValueError, match=reason):  # and so does the decoder, before any decoding
        jpeg.decode_jpegs_host([data])


def test_parse_jpeg_accepts_what_pil_takes_as_ycbcr():
    good = _pil(quality=90, subsampling=0)
    app0, app0_len = _segment(good, 0xE0)
    adobe1 = good[:app0] + _adobe(1) + good[app0 + 2 + app0_len:]   # Adobe transform 1: YCbCr
    assert np.array_equal(jpeg.decode_jpegs_host([adobe1])[0], GEN.pil_pixels(adobe1))
    bare = good[:app0] + good[app0 + 2 + app0_len:]                 # no JFIF, no Adobe, ids 1 2 3: YCbCr
    assert np.array_equal(jpeg.decode_jpegs_host([bare])[0], GEN.pil_pixels(bare))


def test_segments_are_split_at_restart_markers_and_unstuffed():
    a = np.random.RandomState(3).randint(0, 256, size=(24, 40, 3)).astype(np.uint8)
    data = GEN.encode(a, "RGB", 2, 100, restart_marker_blocks=2)
    sos, sos_len = _segment(data, 0xDA)
    scan = data[sos + 2 + sos_len:-2]
    assert data[-2:] == b"\xff\xd9" and b"\xff\x00" in scan  # the case is there
    hdr = jpeg.parse_jpeg(data)
    assert hdr["restart_interval"] == 2 and hdr["mcus"] == 6 and len(hdr["segments"]) == 3
    assert sum(seg.count(b"\xff") for seg in hdr["segments"]) == scan.count(b"\xff\x00")  # every stuffed FF is a plain FF now
    again = b""
    for k, seg in enumerate(hdr["segments"]):
        again += (b"\xff" + bytes([0xD0 + (k - 1) % 8]) if k else b"") + seg.replace(b"\xff", b"\xff\x00")
    assert again == scan
    assert np.array_equal(jpeg.decode_jpegs_host([data])[0], GEN.pil_pixels(data))
    # a restart count that does not fit the MCUs
    dri, _ = _segment(data, 0xDD)
    with pytest.raises(ValueError, match="restart intervals"):
        jpeg.parse_jpeg(_edit(data, dri + 5, 4))


def test_truncated_entropy_data_is_an_error_of_the_decoder_not_a_crash():
    data = GOLDEN["shared_1"][0]
    sos, sos_len = _segment(data, 0xDA)
    start = sos + 2 + sos_len
    cut = data[:start + (len(data) - 2 - start) // 2] + b"\xff\xd9"
    assert jpeg.parse_jpeg(cut)["width"] == 40
    with pytest.raises(ValueError, match="image 1 did not decode"):
        jpeg.decode_jpegs_host([GOLDEN["shared_0"][0], cut, GOLDEN["shared_2"][0]])


def _resized(data, w, h):
    """The file with another size in its frame header."""
    sof, _ = _segment(data, 0xC0)
    b = bytearray(data)
    b[sof + 5:sof + 9] = struct.pack(">HH", h, w)
    return bytes(b)


def test_sizes_whose_samples_do_not_fit_32_bits_are_refused_everywhere():
    """One image holds at most 2**31 - 1 MCU-padded samples: the device counts them in an int.  A few hundred bytes whose
    frame header claims more are refused by parse_jpeg, by decode_jpegs before the device and by the library, and just below
    the limit the library's workspace is the sum worked out here in Python integers (it passes 2**32)."""
    from video_analytics_amd import _ffi
    lib = _ffi.lib()
    files = dict(gray=(_pil("L", quality=90), 1, 1, 1), c444=(_pil(quality=90, subsampling=0), 3, 1, 1),
                 c422=(_pil(quality=90, subsampling=1), 3, 2, 1), c420=(_pil(quality=90, subsampling=2), 3, 2, 2))

    def samples(w, h, nc, hs, vs):
        return jpeg.layout(w, h, nc, hs, vs)["plane_bytes"]
    for name, (data, nc, hs, vs) in files.items():
        assert samples(65535, 65535, nc, hs, vs) > jpeg.MAX_SAMPLES
        big = _resized(data, 65535, 65535)
        with pytest.raises(ValueError, match="samples"):
            jpeg.parse_jpeg(big)
        with pytest.raises(ValueError, match="samples"):
            jpeg.decode_jpegs([big], "cuda")
        with pytest.raises(ValueError, match="samples"):
            jpeg.decode_jpegs_host([big])
        assert lib.va_jpeg_decode_workspace_bytes(1, 65535, 65535, nc, hs, vs) == 0, name
        # the largest square of whole blocks that fits, and the sizes just past it
        side = 16
        while samples(side + 8, side + 8, nc, hs, vs) <= jpeg.MAX_SAMPLES:
            side += 8
        assert side < 65535
        geo = jpeg.layout(side, side, nc, hs, vs)
        want = -(-2 * geo["blocks"] * 128 // 256) * 256 + (2 * geo["plane_bytes"] if nc == 3 else 0)  # two images
        assert lib.va_jpeg_decode_workspace_bytes(2, side, side, nc, hs, vs) == want and want > 2 ** 32, name
        assert jpeg.parse_jpeg(_resized(data, side, side))["width"] == side
        for more in (1, 8):
            fits = samples(side + more, side + more, nc, hs, vs) <= jpeg.MAX_SAMPLES  # one more pixel may still lie inside the MCUs
            assert (lib.va_jpeg_decode_workspace_bytes(1, side + more, side + more, nc, hs, vs) > 0) == fits, (name, more)
            if fits:
                assert jpeg.parse_jpeg(_resized(data, side + more, side + more))["width"] == side + more
            else:
                with pytest.raises(ValueError, match="samples"):
                    jpeg.parse_jpeg(_resized(data, side + more, side + more))
        assert samples(side + 8, side + 8, nc, hs, vs) > jpeg.MAX_SAMPLES
    assert lib.va_jpeg_decode_workspace_bytes(1, 65535, 8, 1, 1, 1) > 0  # a side alone may be the largest
    assert jpeg.parse_jpeg(_resized(files["gray"][0], 65535, 8))["mcu_w"] == 8192


def test_fill_bytes_in_front_of_markers_are_not_data():
    data = GOLDEN["restart3_420_37x53"][0]
    sos, sos_len = _segment(data, 0xDA)
    start = sos + 2 + sos_len
    scan = data[start:-2]
    filled, k = b"", 0
    while k < len(scan):
        if scan[k] == 0xFF and 0xD0 <= scan[k + 1] <= 0xD7:
            filled += b"\xff\xff" + scan[k:k + 2]  # two fill bytes in front of every RSTn
            k += 2
        else:
            filled += scan[k:k + 1]
            k += 1
    padded = data[:start] + filled + b"\xff\xff\xff\xd9"  # and in front of EOI
    assert len(padded) == len(data) + 2 * 3 + 2
    assert jpeg.parse_jpeg(padded)["segments"] == jpeg.parse_jpeg(data)["segments"]
    assert np.array_equal(jpeg.decode_jpegs_host([padded])[0], GOLDEN["restart3_420_37x53"][1])


def test_the_host_model_truncates_to_16_bits_like_the_kernel():
    """Only a corrupt file gets there: a DC sum past 32767 is stored as its low 16 bits, the kernel's (short)."""
    assert [jpeg._int16(v) for v in (0, 32767, 32768, 65534, -32768, -32769)] == [0, 32767, -32768, -2, -32768, 32767]
    dc = jpeg.huffman_table([1] + [0] * 15, [15], dc=True)   # the one code, '0', is category 15
    ac = jpeg.huffman_table([1] + [0] * 15, [0])             # the one code, '0', is EOB
    bits = ("0" + "1" * 15 + "0") * 2                         # twice: DC difference +32767, EOB
    seg = int(bits.ljust(40, "1"), 2).to_bytes(5, "big")
    coef = np.zeros((2, 64), dtype=np.int16)
    geo = jpeg.layout(16, 8, 1, 1, 1)
    assert jpeg._decode_segment(seg, 0, 2, geo, [dict(h=1, v=1)], [(dc, ac)], coef, {}) == 0
    assert coef[:, 0].tolist() == [32767, -2] and not coef[:, 1:].any()


def test_parse_errors_are_value_errors_with_their_reason_and_nothing_is_relabelled():
    """Every truncation is found by a length check of its own: parse_jpeg holds no blanket handler that would turn an indexing
    mistake of the parser into 'truncated header'."""
    import ast
    src = inspect.getsource(jpeg.parse_jpeg) + inspect.getsource(jpeg._parse)
    assert not [n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.Try)]
    good = _pil(quality=90, subsampling=2)
    sos, sos_len = _segment(good, 0xDA)
    for cut in range(2, sos + 2 + sos_len, 3):  # a file cut anywhere in its header
        with pytest.raises(ValueError):
            jpeg.parse_jpeg(good[:cut])


def test_huffman_table_form():
    bits, vals = jpeg.STD_HUFFMAN[(1, 0)]
    look, maxcode, valoff, out = jpeg.huffman_table(bits, vals)
    assert look.dtype == np.uint16 and look.shape == (1 << jpeg.LOOK_BITS,) and maxcode.shape == valoff.shape == (18,)
    assert look.tobytes() + maxcode.tobytes() + valoff.tobytes() + out.tobytes() and 1024 + 72 + 72 + 256 == jpeg.HUFF_BYTES
    # the two 2-bit codes 00 and 01 are symbols 1 and 2; 1010 is EOB (symbol 0); the 16-bit codes end at 0xFFFE
    assert look[0] == (2 << 8) | 1 and look[0b010000000] == (2 << 8) | 2 and look[0b101000000] == (4 << 8) | 0
    assert maxcode[16] == 0xFFFE and maxcode[1] == -1 and maxcode[12] == 0xFF7 and maxcode[13] == 0x1FEF and (np.diff(maxcode[1:17]) >= 0).all() and out[int(valoff[16]) + 0xFFFE] == 0xFA
    assert int((look == 0).sum()) == 5 and (look[-5:] == 0).all()  # the longer codes start with the last five 9-bit prefixes
    with pytest.raises(ValueError):
        jpeg.huffman_table([3] + [0] * 15, [1, 2, 3])  # three codes of one bit
    with pytest.raises(ValueError):
        jpeg.huffman_table(bits, vals[:-1])
    with pytest.raises(ValueError):
        jpeg.huffman_table([0, 1] + [0] * 14, [16], dc=True)


def test_pack_jpegs_keeps_identical_table_sets_once_and_aligns_segments():
    for prefix, nsets in (("batch", 3), ("shared", 1)):
        hdrs = [jpeg.parse_jpeg(GOLDEN["%s_%d" % (prefix, i)][0]) for i in range(5)]
        packed, nseg, n = jpeg.pack_jpegs(hdrs)
        assert (nseg, n) == (5, nsets)
        img = np.frombuffer(packed, dtype=np.int32, count=20).reshape(5, 4)
        assert img[:, 1].tolist() == [0, 1, 2, 3, 4] and img[:, 2].tolist() == [1] * 5 and int(img[:, 0].max()) == nsets - 1
        if prefix == "batch":
            assert img[:, 0].tolist() == [0, 1, 2, 1, 0]
        seg = np.frombuffer(packed, dtype=np.int32, count=40, offset=80).reshape(5, 8)
        data_off = 80 + 5 * 32 + nsets * jpeg.SET_BYTES
        assert (seg[:, 1] % 4 == 0).all() and seg[:, 0].tolist() == [0, 1, 2, 3, 4] and (seg[:, 3] == 0).all() and (seg[:, 4] == 6).all()
        for row, hdr in zip(seg, hdrs):
            assert packed[data_off + row[1]:data_off + row[1] + row[2]] == hdr["segments"][0]
        assert len(packed) == data_off + int(seg[-1, 1]) + (int(seg[-1, 2]) + 3) // 4 * 4
    rst = jpeg.parse_jpeg(GOLDEN["restart3_420_37x53"][0])
    packed, nseg, n = jpeg.pack_jpegs([rst, rst])
    assert (nseg, n) == (8, 1)
    seg = np.frombuffer(packed, dtype=np.int32, count=64, offset=32).reshape(8, 8)
    assert seg[:, 0].tolist() == [0] * 4 + [1] * 4 and seg[:, 3].tolist() == [0, 3, 6, 9] * 2 and seg[:, 4].tolist() == [3] * 8


def test_layout_and_stage_models():
    geo = jpeg.layout(53, 37, 3, 2, 2)
    assert (geo["mcu_w"], geo["mcu_h"]) == (4, 3) and geo["blocks_w"] == [8, 4, 4] and geo["blocks_h"] == [6, 3, 3]
    assert geo["block_base"] == [0, 48, 60] and geo["blocks"] == 72 and geo["plane_bytes"] == 72 * 64
    assert jpeg.layout(53, 37, 1, 1, 1)["blocks_w"] == [7]
    # a flat block: DC 8 * (v - 128) decodes to v
    c = np.zeros((1, 64), dtype=np.int16)
    c[0, 0] = 8 * (200 - 128)
    assert (jpeg.idct_blocks(c, np.ones(64, dtype=np.uint16)) == 200).all()
    s = np.array([[10, 20, 40]])
    assert jpeg.upsample_h2v1(s).tolist() == [[10, 13, 17, 25, 35, 40]]
    assert jpeg.upsample_h2v2(np.array([[16, 32], [48, 64]]))[0].tolist() == [16, 20, 28, 32]
    assert jpeg.ycc_to_rgb([[128]], [[128]], [[128]]).reshape(-1).tolist() == [128, 128, 128]
    assert jpeg.ycc_to_rgb([[255]], [[128]], [[255]]).reshape(-1).tolist() == [255, 164, 255]


# ---- utils ----

def _write_mjpeg_avi(path, jpegs, fourcc=b"MJPG"):
    """Minimal RIFF/AVI writer: one video stream, one '00dc' chunk per JPEG, every second pair inside a 'rec ' list."""
    chunks = b""
    for k, d in enumerate(jpegs):
        c = b"00dc" + struct.pack("<I", len(d)) + d + (b"\0" if len(d) & 1 else b"")
        if k % 4 == 1:
            c = b"LIST" + struct.pack("<I", 4 + len(c)) + b"rec " + c
        chunks += c
    chunks += b"01wb" + struct.pack("<I", 4) + b"\x01\x02\x03\x04"  # an audio chunk: not a frame
    movi = b"LIST" + struct.pack("<I", 4 + len(chunks)) + b"movi" + chunks
    strh = b"strh" + struct.pack("<I", 56) + b"vids" + fourcc + b"\0" * 48
    strl = b"LIST" + struct.pack("<I", 4 + len(strh)) + b"strl" + strh
    hdrl = b"LIST" + struct.pack("<I", 4 + len(strl)) + b"hdrl" + strl
    body = b"AVI " + hdrl + movi
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def video_jpegs(n, h, w, **kw):
    """n textured frames as JPEG byte strings (quality 95, 4:2:0 unless ``kw`` says otherwise)."""
    kw.setdefault("quality", 95)
    return [GEN.encode(GEN.image(h, w, 3, 900 + i), "RGB", kw.pop("sub", 2), **dict(kw)) for i in range(n)]


def test_video_jpegs_walks_the_movi_list(tmp_path):
    jpegs = video_jpegs(6, 24, 32)
    path = str(tmp_path / "v.avi")
    _write_mjpeg_avi(path, jpegs)
    assert utils.videoJpegs(path) == jpegs
    frames = list(utils.iterVideoFrames(path))
    assert len(frames) == 6 and all(f.mode == "RGB" and f.size == (32, 24) for f in frames)
    for f, d in zip(frames, jpegs):
        assert np.array_equal(np.asarray(f), np.asarray(Image.open(io.BytesIO(d)).convert("RGB")))
        assert np.array_equal(np.asarray(f).transpose(2, 0, 1), jpeg.decode_jpegs_host([d])[0])
    _write_mjpeg_avi(str(tmp_path / "x.avi"), jpegs, fourcc=b"XVID")
    with pytest.raises(ValueError, match="XVID"):
        utils.videoJpegs(str(tmp_path / "x.avi"))
    it = utils.iterVideoFrames(str(tmp_path / "x.avi"))  # still a generator: the error comes with the first frame
    with pytest.raises(ValueError, match="XVID"):
        next(it)
    (tmp_path / "n.avi").write_bytes(b"not a riff file")
    with pytest.raises(ValueError, match="not a RIFF/AVI"):
        utils.videoJpegs(str(tmp_path / "n.avi"))


def _flow(n, h, w, seed=0):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w]
    return np.stack([np.stack([8 * np.sin(xx / 7.0 + k) + rs.standard_normal((h, w)), 6 * np.cos(yy / 5.0 - k) + rs.standard_normal((h, w))])
                     for k in range(n)]).astype(np.float32)


def test_flow_images_keep_their_bytes_and_their_reader(tmp_path):
    fl = _flow(3, 24, 40)
    d, r = str(tmp_path / "plain"), str(tmp_path / "restart")
    assert utils.saveFlowImages(fl, d) == 6 and utils.saveFlowImages(fl, r, restartBlocks=5) == 6
    q = utils.flowToImages(fl)
    for k in range(3):
        for prefix, plane in (("flow_x_", 0), ("flow_y_", 1)):
            name = utils.flowFileName(prefix, k + 1)
            buf = io.BytesIO()
            Image.fromarray(q[k, plane], mode="L").save(buf, "JPEG", quality=95)  # the bytes the function wrote before
            plain, restart = (open(os.path.join(x, name), "rb").read() for x in (d, r))
            assert plain == buf.getvalue()
            hdr = jpeg.parse_jpeg(restart)
            assert hdr["restart_interval"] == 5 and len(hdr["segments"]) == 3 and jpeg.parse_jpeg(plain)["restart_interval"] == 0
    # the reader without a device: PIL's pixels, file by file
    want = np.stack([np.stack([np.asarray(Image.open(os.path.join(d, utils.flowFileName(p, k)))) for p in ("flow_x_", "flow_y_")])
                     for k in (1, 2, 3)])
    got = utils.loadFlowImages(d)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(utils.loadFlowImages(d, first=2, count=2), want[1:])
    assert np.array_equal(utils.loadFlowImages(r), want)  # restart markers change the bytes, not the pixels
    assert np.array_equal(jpeg.decode_jpegs_host([open(os.path.join(r, utils.flowFileName("flow_y_", 2)), "rb").read()])[0], want[1, 1])
    with pytest.raises(ValueError, match="missing"):
        utils.loadFlowImages(d, count=4)
    with pytest.raises(ValueError, match="count"):
        utils.loadFlowImages(d, count=0)


def test_the_new_arguments_default_to_the_old_behaviour():
    p = inspect.signature(utils.loadFlowImages).parameters
    assert list(p) == ["flowDir", "first", "count", "device"] and p["device"].default is None
    p = inspect.signature(utils.saveFlowImages).parameters
    assert list(p) == ["flow", "flowDir", "bound", "firstIndex", "quality", "restartBlocks"] and p["restartBlocks"].default is None
    p = inspect.signature(jpeg.decode_jpegs).parameters
    assert list(p) == ["datas", "device", "out", "check"] and p["out"].default is None and p["check"].default is True
    for f in (utils.videoJpegs, utils.loadVideoFrames, utils.loadFrameImages):
        assert callable(f)


def test_device_entry_points_raise_before_the_device():
    """Everything ``decode_jpegs`` refuses on the host is refused without a GPU in the machine."""
    good = GOLDEN["shared_0"][0]
    with pytest.raises(ValueError, match="progressive"):
        jpeg.decode_jpegs([REJECTIONS["progressive"][0]], "cuda")
    with pytest.raises(ValueError, match="one call takes one size and format"):
        jpeg.decode_jpegs([good, GOLDEN["checker"][0]], "cuda")
    with pytest.raises(ValueError, match="CUDA device"):
        jpeg.decode_jpegs([good], "cpu")
    with pytest.raises(ValueError, match="no images"):
        jpeg.decode_jpegs([], "cuda")
