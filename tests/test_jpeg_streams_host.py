"""The JPEG decoder's host model on hand-built streams: tests/jpeg_writer.py writes baseline files from
coefficients, symbol lists and raw bits, tests/golden/make_jpeg_streams_golden.py builds the cases -- every code length, the
first and last code of every length, every bit phase, every segment tail, every magnitude, run and restart layout, and the
DCT basis sign images -- and asserts from the writer's own counts that each reaches its point; PIL's pixels are recorded in
tests/golden/jpeg_streams.npz.  Here: the writer's own checks, jpeg.decode_jpegs_host against the recorded pixels and this
machine's PIL, jpeg.parse_jpeg against what the writer was asked to write, and the status each corrupt stream gives, so that
a failure of tests/test_jpeg_streams_gpu.py can be told from a failure of the model."""
import importlib.util
import io
import os
import re
import warnings

import numpy as np
import pytest
from PIL import Image

from video_analytics_amd import jpeg

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_jpeg_streams_golden", os.path.join(HERE, "golden", "make_jpeg_streams_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


GEN = _generator()
W = GEN.W
CASES = GEN.cases()             # name -> (file bytes, the writer's stats), built now; every reach condition is asserted in there
STATUS = GEN.status_streams()   # name -> (file bytes, the status by construction)


def load_golden():
    """name -> (file bytes, PIL's pixels as recorded)."""
    z = np.load(GEN.OUT)
    return {k[4:]: (z[k].tobytes(), z["px_" + k[4:]]) for k in z.files if k.startswith("jpg_")}


GOLDEN = load_golden()
WRITTEN = sorted(n for n in CASES if CASES[n][1] is not None)  # the writer's files; the others are PIL's encodes


def _scan(data):
    """The entropy-coded bytes of a file: behind the SOS header, in front of EOI and its fill bytes."""
    p = 2
    while True:
        while data[p + 1] == 0xFF:
            p += 1
        m, L = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        p += 2 + L
        if m == 0xDA:
            return data[p:-2].rstrip(b"\xff")


# ---- the writer and the fixture file ----

def test_the_fixture_file_is_small_complete_and_reproducible():
    assert os.path.getsize(GEN.OUT) < os.path.getsize(os.path.join(HERE, "golden", "jpeg_small.npz"))
    assert sorted(CASES) == sorted(GOLDEN)
    for name in WRITTEN:  # the writer is deterministic; PIL's encoder may change its bytes from version to version
        assert CASES[name][0] == GOLDEN[name][0], name
    assert len([n for n in GOLDEN if n.startswith("basis_")]) == 2 * 3 * 4
    for name, (_, px) in GOLDEN.items():
        assert px.shape[-1] <= 64 and px.shape[-2] <= 64, name


def test_huffman_from_lengths_builds_canonical_codes_and_refuses_bad_lengths():
    bits, vals = W.huffman_from_lengths([7, 5, 9], [3, 1, 3])  # a gap at length 2: '0', '100', '101'
    assert bits == [1, 0, 2] + [0] * 13 and vals == [5, 7, 9]
    assert W.code_table((bits, vals)) == {5: (0b0, 1, True, True), 7: (0b100, 3, True, False), 9: (0b101, 3, False, True)}
    table = W.code_table(W.huffman_from_lengths([7, 5, 9, 1], [3, 1, 4, 2]))
    assert table == {5: (0b0, 1, True, True), 1: (0b10, 2, True, True), 7: (0b110, 3, True, True), 9: (0b1110, 4, True, True)}
    W.huffman_from_lengths(range(16), range(1, 17))  # one code of every length: the all-ones code of 16 bits stays free
    for symbols, lengths in (([1, 2, 3], [1, 1, 2]),            # Kraft's inequality
                             ([1, 2], [1, 1]),                  # complete: '1' is all ones
                             ([1, 2, 3, 4], [2, 2, 2, 2]),      # complete
                             (list(range(17)), list(range(1, 17)) + [16]),  # 0xFFFF would be a code
                             ([1], [0]), ([1], [17]), ([1, 1], [2, 3]), ([256], [2]), ([1, 2], [3])):
        with pytest.raises(ValueError):
            W.huffman_from_lengths(symbols, lengths)


def test_block_pairs_is_the_baseline_symbol_sequence():
    c = GEN.zz_block(-5, {1: 3, 20: -1, 63: 7})
    assert W.block_pairs(c, pred=2) == [(3, -7), (0x02, 3), (W.ZRL, 0), (0x21, -1), (W.ZRL, 0), (W.ZRL, 0), (0xA3, 7)]
    assert W.block_pairs(GEN.zz_block(0), pred=0) == [(0, 0), (W.EOB, 0)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_pil_opens_every_case_without_a_warning(name):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(CASES[name][0]))
        im.load()
    assert im.format == "JPEG" and im.size == GOLDEN[name][1].shape[::-1][:2]
    assert np.array_equal(GEN.pil_pixels(GOLDEN[name][0]), GOLDEN[name][1]), "this machine's PIL differs from the recorded pixels"


@pytest.mark.parametrize("name", WRITTEN)
def test_stats_add_up(name):
    data, st = CASES[name]
    scan = _scan(data)
    parts = re.split(b"\xff+[\xd0-\xd7]", scan)
    assert len(parts) == len(st["segments"]) == -(-st["mcus"] // (st["restart"] or st["mcus"]))
    assert sum(s["mcus"] for s in st["segments"]) == st["mcus"] and [s["first"] for s in st["segments"]] == \
        list(range(0, st["mcus"], st["restart"] or st["mcus"]))
    for part, s in zip(parts, st["segments"]):
        assert len(part.replace(b"\xff\x00", b"\xff")) == s["bytes"] and part.count(b"\xff\x00") == s["stuffed"]
        assert s["bits"] + s["padding"] == 8 * s["bytes"] and 0 <= s["padding"] < 8 and s["ends_stuffed"] == part.endswith(b"\xff\x00")
    assert st["stuffed"] == sum(s["stuffed"] for s in st["segments"])
    blocks = sum(sum(st["codes"][k]) for k in st["codes"] if k[0] == "dc")  # one DC code a block
    hdr = jpeg.parse_jpeg(data)
    assert blocks == jpeg.layout(hdr["width"], hdr["height"], len(hdr["components"]), hdr["components"][0]["h"], hdr["components"][0]["v"])["blocks"]
    for key, counts in st["codes"].items():
        assert counts[0] == 0 and sum(1 for n in counts if n) == len(st["first_last"][key])
    if not name.startswith("runs"):  # there, escapes end blocks on other symbols
        assert st["eob"] + st["end63"] == blocks


# ---- the host model ----

@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_host_decoder_equals_pil_on_every_stream(name):
    data, want = GOLDEN[name]
    got = jpeg.decode_jpegs_host([data])[0]
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), "%d values differ from the recorded pixels" % int((got != want).sum())
    assert np.array_equal(got, GEN.pil_pixels(data)), "differs from this machine's PIL"


def test_host_decoder_equals_pil_on_fresh_basis_encodes():
    """What this machine's PIL writes today for the basis images (the bytes may differ from the recorded files)."""
    for name in sorted(set(CASES) - set(WRITTEN)):
        assert np.array_equal(jpeg.decode_jpegs_host([CASES[name][0]])[0], GEN.pil_pixels(CASES[name][0])), name


def test_the_cases_reach_the_model_where_they_aim():
    """The host model's own counters agree with the writer's counts: the long codes, ZRL and EOB were decoded, not skipped."""
    for name in WRITTEN:
        data, st = CASES[name]
        c = {}
        jpeg.decode_jpegs_host([data], c)
        assert c.get("long_codes", 0) == sum(sum(counts[jpeg.LOOK_BITS + 1:]) for counts in st["codes"].values()), name
        assert c.get("zrl", 0) == st["zrl"], name
        if not name.startswith("runs"):
            assert c.get("eob", 0) == st["eob"], name
    c = {}
    jpeg.decode_jpegs_host([CASES["magnitudes_gray_48x64"][0]], c)
    assert c["max_dc_category"] == 11


def test_one_image_under_four_restart_intervals_is_one_image():
    px = [GOLDEN["restart%d_420_19x30" % ri][1] for ri in (1, 2, 3, 7)]
    assert all(np.array_equal(p, px[0]) for p in px[1:])


@pytest.mark.parametrize("name", WRITTEN)
def test_parse_jpeg_reads_what_the_writer_wrote(name):
    data, st = CASES[name]
    hdr = jpeg.parse_jpeg(data)
    assert [(c["tq"], c["td"], c["ta"]) for c in hdr["components"]] == st["selectors"]
    assert hdr["restart_interval"] == st["restart"] and hdr["mcus"] == st["mcus"]
    assert [len(s) for s in hdr["segments"]] == [s["bytes"] for s in st["segments"]]
    assert jpeg._segment_mcus(hdr) == [(s["first"], s["mcus"]) for s in st["segments"]]
    assert sorted(hdr["quant"]) == sorted(st["quant"]) and all(hdr["quant"][k].tolist() == st["quant"][k] for k in st["quant"])
    for key in st["codes"]:  # every table the data was coded with is the table the parser hands on
        cls, th = ("dc", "ac").index(key[0]), key[1]
        bits, vals = hdr["huffman"][(cls, th)]
        assert (list(bits), list(vals)) == st[key[0]][th]
        codes = W.code_table((list(bits), list(vals)))
        assert set(st["symbols"][key]) <= set(codes)
        for length, (first, last) in st["first_last"][key].items():
            assert bits[length - 1] > 0
        look, maxcode, valoff, out = jpeg.huffman_table(bits, vals, dc=cls == 0)
        assert (np.diff(maxcode[1:17]) >= 0).all(), "maxcode must grow with the length"
        for sym in st["symbols"][key]:  # and the decoder's form of it finds every emitted symbol at its code
            code, length = codes[sym][:2]
            if length <= jpeg.LOOK_BITS:
                assert look[code << (jpeg.LOOK_BITS - length)] == (length << 8 | sym)
            else:
                assert look[code >> (length - jpeg.LOOK_BITS)] == 0 and maxcode[length - 1] < code >> 1 and code <= maxcode[length]
                assert out[(int(valoff[length]) + code) & 255] == sym


def test_parse_jpeg_takes_the_later_definition_and_every_layout():
    redefined = jpeg.parse_jpeg(CASES["layout_redefined_444_8x16"][0])
    merged = jpeg.parse_jpeg(CASES["layout_merged_444_8x16"][0])
    for key in ((0, 0), (0, 1), (1, 0), (1, 1)):
        assert (list(redefined["huffman"][key][0]), list(redefined["huffman"][key][1])) == \
            (list(merged["huffman"][key][0]), list(merged["huffman"][key][1])), key
    assert all(np.array_equal(redefined["quant"][k], merged["quant"][k]) for k in (0, 1))
    assert np.array_equal(GOLDEN["layout_redefined_444_8x16"][1], GOLDEN["layout_merged_444_8x16"][1])  # one image, two headers
    four = jpeg.parse_jpeg(CASES["layout_four_444_8x16"][0])
    assert sorted(four["quant"]) == [0, 1, 2, 3] and len({four["quant"][k].tobytes() for k in range(4)}) == 4
    assert len(jpeg.parse_jpeg(CASES["restart7_420_19x30"][0])["segments"]) == 1  # a DRI, and no marker needed


def test_the_batches_pack_to_three_table_sets_and_to_one():
    for prefix, sets, segs in (("sets", 3, 7), ("one", 1, 7)):
        hdrs = [jpeg.parse_jpeg(CASES["%s_%d" % (prefix, i)][0]) for i in range(3)]
        assert len({h["restart_interval"] for h in hdrs}) == 3
        assert jpeg.pack_jpegs(hdrs)[1:] == (segs, sets)
        got = jpeg.decode_jpegs_host([CASES["%s_%d" % (prefix, i)][0] for i in range(3)])
        for i in range(3):
            assert np.array_equal(got[i], GOLDEN["%s_%d" % (prefix, i)][1]), (prefix, i)


# ---- the status, by construction ----

_REASON = {GEN.BAD_CODE: "a code that is in no Huffman table", GEN.BAD_RUN: "a run past coefficient 63",
           GEN.OUT_OF_BITS: "the entropy-coded bytes ran out"}


def test_the_status_bits_are_the_library_s():
    assert (GEN.BAD_CODE, GEN.BAD_RUN, GEN.OUT_OF_BITS) == (jpeg.STATUS_BAD_CODE, jpeg.STATUS_BAD_RUN, jpeg.STATUS_OUT_OF_BITS)


@pytest.mark.parametrize("name", sorted(STATUS))
def test_host_model_gives_each_corrupt_stream_its_one_status(name):
    data, status = STATUS[name]
    if status == 0:
        assert np.array_equal(jpeg.decode_jpegs_host([data])[0], GEN.pil_pixels(data))
        return
    with pytest.raises(ValueError) as e:
        jpeg.decode_jpegs_host([data])
    assert str(e.value) == "decode_jpegs_host: image 0 did not decode: " + _REASON[status]


def test_short_is_exact_without_its_last_byte():
    exact, short = jpeg.parse_jpeg(STATUS["exact"][0]), jpeg.parse_jpeg(STATUS["short"][0])
    assert len(exact["segments"]) == 1 and short["segments"][0] == exact["segments"][0][:-1] and len(exact["segments"][0]) == 4
