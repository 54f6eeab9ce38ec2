"""The host model of the baseline JPEG encoder, without a GPU: jpeg.quant_tables against the DQT of PIL's
files, jpeg.encode_jpegs_host against the recorded bytes (tests/golden/jpeg_encode_small.npz) and this machine's PIL, the
project's own decoder on every file written, the ValueErrors that come before the device, and the utils that write files
with their default arguments."""
import inspect
import io
import json
import os
import struct

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_writer
from test_jpeg_host import _flow, _write_mjpeg_avi, video_jpegs
from video_analytics_amd import jpeg, utils

HERE = os.path.dirname(os.path.abspath(__file__))


def _load():
    z = np.load(os.path.join(HERE, "golden", "jpeg_encode_small.npz"))
    out = {}
    for k, c in enumerate(json.loads(str(z["cases"]))):
        out[c["name"]] = dict(c, img=z["img_%d" % k], bytes=z["bytes_%d" % k], lens=z["lens_%d" % k])
    return out


CASES = _load()


def files_of(case):
    ends = np.cumsum(case["lens"])
    data = case["bytes"].tobytes()
    return [data[int(e - l):int(e)] for l, e in zip(case["lens"], ends)]


def segments_of(data):
    """The header segments of a file in front of its scan -> [(marker, payload)], and the offset of the scan."""
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        m, (n,) = data[p + 1], struct.unpack(">H", data[p + 2:p + 4])
        out.append((m, data[p + 4:p + 2 + n]))
        p += 2 + n
        if m == 0xDA:
            return out, p


def scan_of(data):
    """The entropy-coded bytes of a file: behind SOS, in front of EOI."""
    assert data[-2:] == b"\xff\xd9"
    return data[segments_of(data)[1]:-2]


def annex_k():
    """The Huffman specs PIL wrote into a recorded colour file -> (dc {0, 1}, ac {0, 1}) as tests/jpeg_writer.py takes them:
    Annex K's tables, read from the fixture and not from the package."""
    dc, ac = {}, {}
    for m, s in segments_of(files_of(CASES["c420_16x16_q1"])[0])[0]:
        if m == 0xC4:
            bits = list(s[1:17])
            (dc if s[0] >> 4 == 0 else ac)[s[0] & 15] = (bits, list(s[17:17 + sum(bits)]))
    assert sorted(dc) == sorted(ac) == [0, 1]
    return dc, ac


def pil_bytes(img, quality, subsampling, restart):
    f = io.BytesIO()
    im = Image.fromarray(img if img.ndim == 2 else np.ascontiguousarray(img.transpose(1, 2, 0)))
    im.save(f, "JPEG", quality=quality, subsampling=subsampling, **({} if restart is None else {"restart_marker_blocks": restart}))
    return f.getvalue()


def pil_pixels(data):
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a if a.ndim == 2 else a.transpose(2, 0, 1)


def _dqt(data):
    out = {}
    for m, s in segments_of(data)[0]:
        if m == 0xDB:
            t = np.zeros(64, dtype=np.uint16)
            t[jpeg.ZIGZAG] = np.frombuffer(s[1:65], dtype=np.uint8)
            out[s[0]] = t
    return out


@pytest.mark.parametrize("quality", [1, 20, 30, 50, 75, 95, 100])
def test_quant_tables_are_those_of_pil_s_files(quality):
    luma, chroma = jpeg.quant_tables(quality)
    assert luma.dtype == np.uint16 and luma.shape == (64,) and chroma.shape == (64,)
    got = _dqt(pil_bytes(np.zeros((3, 8, 8), dtype=np.uint8), quality, 2, None))
    assert np.array_equal(got[0], luma) and np.array_equal(got[1], chroma)
    for case in CASES.values():  # and of the recorded files
        if case["quality"] == quality:
            rec = _dqt(files_of(case)[0])
            assert np.array_equal(rec[0], luma) and (1 not in rec or np.array_equal(rec[1], chroma))
    if quality == 1:
        assert luma.max() == 255 and chroma.min() == 255
    if quality == 100:
        assert luma.max() == 1 and chroma.max() == 1


def test_quant_tables_refuse_other_qualities():
    for q in (0, 101, -1, 50.0, None, True):
        with pytest.raises(ValueError, match="quality"):
            jpeg.quant_tables(q)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_host_model_writes_the_recorded_bytes_and_pil_s(name):
    case = CASES[name]
    want = files_of(case)
    got = jpeg.encode_jpegs_host(case["img"], case["quality"], case["subsampling"], case["restart"])
    assert got == want
    for img, data in list(zip(case["img"], want))[:5]:
        assert pil_bytes(img, case["quality"], case["subsampling"], case["restart"]) == data, "this machine's PIL writes other bytes"


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_project_s_decoder_reads_every_file_as_pil_does(name):
    case = CASES[name]
    datas = files_of(case)[:5]
    hdr = jpeg.parse_jpeg(datas[0])
    assert (hdr["width"], hdr["height"]) == case["img"].shape[:0:-1][:2] and hdr["restart_interval"] == (case["restart"] or 0)
    assert np.array_equal(jpeg.decode_jpegs_host(datas), np.stack([pil_pixels(d) for d in datas]))


def test_the_header_is_the_one_pil_writes():
    data = files_of(CASES["c420_53x37_r1"])[0]
    segs, at = segments_of(data)
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert [len(s) + 2 for _, s in segs] == [16, 67, 67, 17, 31, 181, 31, 181, 4, 12]
    assert [s[0] for m, s in segs if m == 0xC4] == [0x00, 0x10, 0x01, 0x11]
    quant = jpeg.quant_tables(95)
    assert jpeg.jpeg_header(37, 53, 3, 2, 2, quant, 1) == data[:at]
    gray = files_of(CASES["gray_17x8_r1000"])[0]
    segs, at = segments_of(gray)
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xDD, 0xDA] and b"\xff\xd0" not in gray[at:]  # DRI, no marker
    assert jpeg.jpeg_header(8, 17, 1, 1, 1, jpeg.quant_tables(75), 1000) == gray[:at]


def test_the_counters_tell_what_an_encode_met():
    c = {}
    case = CASES["gray_47x33_noise_q100_r3"]
    jpeg.encode_jpegs_host(case["img"], 100, 0, 3, counters=c)
    assert c["segments"] == 10 and len(c["padding"]) == 10 and c["stuffed"] > 0 and c["no_eob"] > 0 and "zrl" not in c
    c = {}
    case = CASES["c420_40x24_ramp_q30"]
    jpeg.encode_jpegs_host(case["img"], 30, 2, None, counters=c)
    assert c["zrl"] > 0 and c["zero_blocks"] > 0 and c["eob"] > 0 and c["dummy_blocks"] == 4 * 6 - 3 * 5 and c["segments"] == 1


def test_coefficients_of_a_dummy_block_repeat_the_dc_in_front():
    img = CASES["c420_53x37_q95"]["img"][0]
    coef = jpeg.encode_coefficients(img, jpeg.quant_tables(95), 2, 2)
    geo = jpeg.layout(37, 53, 3, 2, 2)
    luma = coef[:geo["blocks_w"][0] * geo["blocks_h"][0]].reshape(geo["blocks_h"][0], geo["blocks_w"][0], 64)
    assert luma.shape[:2] == (8, 6)
    assert not luma[:, 5, 1:].any() and not luma[7, :, 1:].any()
    assert np.array_equal(luma[:7, 5, 0], luma[:7, 4, 0])                       # the right column: the block to its left
    assert luma[7, 0, 0] == luma[6, 1, 0] and luma[7, 1, 0] == luma[7, 0, 0]    # the bottom row: the block before it in the MCU
    assert luma[7, 4, 0] == luma[6, 4, 0] and luma[7, 5, 0] == luma[6, 4, 0]    # the corner MCU: a chain of three dummies


def block_of(**at):
    """A block with the given values at zigzag positions: ``block_of(z0=5, z63=-1)``."""
    b = np.zeros(64, dtype=np.int16)
    for k, v in at.items():
        b[jpeg_writer.ZIGZAG[int(k[1:])]] = v
    return b


def hand_built_blocks():
    """-> (blocks [NB, 64], the reason each group is there); gray, so raster order is scan order."""
    blocks = []
    # AC +-1, +-1023 and every category 1..10 in one block
    blocks.append(block_of(z1=1, z2=-1, z3=1023, z4=-1023, **{"z%d" % (5 + s): (1 << s) - 1 for s in range(1, 11)},
                         **{"z%d" % (20 + s): -(1 << (s - 1)) for s in range(1, 11)}))
    # DC differences of +-2047 and 0
    for dc in (0, 1023, -1024, 1023, 1023, 0, 0):
        blocks.append(block_of(z0=dc))
    # zero runs of 15, 16, 17, 31, 32, 48 and 62 in front of a value
    for run in (15, 16, 17, 31, 32, 48, 62):
        blocks.append(block_of(z0=3, **{"z%d" % (run + 1): -5}))
    blocks.append(block_of(z63=7))                                            # coefficient 63 alone
    blocks.append(np.r_[0, np.arange(1, 64) % 9 + 1].astype(np.int16))      # 63 non-zero values
    # long codes at every bit phase of a 32-bit word: (run 15, size 10) is a 16-bit code with a 10-bit value; the DC category
    # in front shifts the phase from block to block
    rng = np.random.default_rng(7)
    for k in range(96):
        b = block_of(z0=int(rng.integers(-1000, 1000)), z16=1023, z32=-1023, z48=1023)
        for z in rng.choice(np.arange(1, 16), size=int(rng.integers(0, 6)), replace=False):
            b[jpeg_writer.ZIGZAG[int(z)]] = int(rng.integers(-40, 41))
        blocks.append(b)
    # runs of FF: 1023 is ten 1-bits and the long codes begin with nine or more, so (run 15, size 10) three times over gives
    # FF FF; a block that ends with coefficient 63 = 1023 ends its interval in 1-bits at a phase the DC category in front sets
    dc = 0
    for cat in range(12):
        dc += ((1 << cat) - 1) * (1 if cat % 2 else -1)  # a difference of category `cat` to the block before
        blocks.append(block_of(z0=dc, z63=1023))
    return np.stack(blocks)


@pytest.mark.parametrize("restart", [0, 1, 5])
def test_the_host_entropy_coder_equals_the_independent_writer(restart):
    """The arrays the device's entropy stage is held to (tests/test_jpeg_encode_gpu.py), here for the host model."""
    blocks = hand_built_blocks()
    rows = -(-len(blocks) // 16)
    grid = np.zeros((16 * rows, 64), dtype=np.int16)
    grid[:len(blocks)] = blocks
    dc, ac = annex_k()
    data, _ = jpeg_writer.write_jpeg(128, 8 * rows, [list(grid)], quant={0: np.ones(64)}, dc={0: dc[0]}, ac={0: ac[0]}, restart=restart)
    assert jpeg.entropy_encode_host(grid, 128, 8 * rows, 1, 1, 1, restart) == scan_of(data)
    bad = grid.copy()
    bad[3, 9] = 2048
    with pytest.raises(ValueError, match="outside the baseline categories"):
        jpeg.entropy_encode_host(bad, 128, 8 * rows, 1, 1, 1, restart)


def test_encode_jpegs_refuses_before_the_device():
    """Everything ``encode_jpegs`` refuses is refused without a GPU in the machine."""
    good = torch.zeros((2, 3, 16, 16), dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA"):
        jpeg.encode_jpegs(good)
    with pytest.raises(ValueError, match="uint8"):
        jpeg.encode_jpegs(good.float())
    with pytest.raises(ValueError, match="uint8"):
        jpeg.encode_jpegs(good.numpy())
    for shape in ((16, 16), (2, 4, 16, 16), (1, 2, 3, 16, 16), (0, 16, 16)):
        with pytest.raises(ValueError, match="n,h,w"):
            jpeg.encode_jpegs(torch.zeros(shape, dtype=torch.uint8))
    for shape in ((1, 2, 16), (1, 16, 2), (1, 3, 2, 16), (1, 65536, 3)):
        with pytest.raises(ValueError, match="outside the sizes"):
            jpeg.encode_jpegs(torch.zeros(shape, dtype=torch.uint8))
    for q in (0, 101, 75.5):
        with pytest.raises(ValueError, match="quality"):
            jpeg.encode_jpegs(good, quality=q)
    for s in (3, -1, "4:2:0", None):
        with pytest.raises(ValueError, match="subsampling"):
            jpeg.encode_jpegs(good, subsampling=s)
    for r in (65536, -1, 2.5):
        with pytest.raises(ValueError, match="65535 MCUs"):
            jpeg.encode_jpegs(good, restart_blocks=r)
    with pytest.raises(ValueError, match="contiguous"):
        jpeg.encode_jpegs(good[:, :, :, ::2])
    with pytest.raises(TypeError):
        jpeg.encode_jpegs(good, optimize=True)
    for bad, match in ((dict(quality=0), "quality"), (dict(subsampling=3), "subsampling"), (dict(restart_blocks=70000), "65535")):
        with pytest.raises(ValueError, match=match):
            jpeg.encode_jpegs_host(good.numpy(), **bad)
    with pytest.raises(ValueError, match="uint8"):
        jpeg.encode_jpegs_host(good.numpy().astype(np.int16))
    with pytest.raises(ValueError, match="uint8 tensor"):
        utils.saveFrameImages(good.numpy(), "unused")
    with pytest.raises(ValueError, match="float32 or uint8"):
        utils.saveFlowImagesDevice(np.zeros((2, 2, 8, 8), dtype=np.float64), "unused", "cuda")


def test_the_bound_of_a_scan_holds_the_worst_block():
    """63 values of the longest code and the longest value, a DC difference of 11 bits, all of it FF: the bound is reached by
    no picture, and it is what sizes the device buffers."""
    assert jpeg.BLOCK_BITS == 9 + 11 + 63 * (16 + 10)
    assert jpeg.scan_bound(8, 8, 1, 1, 1) == 2 * (-(-jpeg.BLOCK_BITS // 8) + 1)
    assert jpeg.scan_bound(16, 8, 1, 1, 1, restart=1) == 2 * (-(-2 * jpeg.BLOCK_BITS // 8) + 2) + 2
    for case in CASES.values():
        n, w, h, nc, hs, vs, restart, _ = jpeg._encode_args("t", case["img"].shape, case["quality"], case["subsampling"], case["restart"])
        assert max(len(scan_of(f)) for f in files_of(case)) <= jpeg.scan_bound(w, h, nc, hs, vs, restart)


def test_the_utils_write_what_they_wrote_before(tmp_path):
    p = inspect.signature(utils.convertVideosToFrames).parameters
    assert list(p) == ["rootDir", "saveDir", "videoListLoc", "sampleRate", "mode", "device"] and p["device"].default is None
    p = inspect.signature(jpeg.encode_jpegs).parameters
    assert list(p) == ["images", "quality", "subsampling", "restart_blocks", "check"]
    assert [p[k].default for k in p][1:] == [95, 2, None, True]
    fl = _flow(2, 24, 40)
    assert utils.saveFlowImages(fl, str(tmp_path / "flow")) == 4
    q = utils.flowToImages(fl)
    for k in range(2):
        for prefix, plane in (("flow_x_", 0), ("flow_y_", 1)):
            got = (tmp_path / "flow" / utils.flowFileName(prefix, k + 1)).read_bytes()
            assert got == pil_bytes(q[k, plane], 95, -1, None) == jpeg.encode_jpegs_host(q[k, plane][None])[0]
    root = tmp_path / "videos" / "Cat"
    root.mkdir(parents=True)
    jpegs = video_jpegs(6, 24, 40)
    _write_mjpeg_avi(str(root / "v_Cat_g01_c01.avi"), jpegs)
    (tmp_path / "list.txt").write_text("Cat/v_Cat_g01_c01.avi 1\n")
    utils.convertVideosToFrames(str(tmp_path / "videos"), str(tmp_path / "frames"), str(tmp_path / "list.txt"), sampleRate=2)
    out = tmp_path / "frames" / "Cat" / "v_Cat_g01_c01"
    assert sorted(os.listdir(str(out))) == ["0.jpg", "1.jpg", "2.jpg"]
    for i in range(3):
        frame = Image.open(io.BytesIO(jpegs[2 * i])).convert("RGB")
        buf = io.BytesIO()
        frame.save(buf, "JPEG", quality=95)
        data = (out / ("%d.jpg" % i)).read_bytes()
        assert data == buf.getvalue()
        # and what the device path writes for these frames, stated by the host model: the same file
        assert data == jpeg.encode_jpegs_host(np.asarray(frame).transpose(2, 0, 1)[None], 95, 2)[0]
