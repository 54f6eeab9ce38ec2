"""Baseline JPEG encoding on the device: jpeg.encode_jpegs against the bytes PIL wrote
(tests/golden/jpeg_encode_small.npz) on every fixture and batch, also on a side stream and from an unaligned address; the
forward DCT launch alone against the host model; the entropy stage alone, on coefficient arrays no picture gives, against the
scan of tests/jpeg_writer.py (which imports nothing of the package); the status contract; and the round trips through the
files: saveFlowImagesDevice, loadFlowImages(device=), convertVideosToFrames(device=)."""
import os

import numpy as np
import pytest
import torch

import jpeg_writer
from test_jpeg_encode_host import CASES, annex_k, hand_built_blocks, scan_of
from test_jpeg_host import _flow, _write_mjpeg_avi, video_jpegs

pytestmark = pytest.mark.gpu


def _files(case):
    ends = np.cumsum(case["lens"])
    data = case["bytes"].tobytes()
    return [data[int(e - l):int(e)] for l, e in zip(case["lens"], ends)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_encode_equals_the_recorded_bytes(name):
    from video_analytics_amd import jpeg
    case = CASES[name]
    want = _files(case)
    kw = dict(quality=case["quality"], subsampling=case["subsampling"], restart_blocks=case["restart"])
    img = torch.from_numpy(case["img"]).cuda()
    got = jpeg.encode_jpegs(img, **kw)
    assert isinstance(got, list) and len(got) == len(want) and all(isinstance(g, bytes) for g in got)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "image %d: %d bytes for %d, first difference at %s" % (
            i, len(g), len(w), next((k for k in range(min(len(g), len(w))) if g[k] != w[k]), "the end"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert jpeg.encode_jpegs(img, check=False, **kw) == want
    torch.cuda.current_stream().wait_stream(side)
    raw = torch.empty(img.numel() + 1, dtype=torch.uint8, device="cuda")
    odd = raw[1:].view(img.shape)
    odd.copy_(img)
    assert odd.data_ptr() % 2 == 1 and odd.is_contiguous()
    assert jpeg.encode_jpegs(odd, **kw) == want


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("c4")))
def test_the_forward_dct_launch_alone_equals_the_host_model(name):
    from video_analytics_amd import jpeg
    case = CASES[name]
    hs, vs = {0: (1, 1), 1: (2, 1), 2: (2, 2)}[case["subsampling"]]
    quant = jpeg.quant_tables(case["quality"])
    got = jpeg.fdct_coefficients(torch.from_numpy(case["img"]).cuda(), quant, hs, vs).cpu().numpy()
    for i, img in enumerate(case["img"]):
        want = jpeg.encode_coefficients(img, quant, hs, vs)
        assert got[i].shape == want.shape and np.array_equal(got[i], want), \
            "image %d: blocks %s differ" % (i, np.flatnonzero((got[i] != want).any(axis=1))[:8])


# ---- the entropy stage on hand-built coefficients

@pytest.fixture(scope="module")
def hand_built():
    blocks = hand_built_blocks()
    w = 8 * 16
    rows = -(-len(blocks) // 16)
    grid = np.zeros((16 * rows, 64), dtype=np.int16)
    grid[:len(blocks)] = blocks
    return grid, w, 8 * rows


@pytest.mark.parametrize("restart", [0, 1])
def test_the_entropy_stage_alone_equals_the_independent_writer(hand_built, restart):
    from video_analytics_amd import jpeg
    grid, w, h = hand_built
    dc, ac = annex_k()
    data, stats = jpeg_writer.write_jpeg(w, h, [list(grid)], quant={0: np.ones(64)}, dc={0: dc[0]}, ac={0: ac[0]}, restart=restart)
    # the arrays hold what they are there for, counted by the writer
    assert stats["long_code_offsets"] == set(range(32)), sorted(stats["long_code_offsets"])
    assert stats["zrl"] >= 1 + 1 + 1 + 2 + 3 + 3 and stats["end63"] >= 14 and stats["stuffed"] > 20
    assert max(k for k, n in enumerate(stats["codes"][("dc", 0)]) if n) == 9  # the 9-bit code of DC category 11
    assert {0xFA, 0x01, 0x0A, 0xF0, 0x00} <= stats["symbols"][("ac", 0)] and {0, 11} <= stats["symbols"][("dc", 0)]
    if restart:
        ends = [(s["padding"], s["ends_stuffed"]) for s in stats["segments"]]
        assert (0, True) in ends, "no interval ends with a data FF"
        assert any(p >= 6 and e for p, e in ends), "no interval ends with an FF the fill bits make"
        assert len(stats["segments"]) == len(grid)
    scans, status = jpeg.entropy_encode(torch.from_numpy(grid[None]).cuda(), w, h, 1, 1, 1, restart)
    want = scan_of(data)
    assert b"\xff\xff\x00" not in want and want.count(b"\xff\x00\xff\x00") > 0  # consecutive FF bytes, each stuffed
    assert not status.any() and len(scans) == 1
    assert scans[0] == want, "%d bytes for %d, first difference at %s" % (
        len(scans[0]), len(want), next((k for k in range(min(len(scans[0]), len(want))) if scans[0][k] != want[k]), "the end"))


@pytest.mark.parametrize("sampling,restart", [((2, 2), 0), ((2, 2), 2), ((2, 1), 1), ((1, 1), 3)])
def test_the_entropy_stage_walks_colour_mcus_in_order(sampling, restart):
    """Random sparse coefficients on a colour grid: luma blocks of an MCU in raster order, then Cb, then Cr, with the
    chroma tables, three images in one call."""
    from video_analytics_amd import jpeg
    w, h = 40, 24
    hs, vs = sampling
    geo = jpeg.layout(w, h, 3, hs, vs)
    rng = np.random.default_rng(hs * 10 + vs + restart)
    coef = np.where(rng.random((3, geo["blocks"], 64)) < 0.15, rng.integers(-300, 301, (3, geo["blocks"], 64)), 0).astype(np.int16)
    dc, ac = annex_k()
    scans, status = jpeg.entropy_encode(torch.from_numpy(coef).cuda(), w, h, 3, hs, vs, restart)
    assert not status.any()
    for i in range(3):
        comps = [list(coef[i, b:b + bw * bh]) for b, bw, bh in zip(geo["block_base"], geo["blocks_w"], geo["blocks_h"])]
        data, _ = jpeg_writer.write_jpeg(w, h, comps, quant={0: np.ones(64), 1: np.ones(64)}, dc=dc, ac=ac, sampling=sampling,
                                         restart=restart)
        assert scans[i] == scan_of(data), i


def test_a_coefficient_outside_the_categories_sets_the_status_of_its_image_alone():
    from video_analytics_amd import jpeg
    w, h = 24, 16
    rng = np.random.default_rng(3)
    coef = rng.integers(-20, 21, (4, 6, 64)).astype(np.int16)
    clean, status = jpeg.entropy_encode(torch.from_numpy(coef).cuda(), w, h, 1, 1, 1, 2)
    assert not status.any()
    bad = coef.copy()
    bad[1, 2, 9] = 2048      # an AC value of 12 bits
    bad[3, 4, 0] = 4000      # a DC difference of 12 bits
    scans, status = jpeg.entropy_encode(torch.from_numpy(bad).cuda(), w, h, 1, 1, 1, 2, check=False)
    assert status.tolist() == [0, jpeg.ENC_STATUS_RANGE, 0, jpeg.ENC_STATUS_RANGE]
    assert scans[0] == clean[0] and scans[2] == clean[2]
    with pytest.raises(ValueError, match="image 1 did not encode.*outside the baseline categories"):
        jpeg.entropy_encode(torch.from_numpy(bad).cuda(), w, h, 1, 1, 1, 2)
    # an output buffer that ends inside the third image: that one and the one behind it are reported, none is cut short
    room = len(clean[0]) + len(clean[1]) + len(clean[2]) - 1
    scans, status = jpeg.entropy_encode(torch.from_numpy(coef).cuda(), w, h, 1, 1, 1, 2, check=False, out_bytes=room)
    assert status.tolist() == [0, 0, jpeg.ENC_STATUS_FIT, jpeg.ENC_STATUS_FIT] and scans[:2] == clean[:2] and scans[2:] == [b"", b""]


# ---- through the files

def test_flow_images_round_trip_on_the_device(tmp_path):
    from PIL import Image
    from video_analytics_amd import utils
    fl = _flow(3, 24, 40)
    store = utils.flowToImages(fl)
    host, dev_u8, dev_f32 = (str(tmp_path / d) for d in ("host", "u8", "f32"))
    assert utils.saveFlowImages(fl, host, restartBlocks=5) == 6
    assert utils.saveFlowImagesDevice(torch.from_numpy(store).cuda(), dev_u8, "cuda", restartBlocks=5) == 6
    assert utils.saveFlowImagesDevice(torch.from_numpy(fl).cuda(), dev_f32, "cuda", restartBlocks=5) == 6
    names = sorted(os.listdir(host))
    assert names == sorted(os.listdir(dev_u8)) == sorted(os.listdir(dev_f32)) and len(names) == 6
    for name in names:
        want = open(os.path.join(host, name), "rb").read()
        assert open(os.path.join(dev_u8, name), "rb").read() == want, name
        assert open(os.path.join(dev_f32, name), "rb").read() == want, name
    back = utils.loadFlowImages(dev_u8, device="cuda")
    want = np.stack([np.stack([np.asarray(Image.open(os.path.join(dev_u8, utils.flowFileName(p, k)))) for p in ("flow_x_", "flow_y_")])
                     for k in (1, 2, 3)])
    assert tuple(back.shape) == (3, 2, 24, 40) and np.array_equal(back.cpu().numpy(), want)


def test_convert_videos_to_frames_writes_the_host_path_s_files(tmp_path):
    from video_analytics_amd import utils
    root = tmp_path / "videos" / "Cat"
    root.mkdir(parents=True)
    _write_mjpeg_avi(str(root / "v_Cat_g01_c01.avi"), video_jpegs(6, 24, 40))
    (tmp_path / "list.txt").write_text("Cat/v_Cat_g01_c01.avi 1\n")
    for out, device in (("host", None), ("dev", "cuda")):
        utils.convertVideosToFrames(str(tmp_path / "videos"), str(tmp_path / out), str(tmp_path / "list.txt"), sampleRate=2,
                                    device=device)
    host, dev = (str(tmp_path / d / "Cat" / "v_Cat_g01_c01") for d in ("host", "dev"))
    assert sorted(os.listdir(host)) == sorted(os.listdir(dev)) == ["0.jpg", "1.jpg", "2.jpg"]
    for name in os.listdir(host):
        assert open(os.path.join(dev, name), "rb").read() == open(os.path.join(host, name), "rb").read(), name
