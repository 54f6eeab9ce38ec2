"""Baseline JPEG decoding on the device: jpeg.decode_jpegs against PIL's recorded pixels
(tests/golden/jpeg_small.npz) bit for bit, batches with several and with one table set, restart segments, out= and a side
stream, the status contract on a file cut in half, the IDCT and the upsampling launches alone against the host model, and
the loaders and pipeline calls that take files: loadVideoFrames, loadFlowImages(device=), run_video(path)."""
import os

import numpy as np
import pytest
import torch

from test_jpeg_host import GEN, GOLDEN, _flow, _segment, _write_mjpeg_avi, video_jpegs

pytestmark = pytest.mark.gpu


def _named(prefix):
    """The fixture whose name starts with ``prefix`` -> (file bytes, PIL's pixels)."""
    return GOLDEN[[n for n in sorted(GOLDEN) if n.startswith(prefix)][0]]


def _decode(datas, **kw):
    from video_analytics_amd import jpeg
    out, status = jpeg.decode_jpegs(datas, "cuda", **kw)
    assert status.dtype == torch.int32 and tuple(status.shape) == (len(datas),) and status.is_cuda
    return out, status


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_decode_equals_pil_bit_for_bit(name):
    data, want = GOLDEN[name]
    out, status = _decode([data])
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1,) + want.shape and out.is_contiguous()
    got = out[0].cpu().numpy()
    assert np.array_equal(got, want), "%d values differ from the recorded pixels" % int((got != want).sum())
    assert int(status[0]) == 0
    assert np.array_equal(got, GEN.pil_pixels(data)), "differs from this machine's PIL"


@pytest.mark.parametrize("prefix,sets", [("batch", 3), ("shared", 1)])
def test_a_batch_with_several_table_sets_and_one_that_shares_them(prefix, sets):
    from video_analytics_amd import jpeg
    datas = [GOLDEN["%s_%d" % (prefix, i)][0] for i in range(5)]
    assert jpeg.pack_jpegs([jpeg.parse_jpeg(d) for d in datas])[2] == sets  # one set: the tables are staged in LDS
    out, status = _decode(datas)
    assert tuple(out.shape) == (5, 3, 24, 40) and not status.any()
    for i in range(5):
        assert np.array_equal(out[i].cpu().numpy(), GOLDEN["%s_%d" % (prefix, i)][1]), i


def test_more_segments_than_one_workgroup_holds():
    """70 images, 175 segments (every other image has four): three workgroups of the entropy launch, the last partly filled."""
    from video_analytics_amd import jpeg
    data, want = GOLDEN["restart3_420_37x53"]
    datas = [data, GOLDEN["plain_420_37x53"][0]] * 35
    assert jpeg.pack_jpegs([jpeg.parse_jpeg(d) for d in datas])[1] == 35 * 5
    out, status = _decode(datas)
    assert not status.any() and (out == torch.from_numpy(want).cuda()).all()


@pytest.mark.parametrize("name", sorted(n for n in GOLDEN if n.startswith("restart")))
def test_restart_segments_equal_the_image_decoded_as_one(name):
    from video_analytics_amd import jpeg
    plain = "plain_" + name.split("_", 1)[1]
    assert len(jpeg.parse_jpeg(GOLDEN[name][0])["segments"]) > 1 and len(jpeg.parse_jpeg(GOLDEN[plain][0])["segments"]) == 1
    several, one = _decode([GOLDEN[name][0]])[0], _decode([GOLDEN[plain][0]])[0]
    assert torch.equal(several, one) and np.array_equal(one[0].cpu().numpy(), GOLDEN[plain][1])


def test_out_and_a_side_stream():
    datas = [GOLDEN["shared_%d" % i][0] for i in range(3)]
    want = np.stack([GOLDEN["shared_%d" % i][1] for i in range(3)])
    flat = torch.full((want.size + 1,), 9, dtype=torch.uint8, device="cuda")
    out, _ = _decode(datas, out=flat[1:].view(want.shape))  # one byte past an aligned address: byte stores
    assert out.data_ptr() == flat.data_ptr() + 1 and np.array_equal(out.cpu().numpy(), want) and int(flat[0]) == 9
    gray, gwant = _named("gray_37x53")
    gflat = torch.full((gwant.size + 1,), 9, dtype=torch.uint8, device="cuda")
    gout, _ = _decode([gray], out=gflat[1:].view((1,) + gwant.shape))
    assert np.array_equal(gout[0].cpu().numpy(), gwant) and int(gflat[0]) == 9
    for bad in (torch.empty(want.shape, dtype=torch.uint8), torch.empty(want.shape, dtype=torch.int8, device="cuda"),
                torch.empty((3, 3, 24, 41), dtype=torch.uint8, device="cuda")[..., :40], torch.empty(want.shape[1:], dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError, match="out must be"):
            _decode(datas, out=bad)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out, status = _decode(datas, check=False)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and not status.any()


def test_status_names_the_image_whose_bytes_ran_out():
    from video_analytics_amd import jpeg
    data = GOLDEN["shared_1"][0]
    sos, sos_len = _segment(data, 0xDA)
    start = sos + 2 + sos_len
    cut = data[:start + (len(data) - 2 - start) // 2] + b"\xff\xd9"  # the middle image's entropy bytes, halved: it sits between
    datas = [GOLDEN["shared_0"][0], cut, GOLDEN["shared_2"][0]]      # the other two in the packed buffer
    out, status = _decode(datas, check=False)
    st = status.cpu().numpy()
    assert st[0] == 0 and st[2] == 0 and st[1] != 0 and st[1] & ~(jpeg.STATUS_BAD_CODE | jpeg.STATUS_BAD_RUN | jpeg.STATUS_OUT_OF_BITS) == 0
    for i in (0, 2):
        assert np.array_equal(out[i].cpu().numpy(), GOLDEN["shared_%d" % i][1]), i
    with pytest.raises(ValueError, match="image 1 did not decode"):
        _decode(datas)
    with pytest.raises(ValueError, match="image 1 did not decode"):
        jpeg.decode_jpegs_host(datas)


# ---- the launches alone ----

@pytest.mark.parametrize("w,h,ncomp,hs,vs", [(37, 19, 1, 1, 1), (40, 24, 1, 1, 1), (53, 37, 3, 2, 2), (30, 19, 3, 2, 1), (17, 8, 3, 1, 1)])
def test_idct_launch_equals_the_host_model(w, h, ncomp, hs, vs):
    """The out-of-domain test: blocks of +-1023 times the step 255 are coefficients no 8-bit samples give, and
    the sums wrap at 32 bits.  PIL is deliberately not the judge here: libjpeg's SIMD and C IDCTs give different pixels for
    such blocks (measured on the host: they differ from each other as much as from this model), so there is no libjpeg
    value to equal; the kernel is held to the host model's C "islow" arithmetic with 32-bit wrap and a clamp.  Inside the
    domain PIL judges: tests/test_jpeg_streams_gpu.py, the basis images and the magnitudes."""
    from video_analytics_amd import jpeg
    geo = jpeg.layout(w, h, ncomp, hs, vs)
    rs = np.random.RandomState(w * h)
    n = 2
    coef = np.zeros((n, geo["blocks"], 64), dtype=np.int16)
    dense = rs.rand(n, geo["blocks"]) < 0.5
    coef[dense] = rs.randint(-60, 61, size=(int(dense.sum()), 64))
    coef[~dense, 0] = rs.randint(-1024, 1024, size=int((~dense).sum()))            # DC only
    coef[0, 0] = np.where(rs.rand(64) < 0.5, -1023, 1023)                           # every coefficient at +-1023 ...
    coef[0, 1] = 1023
    coef[1, geo["blocks"] - 1] = -1023
    quant = rs.randint(1, 40, size=(ncomp, 64)).astype(np.uint16)
    quant[0, ::3] = 255                                                              # ... times the largest 8-bit step: the sums wrap
    got = jpeg.idct_planes(torch.from_numpy(coef).cuda(), torch.from_numpy(quant.view(np.int16)).cuda(), w, h, ncomp, hs, vs).cpu().numpy()
    for i in range(n):
        planes = []
        for c in range(ncomp):
            b0, bw, bh = geo["block_base"][c], geo["blocks_w"][c], geo["blocks_h"][c]
            planes.append(jpeg.blocks_to_plane(jpeg.idct_blocks(coef[i, b0:b0 + bw * bh], quant[c]), bw, bh))
        if ncomp == 1:
            assert np.array_equal(got[i], planes[0][:h, :w])
        else:
            assert np.array_equal(got[i], np.concatenate([p.reshape(-1) for p in planes]))


@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 1), (2, 2)])
@pytest.mark.parametrize("w,h", [(4, 4), (3, 3), (5, 9), (6, 10), (17, 9), (18, 4), (53, 37)])
def test_upsample_launch_equals_the_host_model(w, h, hs, vs):
    """Chroma widths 2, 3 and 9 and chroma heights 2 and 5: the first, last and clamped rows and columns; the padding holds
    noise of its own, which must never show."""
    from video_analytics_amd import jpeg
    geo = jpeg.layout(w, h, 3, hs, vs)
    rs = np.random.RandomState(100 * w + h + hs + vs)
    flat = rs.randint(0, 256, size=(2, geo["plane_bytes"])).astype(np.uint8)
    flat[1, geo["plane_off"][1]:] = rs.choice([0, 255], size=geo["plane_bytes"] - geo["plane_off"][1])  # saturated chroma: the clamps
    got = jpeg.upsample_planes(torch.from_numpy(flat).cuda(), w, h, hs, vs).cpu().numpy()
    for i in range(2):
        planes = [flat[i, off:off + 64 * bw * bh].reshape(8 * bh, 8 * bw)
                  for off, bw, bh in zip(geo["plane_off"], geo["blocks_w"], geo["blocks_h"])]
        assert np.array_equal(got[i], jpeg.planes_to_rgb(planes, w, h, hs, vs)), i


# ---- files in, tensors out ----

SCHEDULE = dict(epsilon=0.0, nscales=3, warps=1, iters=10)  # a shortened TV-L1 schedule


@pytest.fixture(scope="module")
def pipe():
    from video_analytics_amd import _ffi, pipeline
    p = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(**SCHEDULE))
    yield p
    p.close()


def _same(a, b):
    for key in ("scores_s", "scores_t", "scores", "pred", "desc_s", "desc_t", "logits_s_items", "logits_t_items"):
        assert torch.equal(a[key], b[key]), key
    assert a["starts"] == b["starts"] and a["frame_size"] == b["frame_size"]


def _keep(out):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def test_video_file_to_frames_and_through_run_video(tmp_path, pipe):
    from video_analytics_amd import utils
    path = str(tmp_path / "v.avi")
    _write_mjpeg_avi(path, video_jpegs(12, 32, 48))
    frames = utils.loadVideoFrames(path, "cuda")
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (12, 3, 32, 48)
    want = np.stack([np.asarray(f).transpose(2, 0, 1) for f in utils.iterVideoFrames(path)])
    assert np.array_equal(frames.cpu().numpy(), want)
    kw = dict(n_snippets=2, rescale=(224, 224))
    from_rgb = _keep(pipe.run_video(torch.from_numpy(want).cuda(), **kw))
    from_path = pipe.run_video(path, **kw)
    torch.cuda.synchronize()
    _same(from_path, from_rgb)
    gray_path = str(tmp_path / "g.avi")
    _write_mjpeg_avi(gray_path, [GOLDEN["checker"][0]] * 2)
    g = utils.loadVideoFrames(gray_path, "cuda")  # gray frames: three equal channels, as convert("RGB") gives them
    assert tuple(g.shape) == (2, 3, 16, 32) and np.array_equal(g[1].cpu().numpy(), np.stack([GOLDEN["checker"][1]] * 3))
    _write_mjpeg_avi(str(tmp_path / "x.avi"), video_jpegs(2, 32, 48), fourcc=b"XVID")
    with pytest.raises(ValueError, match="XVID"):
        pipe.run_video(str(tmp_path / "x.avi"), **kw)
    with pytest.raises(ValueError, match="without gray frames"):
        pipe.run_video(path, torch.zeros((12, 32, 48), dtype=torch.uint8, device="cuda"), n_snippets=2)


def test_evaluate_videos_and_train_videos_take_paths(tmp_path, pipe):
    import random
    from video_analytics_amd import _ffi, pipeline, utils, video
    paths = []
    for i in range(2):
        paths.append(str(tmp_path / ("v%d.avi" % i)))
        _write_mjpeg_avi(paths[-1], [GEN.encode(GEN.image(32, 48, 3, 700 + 20 * i + t), "RGB", 2, 95) for t in range(12)])
    frames = [utils.loadVideoFrames(p, "cuda") for p in paths]
    kw = dict(n_snippets=2, rescale=(224, 224))
    want = video.evaluateVideos(pipe, frames, [3, 7], **kw)
    got = video.evaluateVideos(pipe, [paths[0], (paths[1], None)], [3, 7], **kw)  # both spellings
    assert got[:3] == want[:3] and np.array_equal(got[3], want[3])
    # one training step from files equals the step from their decoded frames: fresh pipelines, the same draws
    outs = []
    for videos in ([paths[0], (paths[1], None)], frames):
        p = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(**SCHEDULE))
        out = p.train_videos(videos, torch.tensor([3, 7]), k=1, lr=1e-4, dropout_seed=5, rng=random.Random(11), rescale=(256, 340))
        torch.cuda.synchronize()
        outs.append(out)
        p.close()
    a, b = outs
    assert a["starts"] == b["starts"] and torch.equal(a["crops"], b["crops"]) and torch.equal(a["flow"], b["flow"])
    for key in ("stats_s", "stats_t", "desc_s", "desc_t"):
        assert torch.isfinite(a[key]).all() and torch.equal(a[key], b[key]), key
    with pytest.raises(ValueError, match="without gray frames"):
        pipe.train_videos([(paths[0], torch.zeros((12, 32, 48), dtype=torch.uint8, device="cuda"))], torch.tensor([3]), k=1)


def test_flow_and_frame_files_on_the_device(tmp_path, pipe):
    from video_analytics_amd import utils
    d = str(tmp_path / "flow")
    utils.saveFlowImages(_flow(11, 224, 224, seed=5), d, restartBlocks=28)  # a restart marker per block row: 28 lanes an image
    host = utils.loadFlowImages(d)
    dev = utils.loadFlowImages(d, device="cuda")
    assert dev.dtype == torch.uint8 and tuple(dev.shape) == (11, 2, 224, 224) and dev.is_contiguous()
    assert np.array_equal(dev.cpu().numpy(), host)
    assert np.array_equal(utils.loadFlowImages(d, first=3, count=4, device="cuda").cpu().numpy(), host[2:6])
    with pytest.raises(ValueError, match="missing"):
        utils.loadFlowImages(d, count=12, device="cuda")
    os.replace(os.path.join(d, utils.flowFileName("flow_y_", 11)), str(tmp_path / "kept.jpg"))
    with pytest.raises(ValueError, match="missing"):
        utils.loadFlowImages(d, device="cuda")
    with open(os.path.join(d, utils.flowFileName("flow_y_", 11)), "wb") as f:
        f.write(_named("gray_16x16")[0])
    with pytest.raises(ValueError, match="not the size"):
        utils.loadFlowImages(d, device="cuda")
    with open(os.path.join(d, utils.flowFileName("flow_y_", 11)), "wb") as f:
        f.write(GOLDEN["shared_0"][0])
    with pytest.raises(ValueError, match="single-channel"):
        utils.loadFlowImages(d, device="cuda")
    rgb = torch.from_numpy(np.random.RandomState(2).randint(0, 256, size=(12, 3, 224, 224)).astype(np.uint8)).cuda()
    uploaded = _keep(pipe.run_video(rgb, flow=torch.from_numpy(host).cuda(), n_snippets=2))
    decoded = pipe.run_video(rgb, flow=dev, n_snippets=2)
    torch.cuda.synchronize()
    _same(decoded, uploaded)
    # the numbered frame files of convertVideosToFrames
    paths = []
    for i, data in enumerate(video_jpegs(3, 24, 32)):
        paths.append(str(tmp_path / ("%d.jpg" % i)))
        with open(paths[-1], "wb") as f:
            f.write(data)
    got = utils.loadFrameImages(paths, "cuda")
    assert np.array_equal(got.cpu().numpy(), np.stack([GEN.pil_pixels(open(p, "rb").read()) for p in paths]))
    with pytest.raises(ValueError, match="missing"):
        utils.loadFrameImages(paths + [str(tmp_path / "none.jpg")], "cuda")
