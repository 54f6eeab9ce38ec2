"""The device crop and flip (va_flow_to_stack_crop, va_crop_images_u8) against numpy gathers of the
oracle's S9 volume, against the host transforms of the reference's data path (Sheet03/utils.py:137-151 applied per
image, Sheet03/temporalModel.py:86), and 320x240 clips end to end through TwoStreamPipeline."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _gather(planes, crops, size=224):
    """numpy reference of S10: plane i cropped by row i of crops (flip mirrors the columns)."""
    out = []
    for p, (top, left, flip) in zip(planes, crops.tolist()):
        win = p[..., top:top + size, left:left + size]
        out.append(win[..., ::-1] if flip else win)
    return np.ascontiguousarray(np.stack(out))


def _extremes(crops, h, w):
    """Overwrite the first rows with hand-written crops: offsets 0 and maximum, odd lefts, flip on and off."""
    rows = [(0, 0, 0), (h - 224, w - 224, 1), (0, w - 224, 0), (h - 224, 0, 1), (5, 33, 1), (h - 224, 1, 0), (1, 97 % (w - 223), 1)]
    crops = crops.clone()
    for i, r in enumerate(rows[:crops.shape[0]]):
        crops[i] = torch.tensor(r, dtype=torch.int32)
    return crops


def test_flow_crop_equals_s9_then_gather(oracle_tvl1):
    from video_analytics_amd import augment
    from video_analytics_amd import flow as vflow
    rs = np.random.RandomState(0)
    fl = (rs.standard_normal((7, 2, 241, 321)) * 12.0).astype(np.float32)  # sigma 12 px: both clamps at +-20 are hit
    full = oracle_tvl1.flow_to_stack(fl)
    assert (full == full.min()).any() and full.min() < full.max()
    random.seed(0)
    crops = _extremes(augment.draw_flow_crops(7, 1, 241, 321), 241, 321)
    got = vflow.crop_flow_to_stack(torch.from_numpy(fl).cuda(), crops).cpu().numpy()
    assert got.shape == (14, 224, 224)
    assert np.array_equal(got, _gather(full, crops))


def test_flow_crop_of_the_whole_frame_equals_flow_to_stack():
    from video_analytics_amd import flow as vflow
    g = torch.Generator().manual_seed(1)
    fl = ((torch.rand(5, 2, 224, 224, generator=g) - 0.5) * 60.0).cuda()
    none = torch.zeros(10, 3, dtype=torch.int32)
    assert torch.equal(vflow.crop_flow_to_stack(fl, none), vflow.flow_to_stack(fl))
    small = fl[:, :, :100, :100].contiguous()
    assert torch.equal(vflow.crop_flow_to_stack(small, none, size=100), vflow.flow_to_stack(small))


def test_flow_crop_full_batch_native_size(oracle_tvl1):
    """B = 32 clips, L = 10: 640 channels of 320x240 flow, each with its own crop."""
    from video_analytics_amd import augment
    from video_analytics_amd import flow as vflow
    rs = np.random.RandomState(2)
    fl = (rs.standard_normal((320, 2, 240, 320)) * 12.0).astype(np.float32)
    random.seed(2)
    crops = _extremes(augment.draw_flow_crops(32, 10, 240, 320), 240, 320)
    got = vflow.crop_flow_to_stack(torch.from_numpy(fl).cuda(), crops).view(32, 20, 224, 224).cpu().numpy()
    ref = _gather(oracle_tvl1.flow_to_stack(fl), crops).reshape(32, 20, 224, 224)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("n,c,h,w", [(5, 3, 241, 321), (4, 3, 240, 320), (3, 1, 225, 300), (2, 20, 224, 224)])
def test_image_crop_equals_numpy_slicing(n, c, h, w):
    from video_analytics_amd import augment
    rs = np.random.RandomState(n * 100 + c)
    x = rs.randint(0, 256, size=(n, c, h, w)).astype(np.uint8)
    random.seed(n)
    crops = _extremes(augment.draw_image_crops(n, h, w), h, w)
    ref = _gather(x, crops)
    got = augment.crop_images(torch.from_numpy(x).cuda(), crops).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, ref)
    nhwc = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda()
    assert np.array_equal(augment.crop_images(nhwc, crops, layout="NHWC").cpu().numpy(), ref)


def test_device_path_replays_the_host_dataset():
    """Seeded host transforms (getTransforms() on every flow image in interleave order, on the RGB frames) and the
    seeded device path give the same [20,224,224] volumes and the same normalised RGB crops, bit for bit."""
    from video_analytics_amd import _ffi, augment, synth, temporalModel, utils
    from video_analytics_amd import flow as vflow
    from video_analytics_amd.parameters import NORM_MEANS_TF, NORM_STDS_TF
    B, L = 2, 10
    rgb, gray, _ = synth.synth_clips(B, seed=3, H=240, W=320)
    params = _ffi.default_tvl1_params(epsilon=0.0, iters=10, warps=1)
    fl = vflow.tvl1_flow(gray.cuda(), params)
    q = utils.flowToImages(fl)  # [B*L,2,240,320] u8: the flow JPEGs' pixels
    tf = utils.getTransforms()
    random.seed(42)
    host = torch.stack([torch.stack([tf(q[b * L + k, a]) for k in range(L) for a in (0, 1)]).squeeze(1) for b in range(B)])
    host_state = random.getstate()
    random.seed(42)
    crops = augment.draw_flow_crops(B, L, 240, 320)
    assert random.getstate() == host_state
    dev = vflow.crop_flow_to_stack(fl, crops).view(B, 2 * L, 224, 224).cpu()
    assert host.shape == dev.shape and torch.equal(host, dev)
    vol = temporalModel.flowVolumesFromFrames(gray.cuda(), tvl1_params=params, crops=crops)
    assert tuple(vol.shape) == (B, 2 * L, 224, 224) and torch.equal(vol.cpu(), dev)

    random.seed(43)
    host_rgb = torch.stack([tf(rgb[b].permute(1, 2, 0).numpy()) for b in range(B)])
    random.seed(43)
    rcrops = augment.draw_image_crops(B, 240, 320)
    norm = utils.Compose([utils.ToTensor(), utils.Normalize(NORM_MEANS_TF, NORM_STDS_TF)])
    for layout, x in (("NCHW", rgb), ("NHWC", rgb.permute(0, 2, 3, 1).contiguous())):
        u8 = augment.crop_images(x.cuda(), rcrops, layout=layout).cpu()
        dev_rgb = torch.stack([norm(u8[b].permute(1, 2, 0).numpy()) for b in range(B)])
        assert torch.equal(host_rgb, dev_rgb), layout


def test_native_resolution_pipeline(oracle_tvl1):
    from oracle import vgg_oracle
    from video_analytics_amd import _ffi, augment, pipeline, synth, utils
    from video_analytics_amd import flow as vflow
    from video_analytics_amd.parameters import NORM_MEANS_TF, NORM_STDS_TF
    n, L, H, W = 3, 10, 240, 320
    rgb, gray, _ = synth.synth_clips(n, seed=17, H=H, W=W)
    kw = dict(epsilon=0.0, iters=28, warps=2)  # 5 scales: 320, 256, 205, 164, 131 columns
    fl_ref = oracle_tvl1.tvl1_flow(gray.numpy(), oracle_tvl1.default_params(**kw), nthreads=8)
    fl = vflow.tvl1_flow(gray.cuda(), _ffi.default_tvl1_params(**kw)).cpu().numpy()
    assert np.array_equal(fl, fl_ref), "320x240 flow differs from the oracle: max abs diff %g" % np.abs(fl - fl_ref).max()

    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(**kw))
    with pytest.raises(ValueError, match="crops="):
        pipe.run_batch(rgb.cuda(), gray.cuda())
    random.seed(5)
    crops = augment.draw_clip_crops(n, L, (H, W), (H, W))
    out = pipe.run_batch(rgb.cuda(), gray.cuda(), crops=crops)

    # host-built crops of the same draws: numpy slicing + the reference's ToTensor/Normalize, the oracle's S9 volume
    norm = utils.Compose([utils.ToTensor(), utils.Normalize(NORM_MEANS_TF, NORM_STDS_TF)])
    xs = torch.stack([norm(p.transpose(1, 2, 0)) for p in _gather(rgb.numpy(), crops[0])])
    xt = torch.from_numpy(_gather(oracle_tvl1.flow_to_stack(fl_ref), crops[1]).reshape(n, 2 * L, 224, 224))
    _, ds, ls = pipe.spatial.forward(xs.cuda())
    _, dt, lt = pipe.temporal.forward(xt.cuda())
    torch.cuda.synchronize()
    for got, ref in ((out["logits_s"], ls), (out["desc_s"], ds), (out["logits_t"], lt), (out["desc_t"], dt)):
        assert torch.equal(got, ref)

    ws = synth.synth_vgg16_weights(c_in=3, seed=1)
    wt = synth.synth_vgg16_weights(c_in=20, seed=2)
    wt["conv_w"][0] = vgg_oracle.copy_first_layer(wt["conv_w"][0], 20)
    _, _, ls_ref = vgg_oracle.forward(xs, ws["conv_w"], ws["conv_b"], ws["fc_w"], ws["fc_b"])
    _, _, lt_ref = vgg_oracle.forward(xt, wt["conv_w"], wt["conv_b"], wt["fc_w"], wt["fc_b"])
    assert float((out["logits_s"].cpu() - ls_ref).abs().max()) < 1e-3
    assert float((out["logits_t"].cpu() - lt_ref).abs().max()) < 1e-3

    # two pipelined submits, the second one ragged (2 clips), equal the unpipelined runs
    random.seed(6)
    crops2 = augment.draw_clip_crops(2, L, (H, W), (H, W))
    single = pipe.run_batch(rgb[:2].cuda(), gray[:2].cuda(), crops=crops2)
    a = pipe.submit(rgb.cuda(), gray.cuda(), crops=crops)
    b = pipe.submit(rgb[:2].cuda(), gray[:2].cuda(), crops=crops2)
    pipe.wait()
    for k in ("logits_s", "logits_t", "desc_s", "desc_t"):
        assert torch.equal(a[k], out[k]) and torch.equal(b[k], single[k]), k
    pipe.close()


def test_bad_crops_are_refused_on_the_host():
    from video_analytics_amd import _ffi, augment, pipeline, synth
    from video_analytics_amd import flow as vflow
    fl = torch.zeros(2, 2, 240, 320, device="cuda")
    ok = torch.zeros(4, 3, dtype=torch.int32)
    for bad in (torch.tensor([[17, 0, 0]] * 4, dtype=torch.int32), torch.tensor([[0, -1, 0]] * 4, dtype=torch.int32),
                ok[:3], ok.long(), ok.cuda()):
        with pytest.raises(ValueError):
            vflow.crop_flow_to_stack(fl, bad)
    with pytest.raises(ValueError):
        vflow.crop_flow_to_stack(fl[:, :, :200], ok)  # frame smaller than the crop
    x = torch.zeros(4, 3, 240, 320, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        augment.crop_images(x, torch.tensor([[0, 97, 1]] * 4, dtype=torch.int32))
    with pytest.raises(ValueError):
        augment.crop_images(x, ok, layout="CHWN")
    rgb, gray, _ = synth.synth_clips(1, seed=0, H=240, W=320)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=_ffi.default_tvl1_params(epsilon=0.0, iters=4, warps=1))
    rc, fc = augment.draw_clip_crops(1, 10, (240, 320), (240, 320))
    with pytest.raises(ValueError, match="crops="):
        pipe.submit(rgb.cuda(), gray.cuda(), crops=(None, fc))  # 320x240 rgb without its crop
    with pytest.raises(ValueError):
        pipe.submit(rgb.cuda(), gray.cuda(), crops=(rc, fc[:19]))
    assert pipe._n == 0  # nothing was enqueued
    pipe.close()
