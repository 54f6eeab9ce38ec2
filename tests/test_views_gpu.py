"""Ten-crop evaluation on the device: the view gathers va_flow_to_stack_views / va_crop_images_u8_views
against numpy gathers of the oracle's S9 volume, the TSN inversion of mirrored x-flow images, va_view_mean against a
float32 loop in view order, TwoStreamPipeline(views=) at 320x240 against independently built inputs and the torch-CPU
oracle, and validate() on five-dimensional ten-crop batches."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEAN, STD = np.float32(0.485), np.float32(0.229)


def _normalise(q_u8):
    """S9's normalisation of 8-bit flow images, in float32: (q/255 - mean)/std."""
    return (q_u8.astype(np.float32) / np.float32(255.0) - MEAN) / STD


def _volume_rows(fl, crops, L, invert, oracle):
    """numpy reference: the oracle's S9 volume of flow [N,2,H,W] gathered by one crop row per output plane, output plane
    o = (b*V + v)*2L + c reading source plane b*2L + c (V = rows / N / 2); with ``invert``, mirrored x-flow planes are
    recomputed from utils.flowToImages as 255 - q."""
    from video_analytics_amd import utils
    N, _, H, W = fl.shape
    full = oracle.flow_to_stack(fl)                              # [2N,H,W]
    inv = _normalise(255 - utils.flowToImages(fl).reshape(2 * N, H, W)) if invert else None
    C = 2 * L
    V = crops.shape[0] // (2 * N)
    out = np.empty((crops.shape[0], 224, 224), dtype=np.float32)
    for o, (top, left, flip) in enumerate(crops.tolist()):
        b, c = o // (V * C), o % C
        src = b * C + c
        plane = inv[src] if (invert and flip and c % 2 == 0) else full[src]
        win = plane[top:top + 224, left:left + 224]
        out[o] = win[:, ::-1] if flip else win
    return out


def _views_entry(fl, crops, n_clips, L, V, invert):
    """va_flow_to_stack_views called directly: crops CPU int32 [n_clips*V*2L,3], one row per output plane."""
    from video_analytics_amd import _ffi, augment
    N, _, H, W = fl.shape
    out = torch.empty((n_clips * V * 2 * L, 224, 224), dtype=torch.float32, device=fl.device)
    d = augment.crops_to_device(crops, fl.device)
    _ffi.check(_ffi.lib().va_flow_to_stack_views(_ffi.ctx(fl.device.index), _ffi.ptr(fl), n_clips, L, V, W, H, 20.0, 0.485,
                                                 0.229, _ffi.ptr(d), int(invert), 224, 224, _ffi.ptr(out),
                                                 _ffi.stream_ptr(fl.device)))
    return out


@pytest.mark.parametrize("h,w", [(241, 321), (240, 320)])
@pytest.mark.parametrize("invert", [False, True])
def test_flow_views_equal_s9_then_gather(oracle_tvl1, h, w, invert):
    from video_analytics_amd import augment
    from video_analytics_amd import flow as vflow
    B, L = 32, 10
    rs = np.random.RandomState(h + int(invert))
    fl = (rs.standard_normal((B * L, 2, h, w)) * 12.0).astype(np.float32)  # sigma 12 px: both clamps at +-20 are hit
    views = augment.ten_crop_views(h, w)
    got = vflow.crop_flow_to_stack_views(torch.from_numpy(fl).cuda(), views, L, invert_x_on_flip=invert)
    assert tuple(got.shape) == (B, 10, 2 * L, 224, 224)
    ref = _volume_rows(fl, augment.expand_views(views, B, 2 * L), L, invert, oracle_tvl1)
    assert np.array_equal(got.cpu().numpy().reshape(-1, 224, 224), ref)
    if invert:  # the inversion changed exactly the mirrored x-flow planes
        plain = _volume_rows(fl, augment.expand_views(views, B, 2 * L), L, False, oracle_tvl1).reshape(B, 10, 2 * L, 224, 224)
        ref = ref.reshape(B, 10, 2 * L, 224, 224)
        differs = np.array([[[not np.array_equal(ref[0, v, c], plain[0, v, c]) for c in range(2 * L)] for v in range(10)]])
        assert differs[0, 5:, 0::2].all() and not differs[0, :5].any() and not differs[0, :, 1::2].any()


def test_single_view_entry_equals_the_crop_entry_and_inverts_only_mirrored_x(oracle_tvl1):
    from video_analytics_amd import augment, utils
    from video_analytics_amd import flow as vflow
    B, L, h, w = 6, 10, 240, 320
    rs = np.random.RandomState(11)
    fl_np = (rs.standard_normal((B * L, 2, h, w)) * 12.0).astype(np.float32)
    fl = torch.from_numpy(fl_np).cuda()
    random.seed(11)
    crops = augment.draw_flow_crops(B, L, h, w)
    base = vflow.crop_flow_to_stack(fl, crops)  # va_flow_to_stack_crop
    assert torch.equal(_views_entry(fl, crops, B, L, 1, False), base)
    on = _views_entry(fl, crops, B, L, 1, True)
    assert torch.equal(vflow.crop_flow_to_stack(fl, crops, invert_x_on_flip=True), on)  # one clip of B*L pairs, the same rows
    flip = crops[:, 2].numpy() == 1
    even = (np.arange(B * 2 * L) % 2) == 0
    changed = flip & even
    assert changed.any() and (flip & ~even).any()
    base, on = base.cpu().numpy(), on.cpu().numpy()
    assert np.array_equal(on[~changed], base[~changed])
    inv = _normalise(255 - utils.flowToImages(fl_np).reshape(2 * B * L, h, w))
    for o in np.nonzero(changed)[0]:
        top, left, _ = crops[o].tolist()
        assert np.array_equal(on[o], inv[o, top:top + 224, left:left + 224][:, ::-1]), o
        assert not np.array_equal(on[o], base[o])


@pytest.mark.parametrize("n,c,h,w", [(5, 3, 240, 320), (3, 3, 225, 321), (2, 1, 224, 224)])
def test_image_views_equal_numpy_slicing(n, c, h, w):
    from video_analytics_amd import augment
    rs = np.random.RandomState(n * 10 + c)
    x = rs.randint(0, 256, size=(n, c, h, w)).astype(np.uint8)
    views = augment.ten_crop_views(h, w)
    ref = np.empty((n, 10, c, 224, 224), dtype=np.uint8)
    for i in range(n):
        for v, (top, left, flip) in enumerate(views.tolist()):
            win = x[i, :, top:top + 224, left:left + 224]
            ref[i, v] = win[:, :, ::-1] if flip else win
    got = augment.crop_image_views(torch.from_numpy(x).cuda(), views)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref)
    nhwc = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda()
    assert np.array_equal(augment.crop_image_views(nhwc, views, layout="NHWC").cpu().numpy(), ref)
    # three views: a table of any length
    assert np.array_equal(augment.crop_image_views(torch.from_numpy(x).cuda(), views[3:6]).cpu().numpy(), ref[:, 3:6])


@pytest.mark.parametrize("V", [1, 3, 10])
@pytest.mark.parametrize("d", [7, 101, 256])
def test_view_mean_equals_a_float32_loop_in_view_order(V, d):
    from video_analytics_amd import vgg
    rs = np.random.RandomState(V * 1000 + d)
    x = (rs.standard_normal((37, V, d)) * np.exp(rs.uniform(-8, 8, size=(37, V, d)))).astype(np.float32)
    acc = x[:, 0].copy()
    for v in range(1, V):
        acc = acc + x[:, v]
    ref = acc / np.float32(V)
    got = vgg.view_mean(torch.from_numpy(x).cuda()).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, ref)


def test_pipeline_ten_views_at_native_size(oracle_tvl1):
    """B = 32 clips of 320x240, ten views, fp32: 320 images per stream in one forward_views chunk."""
    from oracle import vgg_oracle
    from video_analytics_amd import _ffi, augment, pipeline, synth
    from video_analytics_amd import flow as vflow
    from video_analytics_amd.parameters import NORM_MEANS_TF, NORM_STDS_TF
    B, L, H, W = 32, 10, 240, 320
    rgb, gray, _ = synth.synth_clips(B, seed=23, H=H, W=W)
    params = _ffi.default_tvl1_params(epsilon=0.0, iters=10, warps=1, nscales=3)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    views = augment.ten_crop_views(H, W)
    with pytest.raises(ValueError):
        pipe.submit(rgb.cuda(), gray.cuda(), views=(views, views), crops=augment.draw_clip_crops(B, L, (H, W), (H, W)))
    with pytest.raises(ValueError):
        pipe.submit(rgb.cuda(), None, flow_stack=torch.zeros(B, 20, 224, 224, device="cuda"), views=(views, views))
    assert pipe._n == 0
    out = pipe.run_batch(rgb.cuda(), gray.cuda(), views=(views, views), invert_flow_x=True)

    # inputs built independently: the volume as a numpy gather of tvl1_flow's flow, the RGB views by slicing
    fl = vflow.tvl1_flow(gray.cuda(), params).cpu().numpy()
    xt = _volume_rows(fl, augment.expand_views(views, B, 2 * L), L, True, oracle_tvl1).reshape(B * 10, 2 * L, 224, 224)
    xs = np.empty((B * 10, 3, 224, 224), dtype=np.uint8)
    r = rgb.numpy()
    for b in range(B):
        for v, (top, left, flip) in enumerate(views.tolist()):
            win = r[b, :, top:top + 224, left:left + 224]
            xs[b * 10 + v] = win[:, :, ::-1] if flip else win
    _, ds, ls = pipe.spatial.forward(torch.from_numpy(xs).cuda())
    _, dt, lt = pipe.temporal.forward(torch.from_numpy(xt).cuda())
    torch.cuda.synchronize()
    for key, ref in (("logits_s", ls), ("desc_s", ds), ("logits_t", lt), ("desc_t", dt)):
        per = out[key + "_views"]
        assert tuple(per.shape) == (B, 10, ref.shape[1]), key
        assert torch.equal(per.reshape(B * 10, -1), ref), key
        p = per.cpu().numpy()
        acc = p[:, 0].copy()
        for v in range(1, 10):
            acc = acc + p[:, v]
        assert np.array_equal(out[key].cpu().numpy(), acc / np.float32(10)), key

    rows = [0, 166, 167, 168, 319]  # image 167 straddles 2 GiB of fp32 224x224x64 activations
    ws = synth.synth_vgg16_weights(c_in=3, seed=1)
    wt = synth.synth_vgg16_weights(c_in=20, seed=2)
    wt["conv_w"][0] = vgg_oracle.copy_first_layer(wt["conv_w"][0], 20)
    xs_r = vgg_oracle.normalize_u8(torch.from_numpy(xs[rows]), NORM_MEANS_TF, NORM_STDS_TF)
    _, _, ls_ref = vgg_oracle.forward(xs_r, ws["conv_w"], ws["conv_b"], ws["fc_w"], ws["fc_b"])
    _, _, lt_ref = vgg_oracle.forward(torch.from_numpy(xt[rows]), wt["conv_w"], wt["conv_b"], wt["fc_w"], wt["fc_b"])
    assert float((out["logits_s_views"].reshape(B * 10, -1)[rows].cpu() - ls_ref).abs().max()) < 1e-3
    assert float((out["logits_t_views"].reshape(B * 10, -1)[rows].cpu() - lt_ref).abs().max()) < 1e-3
    pipe.close()


def test_bf16_views_run_in_chunks_of_whole_clips():
    """B = 33 clips of ten views: 330 images, two chunks (320 + 10), each equal to a direct forward of that chunk."""
    from video_analytics_amd import synth, vgg
    from video_analytics_amd.parameters import NORM_MEANS_TF, NORM_STDS_TF
    w = synth.synth_vgg16_weights(c_in=3, seed=1, device=torch.device("cuda", 0))
    m = vgg.Vgg16Stream(w["conv_w"], w["conv_b"], w["fc_w"], w["fc_b"], 101, 256, NORM_MEANS_TF, NORM_STDS_TF, device=0,
                        dtype="bf16")
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (33, 10, 3, 224, 224), generator=g, dtype=torch.uint8).cuda()
    desc, logits, desc_v, logits_v = m.forward_views(x)
    flat = x.view(330, 3, 224, 224)
    _, d0, l0 = m.forward(flat[:320])
    _, d1, l1 = m.forward(flat[320:])
    assert torch.equal(desc_v.view(330, -1), torch.cat([d0, d1])) and torch.equal(logits_v.view(330, -1), torch.cat([l0, l1]))
    assert torch.equal(desc, vgg.view_mean(desc_v)) and torch.equal(logits, vgg.view_mean(logits_v))
    assert bool(torch.isfinite(logits).all())
    m.close()


def _recompute(model, batches):
    """validate()'s result recomputed from forward_views: (correct / n, summed per-batch mean CE, {video: desc})."""
    from video_analytics_amd import vgg
    loss, correct, descs, n = 0, 0, {}, 0
    for d, l, ns in batches:
        desc, logits, _, _ = model.forward_views(d.cuda())
        v = vgg.validate_batch(logits, l).cpu()
        loss = loss + v[0]
        correct += int(v[1].item())
        for i, name in enumerate(ns):
            descs[name] = desc[i].clone()
        n += len(ns)
    return correct / n, loss, descs


def _check_validate(net, batches):
    acc_r, loss_r, desc_r = _recompute(net.model, batches)
    acc, loss = net.validate()
    assert acc == acc_r and torch.equal(torch.as_tensor(loss), torch.as_tensor(loss_r))
    assert list(net.testDict.keys()) == list(desc_r.keys())
    for name, ref in desc_r.items():
        meter, label = net.testDict[name]
        assert meter.count == 1 and int(label) == 1
        assert torch.equal(meter.avg.cpu(), ref.cpu()), name


def test_validate_on_ten_crop_batches(tmp_path):
    from PIL import Image
    from video_analytics_amd import utils as U
    from video_analytics_amd.spatialModel import SpatialDataset, SpatialNetwork
    from video_analytics_amd.temporalModel import TemporalDataset, TemporalNetwork
    lines = open(os.path.join(GOLD, "demoTest.txt")).readlines()[:3]
    lst = tmp_path / "list.txt"
    lst.write_text("".join(lines))
    (tmp_path / "classInd.txt").write_text("1 ApplyEyeMakeup\n2 ApplyLipstick\n3 Archery\n")
    rng = np.random.default_rng(3)
    L = 2
    for line in lines:
        _, videoName, _, category, _, _ = U.videoInfo(line, "test")
        fd = tmp_path / "frames" / category / videoName
        fd.mkdir(parents=True)
        for i in range(3):
            img = rng.integers(0, 255, (30, 40, 3), dtype=np.uint8).repeat(8, axis=0).repeat(8, axis=1)
            Image.fromarray(img).save(str(fd / ("%d.jpg" % i)), quality=90)
        od = tmp_path / "flows" / category / videoName
        od.mkdir(parents=True)
        for k in range(1, 5):
            for prefix in ("flow_x_", "flow_y_"):
                img = rng.integers(0, 255, (30, 40), dtype=np.uint8).repeat(8, axis=0).repeat(8, axis=1)
                Image.fromarray(img, mode="L").save(str(od / U.flowFileName(prefix, k)), quality=90)
    tf = U.getTenCropTransforms()
    tft = U.getTenCropTransforms(invertFlowX=True)
    cl = str(tmp_path / "classInd.txt")
    sds = SpatialDataset(str(lst), str(tmp_path / "frames"), tf, mode="test", actionLabelLoc=cl)
    tds = TemporalDataset(str(lst), str(tmp_path / "flows"), tft, flowSampleSize=L, mode="test", actionLabelLoc=cl)
    for ds, c, Net, args in ((sds, 3, SpatialNetwork, ()), (tds, 2 * L, TemporalNetwork, (L,))):
        loader = U.getDataLoader(ds, batchSize=2, nWorkers=0, shuffle=False)
        random.seed(7)
        batches = [(d.clone(), l.clone(), list(n)) for d, l, n in loader]
        assert [tuple(d.shape) for d, _, _ in batches] == [(2, 10, c, 224, 224), (1, 10, c, 224, 224)]
        net = Net(101, *args, 1, 0.1, 0.9, 256, None, loader, [10, 20], None, gpu=True)
        random.seed(7)  # the same frame / start draws again
        _check_validate(net, batches)
        net.model.close()
