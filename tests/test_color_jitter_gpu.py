"""Colour jitter on the device: va_color_jitter_u8 against the PIL golden file and against the numpy
ops of video_analytics_amd/utils.py (themselves held to PIL by tests/test_color_jitter_host.py) bit for bit, on every RGB
colour, with contrast before and after other ops, mixed rows, in place, with lighting; the seeded data path against the
host's getTransforms(jitter=...); and TwoStreamPipeline.train_videos against the same pieces called by hand."""
import hashlib
import random

import numpy as np
import pytest
import torch

from test_color_jitter_host import check_rgb_pca, every_colour, golden_module, in_slabs, jitter_numpy

pytestmark = pytest.mark.gpu

IDENTITY = [0, 0, 0, 0, 1.0, 1.0, 1.0, 0]


def _to_device(imgs_hwc):
    """u8 [n,h,w,3] (numpy) -> CUDA u8 [n,3,h,w]."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(imgs_hwc).transpose(0, 3, 1, 2))).cuda()


def _to_host(x):
    """CUDA u8 [n,3,h,w] -> numpy u8 [n,h,w,3]."""
    return np.ascontiguousarray(x.cpu().numpy().transpose(0, 2, 3, 1))


def _table(rows):
    return torch.tensor(rows, dtype=torch.float32).view(len(rows), 8)


def _row(op, value):
    """A row with one op."""
    r = list(IDENTITY)
    r[0] = op
    r[7 if op == 4 else 3 + op] = value
    return r


@pytest.fixture(scope="module")
def golden():
    gen = golden_module()
    return gen, np.load(gen.OUT)


# ---- the golden file ----

@pytest.mark.parametrize("h,w", [(5, 7), (33, 61), (224, 224)])
def test_device_equals_the_pil_golden_for_all_24_orders(golden, h, w):
    from video_analytics_amd import augment
    gen, z = golden
    nm, img = gen.name(h, w), gen.image(h, w)
    table = torch.from_numpy(z["table_" + nm])
    assert tuple(table.shape) == (24, 8)
    got = _to_host(augment.color_jitter(_to_device(np.stack([img] * 24)), table))
    ref = np.stack([jitter_numpy(img, row) for row in table.numpy()])
    bad = (got != ref).reshape(24, -1).sum(axis=1)
    print("%s: bytes that differ from the numpy ops, per order: %s" % (nm, bad.tolist()))
    if nm in gen.STORED:
        assert np.array_equal(z["image_" + nm], img)
        assert np.array_equal(got, z["out_" + nm]), bad.tolist()
    else:
        assert hashlib.sha256(img.tobytes()).digest() == z["image_sha_" + nm].tobytes()
        assert np.array_equal(got.reshape(24, -1, 3).sum(axis=1, dtype=np.int64), z["sums_" + nm]), bad.tolist()
        for i in range(24):
            assert hashlib.sha256(got[i].tobytes()).digest() == z["sha_" + nm][i].tobytes(), (i, bad.tolist())
    assert np.array_equal(got, ref)


def test_the_ops_before_contrast_move_its_gray_value(golden):
    from video_analytics_amd import augment
    gen, z = golden
    img = gen.image(33, 61)
    table = torch.from_numpy(z["table_placement"])
    assert table[:, :2].tolist() == [[1, 2], [2, 1]]
    got = _to_host(augment.color_jitter(_to_device(np.stack([img] * 2)), table))
    assert np.array_equal(got, z["out_placement"]) and not np.array_equal(got[0], got[1])


def test_the_tie_and_the_constant_images():
    """N = 2 pixels with gray levels 10 and 11: the mean 10.5 rounds up to m = 11; constant 0 and 255 images keep m there."""
    from video_analytics_amd import augment, utils
    imgs = np.stack([np.array([[[10, 10, 10], [11, 11, 11]]], dtype=np.uint8), np.zeros((1, 2, 3), np.uint8),
                     np.full((1, 2, 3), 255, np.uint8)])
    x = _to_device(imgs)
    for f in (0.0, 0.5, 1.5):
        got = _to_host(augment.color_jitter(x, _table([_row(2, f)] * 3)))
        for i, m in enumerate((11, 0, 255)):
            assert np.array_equal(got[i], utils.adjustContrast(imgs[i], f)), (i, f)
            if f == 0.0:
                assert (got[i] == m).all()


# ---- every RGB colour ----

@pytest.fixture(scope="module")
def domain():
    """(numpy u8 [4096,4096,3], CUDA u8 [64,3,512,512]): every RGB colour once; image i is rows 64 i .. 64 i + 63 of the
    numpy array read as 512 x 512 pixels."""
    full = every_colour()
    x = torch.from_numpy(full.reshape(64, 512, 512, 3)).cuda().permute(0, 3, 1, 2).contiguous()
    return full, x


FULL_DOMAIN = [(1, 0.37), (1, 1.0), (1, 1.83), (3, 0.0), (3, 0.61), (3, 1.9), (4, 1), (4, 128), (4, 243), (2, 0.45), (2, 1.6)]


@pytest.mark.parametrize("op,value", FULL_DOMAIN, ids=["%s-%s" % (("b", "c", "s", "h")[o - 1], v) for o, v in FULL_DOMAIN])
def test_one_op_on_every_colour_equals_the_numpy_op(domain, op, value):
    from video_analytics_amd import augment, utils
    full, x = domain
    got = _to_host(augment.color_jitter(x, _table([_row(op, value)] * 64))).reshape(4096, 4096, 3)
    if op == 2:  # each 512 x 512 image with its own m
        imgs = full.reshape(64, 512, 512, 3)
        means = [utils.contrastMean(im) for im in imgs]
        assert len(set(means)) > 1
        ref = np.stack([utils.adjustContrast(im, value, m) for im, m in zip(imgs, means)]).reshape(4096, 4096, 3)
    else:
        fn = {1: utils.adjustBrightness, 3: utils.adjustSaturation, 4: utils.adjustHue}[op]
        ref = in_slabs(lambda a: fn(a, value), full)
    bad = int((got != ref).any(axis=-1).sum())
    print("op %d value %s: %d of 16777216 colours differ" % (op, value, bad))
    assert bad == 0


# ---- rows, buffers ----

def test_mixed_rows_in_one_call_equal_one_call_each(golden):
    from video_analytics_amd import augment
    gen, z = golden
    imgs = np.stack([gen.image(33, 61), gen.image(33, 61)[::-1], gen.image(33, 61)[:, ::-1], gen.image(33, 61)])
    rows = [z["table_33x61"][5].tolist(), [0.0] * 8, z["table_33x61"][17].tolist(), _row(3, 1.4)]  # row 1: all zeros
    x = _to_device(imgs)
    got = augment.color_jitter(x, _table(rows))
    for i in range(4):
        one = augment.color_jitter(x[i:i + 1], _table([rows[i]]))
        assert torch.equal(got[i:i + 1], one), i
        assert np.array_equal(_to_host(one)[0], jitter_numpy(imgs[i], np.array(rows[i]))), i
    assert torch.equal(got[1], x[1])  # a row of zeros leaves the image's bits


@pytest.mark.parametrize("h,w", [(601, 500), (523, 515)])
def test_an_image_of_more_pixels_than_one_grid_covers(golden, h, w):
    """Above 1024 x 256 pixels an image's workgroups stride over it: 300 500 pixels (4-byte runs) and 269 345 (the byte path),
    two images with different rows, contrast after and before the other ops."""
    from video_analytics_amd import augment
    gen, z = golden
    assert h * w > 1024 * 256
    imgs = np.random.RandomState(h).randint(0, 256, size=(2, h, w, 3)).astype(np.uint8)
    rows = z["table_224x224"][[22, 7]]
    assert rows[0, 3] == 2 and rows[1, 0] == 2
    got = _to_host(augment.color_jitter(_to_device(imgs), torch.from_numpy(rows)))
    for i in range(2):
        assert np.array_equal(got[i], jitter_numpy(imgs[i], rows[i])), i


@pytest.mark.parametrize("h,w", [(33, 61), (224, 224)])
def test_in_place_equals_out_of_place_and_calls_repeat(golden, h, w):
    from video_analytics_amd import augment
    gen, z = golden
    table = torch.from_numpy(z["table_" + gen.name(h, w)][:6])
    x = _to_device(np.stack([gen.image(h, w)] * 6))
    a = augment.color_jitter(x, table)
    b = augment.color_jitter(x, table)
    assert torch.equal(a, b)
    y = x.clone()
    c = augment.color_jitter(y, table, out=y)
    assert c.data_ptr() == y.data_ptr() and torch.equal(y, a)
    # a buffer one byte past a 4-byte boundary: the byte path, source and destination
    flat = torch.full((x.numel() + 1,), 77, dtype=torch.uint8, device="cuda")
    flat[1:] = x.reshape(-1)
    un = flat[1:].view(x.shape)
    assert un.data_ptr() % 4 == 1
    assert torch.equal(augment.color_jitter(un, table), a)
    out = torch.full((x.numel() + 2,), 55, dtype=torch.uint8, device="cuda")
    assert torch.equal(augment.color_jitter(x, table, out=out[1:-1]), a) and int(out[0]) == 55 and int(out[-1]) == 55
    assert torch.equal(augment.color_jitter(un, table, out=un), a) and int(flat[0]) == 77


def test_bad_arguments_are_refused():
    from video_analytics_amd import _ffi, augment
    x = torch.zeros(2, 3, 8, 8, dtype=torch.uint8, device="cuda")
    good = _table([IDENTITY] * 2)
    for bad in (x.float(), x.cpu(), x[:, :2], x[0]):
        with pytest.raises(ValueError):
            augment.color_jitter(bad, good)
    for bad in (good[:1], good.cuda(), _table([[5, 0, 0, 0, 1, 1, 1, 0]] * 2), _table([[2, 2, 0, 0, 1, 1, 1, 0]] * 2)):
        with pytest.raises(ValueError):
            augment.color_jitter(x, bad)
    with pytest.raises(ValueError):
        augment.color_jitter(x, good, lighting=torch.zeros(3, 3))
    with pytest.raises(ValueError):
        augment.color_jitter(x, good, out=torch.zeros(2, 3, 8, 4, dtype=torch.uint8, device="cuda"))
    L, c, st = _ffi.lib(), _ffi.ctx(0), _ffi.stream_ptr(x.device)
    tab = good.cuda()
    work = torch.zeros(2 * _ffi.VA_COLOR_JITTER_PARTIALS, dtype=torch.int32, device="cuda")
    big = torch.zeros(2 * 3 * 8 * 8 + 8, dtype=torch.uint8, device="cuda")

    def call(src=x, n=2, w=8, h=8, table=tab, lighting=None, dst=x, ws=work):
        return L.va_color_jitter_u8(c, _ffi.ptr(src), n, w, h, _ffi.ptr(table), _ffi.ptr(lighting), _ffi.ptr(dst), _ffi.ptr(ws), st)
    assert call() == _ffi.VA_OK and call(ws=None) == _ffi.VA_OK
    for kw in (dict(src=None), dict(table=None), dict(dst=None), dict(n=0), dict(w=0), dict(h=-1), dict(n=65536),
               dict(w=1 << 15, h=1 << 15), dict(ws=work.view(torch.uint8)[1:]), dict(table=tab.view(torch.uint8)[2:]),
               dict(src=big, dst=big[8:])):  # overlapping, not equal
        assert call(**kw) == _ffi.VA_ERR_INVALID, kw
        assert b"va_color_jitter_u8" in L.va_last_error()
    torch.cuda.synchronize()


# ---- lighting ----

def test_lighting_equals_rint_of_the_clamped_sum(golden):
    from video_analytics_amd import augment, utils
    gen, z = golden
    imgs = np.stack([gen.image(33, 61)] * 4)
    x = _to_device(imgs)
    light = torch.tensor([[0.0, 0.0, 0.0], [12.3, -7.75, 0.5], [300.0, -300.0, 254.5], [-0.5, 1.5, 2.5]], dtype=torch.float32)
    got = _to_host(augment.color_jitter(x, _table([IDENTITY] * 4), lighting=light))
    for i in range(4):
        assert np.array_equal(got[i], utils.applyLighting(imgs[i], light[i].numpy())), i
    assert np.array_equal(got[0], imgs[0]) and (got[2][..., 0] == 255).all() and (got[2][..., 1] == 0).all()
    rows = z["table_33x61"][[3, 9, 14, 20]]
    both = _to_host(augment.color_jitter(x, torch.from_numpy(rows), lighting=light))  # applied last
    for i in range(4):
        assert np.array_equal(both[i], utils.applyLighting(jitter_numpy(imgs[i], rows[i]), light[i].numpy())), i


def test_rgb_pca_on_the_device_agrees_with_numpy_eigh():
    from video_analytics_amd import augment
    x = torch.from_numpy(np.random.RandomState(6).randint(0, 256, size=(7, 3, 60, 80)).astype(np.uint8))
    x[:, 2] = x[:, 0] // 3 + x[:, 2] // 2
    val, vec = augment.rgb_pca(x.cuda())
    check_rgb_pca(x, val, vec)
    off = augment.draw_lighting(3, val, vec, rng=random.Random(2))
    assert tuple(off.shape) == (3, 3) and torch.isfinite(off).all()


# ---- the data path ----

def test_device_path_replays_the_hosts_jittered_transforms():
    """Seeded host getTransforms(jitter=...) on 4 frames of 240x320 and the seeded device path (crop_images, color_jitter, the
    stream's ToTensor + Normalize of the u8 input) give the same normalised crops, bit for bit."""
    from video_analytics_amd import augment, synth, utils
    from video_analytics_amd.parameters import NORM_MEANS_TF, NORM_STDS_TF
    jitter = [.4, .4, .4, .1]
    rgb, _, _ = synth.synth_clips(4, seed=3, H=240, W=320)
    tf = utils.getTransforms(jitter=jitter)
    random.seed(44)
    host = torch.stack([tf(rgb[b].permute(1, 2, 0).numpy()) for b in range(4)])
    state = random.getstate()
    random.seed(44)
    crops, params = augment.draw_image_transforms(4, 240, 320, jitter)
    assert random.getstate() == state
    assert sorted(params[0, :4].tolist()) == [1, 2, 3, 4]
    norm = utils.Compose([utils.ToTensor(), utils.Normalize(NORM_MEANS_TF, NORM_STDS_TF)])
    for layout, x in (("NCHW", rgb), ("NHWC", rgb.permute(0, 2, 3, 1).contiguous())):
        u8 = augment.crop_images(x.cuda(), crops, layout=layout)
        u8 = augment.color_jitter(u8, params, out=u8).cpu()
        dev = torch.stack([norm(u8[b].permute(1, 2, 0).numpy()) for b in range(4)])
        assert torch.equal(host, dev), layout


# ---- train_videos ----

def test_train_videos_jitters_the_spatial_input_alone():
    from test_tsn_gpu import _state, _videos
    from test_video_gpu import SCHEDULE
    from video_analytics_amd import _ffi, augment, pipeline
    from video_analytics_amd.video import segmentStarts
    L, k, lr, mu, seed = 10, 3, 1e-4, 0.9, 5
    vids, starts = _videos()
    dev = [(r.cuda(), g.cuda()) for r, g in vids]
    crops = augment.draw_scale_jitter_crops(6, 240, 320, random.Random(3))
    labels = torch.tensor([5, 77])
    table = augment.draw_color_jitter(6, .4, .4, .4, .1, rng=random.Random(12))
    table[2] = torch.tensor(IDENTITY)
    light = augment.draw_lighting(6, [3.0, 40.0, 900.0], torch.eye(3, dtype=torch.float64), rng=random.Random(13))
    params = _ffi.default_tvl1_params(**SCHEDULE)
    pipe = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    twin = pipeline.TwoStreamPipeline(device=0, tvl1_params=params)
    kw = dict(k=k, starts=starts, crops=crops, lr=lr, momentum=mu, dropout_seed=seed)
    out = pipe.train_videos(dev, labels, jitter=table, lighting=light, **kw)
    assert torch.equal(out["jitter"], table)
    # the spatial stream by hand on the twin: resize_images -> color_jitter -> train_step_consensus
    frames = torch.cat([rgb[torch.tensor(st).cuda()] for (rgb, _), st in zip(dev, starts)])
    rgb_table = torch.cat([torch.arange(6, dtype=torch.int32).view(6, 1), crops], dim=1)
    plain_xs = augment.resize_images(frames, rgb_table)
    xs = augment.color_jitter(plain_xs, table, light)
    assert torch.equal(xs[2], torch.from_numpy(
        np.rint(np.clip(plain_xs[2].cpu().numpy().astype(np.float32) + light[2].numpy().reshape(3, 1, 1), 0, 255)).astype(np.uint8)).cuda())
    assert not torch.equal(xs[0], plain_xs[0])
    stats, desc = twin.spatial.train_step_consensus(xs, labels, k, lr, mu, seed)
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and torch.equal(out["stats_s"], stats) and torch.equal(out["desc_s"], desc)
    assert all(torch.equal(a, b) for a, b in zip(_state(pipe.spatial), _state(twin.spatial)))
    # the temporal stream: the unjittered run's bits
    base = twin.train_videos(dev, labels, **kw)
    assert base["jitter"] is None
    assert torch.equal(out["stats_t"], base["stats_t"]) and torch.equal(out["desc_t"], base["desc_t"])
    assert all(torch.equal(a, b) for a, b in zip(_state(pipe.temporal), _state(twin.temporal)))
    # color_jitter=: drawn from the step's generator after the starts and the crops
    a = pipe.train_videos(dev, labels, k=k, lr=lr, rng=random.Random(9), color_jitter=(.4, .4, .4, .1))
    rng = random.Random(9)
    assert a["starts"] == [segmentStarts(g.shape[0], k, L, rng) for _, g in vids]
    assert torch.equal(a["crops"], augment.draw_scale_jitter_crops(6, 240, 320, rng))
    assert torch.equal(a["jitter"], augment.draw_color_jitter(6, .4, .4, .4, .1, rng))
    assert torch.isfinite(a["stats_s"]).all() and torch.isfinite(a["stats_t"]).all()
    pipe.close()
    twin.close()


def test_train_videos_refuses_bad_jitter_before_anything_is_enqueued(monkeypatch):
    from video_analytics_amd import _ffi, augment, pipeline
    from video_analytics_amd import flow as vflow
    pipe = pipeline.TwoStreamPipeline(device=0)
    rgb = torch.zeros(25, 3, 240, 320, dtype=torch.uint8, device="cuda")
    gray = torch.zeros(25, 240, 320, dtype=torch.uint8, device="cuda")
    crops = augment.draw_scale_jitter_crops(6, 240, 320, random.Random(1))
    table = augment.draw_color_jitter(6, .4, .4, .4, .1, rng=random.Random(2))
    light = torch.zeros(6, 3)
    torch.cuda.synchronize()

    def boom(*a, **k):
        raise AssertionError("reached the GPU")
    for mod, name in ((_ffi, "ctx"), (_ffi, "lib"), (vflow, "tvl1_flow"), (vflow, "tvl1_flow_concurrent"),
                      (vflow, "resize_flow_to_stack"), (augment, "resize_images"), (augment, "crops_to_device"),
                      (augment, "color_jitter")):
        monkeypatch.setattr(mod, name, boom)
    good = dict(videos=[(rgb, gray), (rgb, gray)], labels=[1, 2], k=3, starts=[[0, 3, 14], [0, 7, 14]], crops=crops, jitter=table,
                lighting=light)
    with pytest.raises(AssertionError, match="reached the GPU"):
        pipe.train_videos(**good)  # a good call passes every host check
    code, twice, nan = table.clone(), table.clone(), table.clone()
    code[1, 0] = 7
    twice[3, :4] = torch.tensor([2, 1, 2, 0])
    nan[5, 4] = float("nan")
    cases = dict(code=dict(jitter=code), twice=dict(jitter=twice), nan=dict(jitter=nan), rows=dict(jitter=table[:5]),
                 dtype=dict(jitter=table.double()), device=dict(jitter=table.cuda()), both=dict(color_jitter=(.4, .4, .4, .1)),
                 hue=dict(jitter=None, color_jitter=(.4, .4, .4, .6)), negative=dict(jitter=None, color_jitter=(-1, 0, 0, 0)),
                 three=dict(jitter=None, color_jitter=(.4, .4, .4)), light_rows=dict(lighting=light[:5]),
                 light_nan=dict(lighting=torch.full((6, 3), float("nan"))), light_device=dict(lighting=light.cuda()))
    for name, kw in cases.items():
        with pytest.raises(ValueError):
            pipe.train_videos(**dict(good, **kw))
            pytest.fail(name)
    monkeypatch.undo()
    pipe.close()
