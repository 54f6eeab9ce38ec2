"""Colour jitter on the host: the numpy ops of video_analytics_amd/utils.py against PIL itself (the
judge: torchvision's ColorJitter jitters PIL images), utils.ColorJitter against the PIL composition under the same seed, the
draw sequence, augment's tables and draws, and the golden file against its generator."""
import hashlib
import importlib.util
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLEND_FACTORS = [0.0, 0.5, 1.0, float(np.nextafter(np.float32(1), np.float32(2))), 1.7, 2.0]


def golden_module():
    path = os.path.join(ROOT, "tests", "golden", "make_color_jitter_golden.py")
    spec = importlib.util.spec_from_file_location("make_color_jitter_golden", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def every_colour():
    """u8 [4096,4096,3]: every RGB colour once, pixel index = R << 16 | G << 8 | B."""
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def in_slabs(fn, img, slabs=16):
    """``fn`` (a per-pixel op) over row slabs of ``img`` on a few threads (numpy releases the GIL) -> the whole result."""
    parts = np.array_split(img, slabs, axis=0)
    with ThreadPoolExecutor(max_workers=8) as pool:
        return np.concatenate(list(pool.map(fn, parts)), axis=0)


def row_ops(row):
    """A table row ``{op0..op3, fb, fc, fs, shift}`` -> ``[(op, value), ...]`` for ``utils.applyColorJitter``."""
    return [(int(row[k]), int(row[7]) if int(row[k]) == 4 else float(row[3 + int(row[k])])) for k in range(4) if int(row[k])]


def jitter_numpy(img, row):
    from video_analytics_amd import utils
    return utils.applyColorJitter(img, row_ops(row))


def _random_image(h, w, seed, mode="RGB"):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, size=(h, w, 3) if mode == "RGB" else (h, w)).astype(np.uint8)


# ---- the ops against PIL ----

def test_both_hsv_conversions_equal_pil_on_every_colour():
    from video_analytics_amd import utils
    full = every_colour()
    hsv = np.asarray(Image.fromarray(full, "RGB").convert("HSV"))
    mine = in_slabs(utils.rgbToHsv, full)
    assert int((mine != hsv).any(axis=-1).sum()) == 0
    rgb = np.asarray(Image.fromarray(full, "HSV").convert("RGB"))  # the same array read as every (h, s, v)
    back = in_slabs(utils.hsvToRgb, full)
    assert int((back != rgb).any(axis=-1).sum()) == 0


@pytest.mark.parametrize("mode", ["RGB", "L"])
def test_the_three_blends_equal_pil(mode):
    from video_analytics_amd import utils
    img = _random_image(224, 224, 7, mode)
    im = Image.fromarray(img)
    factors = BLEND_FACTORS + [float(f) for f in np.random.RandomState(8).uniform(0.0, 3.0, size=38)]
    assert len(factors) == 44
    for f in factors:
        assert np.array_equal(utils.adjustBrightness(img, f), np.asarray(ImageEnhance.Brightness(im).enhance(f))), f
        assert np.array_equal(utils.adjustContrast(img, f), np.asarray(ImageEnhance.Contrast(im).enhance(f))), f
        assert np.array_equal(utils.adjustSaturation(img, f), np.asarray(ImageEnhance.Color(im).enhance(f))), f
    if mode == "RGB":
        assert np.array_equal(utils.grayLevel(img), np.asarray(im.convert("L")))


def test_contrast_mean_rounds_half_up_in_integers():
    from video_analytics_amd import utils
    tie = np.array([[[10, 10, 10], [11, 11, 11]]], dtype=np.uint8)  # L = 10, 11: the mean is exactly 10.5
    assert utils.grayLevel(tie).tolist() == [[10, 11]] and utils.contrastMean(tie) == 11
    for img, m in ((tie, 11), (np.zeros((3, 5, 3), np.uint8), 0), (np.full((3, 5, 3), 255, np.uint8), 255),
                   (np.array([[10, 11]], dtype=np.uint8), 11)):
        assert utils.contrastMean(img) == m
        for f in (0.0, 0.5, 1.5):
            want = np.asarray(ImageEnhance.Contrast(Image.fromarray(img)).enhance(f))
            assert np.array_equal(utils.adjustContrast(img, f), want), (m, f)
            if f == 0.0:
                assert (want == m).all()


@pytest.mark.parametrize("factor,shift", [(0, 0), (0.5, 127), (-0.5, 129), (0.05, 12), (-0.05, 244)])
def test_hue_shifts_equal_the_wrap_around_add_on_pil(factor, shift):
    from video_analytics_amd import utils
    assert utils.hueShift(factor) == shift
    img = _random_image(33, 61, 9)
    h, s, v = Image.fromarray(img).convert("HSV").split()
    nh = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        nh += np.array(int(factor * 255)).astype(np.uint8)  # torchvision's np.uint8 add
    want = np.asarray(Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB"))
    assert np.array_equal(utils.adjustHue(img, utils.hueShift(factor)), want)
    gray = _random_image(5, 7, 1, "L")
    assert utils.adjustHue(gray, shift) is gray and utils.adjustSaturation(gray, 1.5) is gray


def test_lighting_is_rint_of_the_clamped_sum():
    from video_analytics_amd import utils
    img = _random_image(5, 7, 2)
    off = np.array([300.0, -12.5, 0.49], dtype=np.float32)
    got = utils.applyLighting(img, off)
    assert (got[..., 0] == 255).all() and np.array_equal(got[..., 2], img[..., 2])
    assert np.array_equal(got[..., 1], np.rint(np.maximum(img[..., 1].astype(np.float32) - np.float32(12.5), 0)).astype(np.uint8))


# ---- the class, the draws ----

def _spec_draws(rng, b, c, s, h):
    """DESIGN.md S32's draw order, restated: one uniform per non-zero parameter in the order b, c, s, h, then a shuffle."""
    ops = []
    if b:
        ops.append((1, rng.uniform(max(0, 1 - b), 1 + b)))
    if c:
        ops.append((2, rng.uniform(max(0, 1 - c), 1 + c)))
    if s:
        ops.append((3, rng.uniform(max(0, 1 - s), 1 + s)))
    if h:
        ops.append((4, int(rng.uniform(-h, h) * 255) % 256))
    if ops:
        rng.shuffle(ops)
    return ops


@pytest.mark.parametrize("mode", ["RGB", "L"])
@pytest.mark.parametrize("params", [(0.4, 0.4, 0.4, 0.1), (0, 0.9, 0, 0.5), (1.5, 0, 0.3, 0), (0, 0, 0, 0.25)])
def test_color_jitter_equals_the_pil_composition_under_the_same_seed(mode, params):
    from video_analytics_amd import utils
    gen = golden_module()
    img = _random_image(33, 61, 11, mode)
    tf = utils.ColorJitter(*params)
    seeded = utils.ColorJitter(*params, rng=random.Random(77))
    ref_rng = random.Random(77)
    random.seed(77)
    for _ in range(6):
        im = Image.fromarray(img)
        for op, value in _spec_draws(ref_rng, *params):
            im = gen.pil_op(im, op, value)
        want = np.asarray(im)
        assert np.array_equal(tf(img), want) and np.array_equal(seeded(img), want)
    assert random.getstate() == ref_rng.getstate()


class _Recorder(object):
    def __init__(self):
        self.calls, self.rng = [], random.Random(3)

    def uniform(self, a, b):
        self.calls.append(("uniform", a, b))
        return self.rng.uniform(a, b)

    def shuffle(self, x):
        self.calls.append(("shuffle", [op for op, _ in x]))
        self.rng.shuffle(x)


def test_the_draw_sequence():
    from video_analytics_amd import augment, utils
    img = _random_image(5, 7, 4)
    rec = _Recorder()
    utils.ColorJitter(0.4, 0.3, 0.2, 0.1, rng=rec)(img)
    assert rec.calls == [("uniform", 0.6, 1.4), ("uniform", 0.7, 1.3), ("uniform", 0.8, 1.2), ("uniform", -0.1, 0.1),
                         ("shuffle", [1, 2, 3, 4])]
    rec = _Recorder()
    utils.ColorJitter(2.0, 0, 0.2, 0, rng=rec)(img)  # max(0, 1 - p)
    assert rec.calls == [("uniform", 0, 3.0), ("uniform", 0.8, 1.2), ("shuffle", [1, 3])]
    rec = _Recorder()
    assert utils.ColorJitter(0, 0, 0, 0, rng=rec)(img) is img and rec.calls == []
    table = augment.draw_color_jitter(3, 0, 0, 0, 0, rng=rec)
    assert rec.calls == [] and table.tolist() == [list(augment.IDENTITY_JITTER_ROW)] * 3
    rec = _Recorder()
    utils.ColorJitter(0, 0.5, 0, 0, rng=rec)(img)  # one active op: one uniform and a shuffle of one
    assert rec.calls == [("uniform", 0.5, 1.5), ("shuffle", [2])]
    # the table of n images: the same calls image by image, the values where the row format puts them
    rec, ref = _Recorder(), random.Random(3)
    table = augment.draw_color_jitter(4, 0.4, 0.3, 0.2, 0.1, rng=rec)
    assert table.dtype == torch.float32 and tuple(table.shape) == (4, 8) and len(rec.calls) == 20
    for row in table.tolist():
        ops = _spec_draws(ref, 0.4, 0.3, 0.2, 0.1)
        assert row[:4] == [op for op, _ in ops]
        for op, value in ops:
            assert row[7 if op == 4 else 3 + op] == (value if op == 4 else float(np.float32(value)))


def test_get_transforms_with_jitter_runs_and_is_seed_reproducible():
    from video_analytics_amd import utils
    img = _random_image(240, 320, 5)
    tf = utils.getTransforms(jitter=[.4, .4, .4, .1])
    random.seed(21)
    a = tf(img)
    random.seed(21)
    b = tf(img)
    c = tf(img)
    assert a.dtype == torch.float32 and tuple(a.shape) == (3, 224, 224) and torch.equal(a, b) and not torch.equal(a, c)
    random.seed(21)
    plain = utils.getTransforms()(img)  # the default jitter: the identity, the crop's and the flip's draws alone
    assert not torch.equal(a, plain)


def test_draw_image_transforms_replays_get_transforms_draw_for_draw():
    from video_analytics_amd import augment, utils
    from video_analytics_amd.parameters import NORM_MEANS_TF, NORM_STDS_TF
    jitter = [.4, .4, .4, .1]
    imgs = [_random_image(240, 320, 30 + i) for i in range(3)]
    tf = utils.getTransforms(jitter=jitter)
    random.seed(99)
    host = [tf(im) for im in imgs]
    state = random.getstate()
    random.seed(99)
    crops, params = augment.draw_image_transforms(3, 240, 320, jitter)
    assert random.getstate() == state
    augment.check_crops(crops, 3, 240, 320, 224, "test")
    augment.check_color_jitter(params, 3)
    norm = utils.Compose([utils.ToTensor(), utils.Normalize(NORM_MEANS_TF, NORM_STDS_TF)])
    for im, want, (top, left, flip), row in zip(imgs, host, crops.tolist(), params.numpy()):
        v = im[top:top + 224, left:left + 224]
        v = v[:, ::-1] if flip else v
        assert torch.equal(norm(jitter_numpy(v, row)), want)
    # without jitter: draw_image_crops' numbers and identity rows
    random.seed(5)
    c0, p0 = augment.draw_image_transforms(4, 240, 320, None)
    random.seed(5)
    assert torch.equal(c0, augment.draw_image_crops(4, 240, 320)) and p0.tolist() == [list(augment.IDENTITY_JITTER_ROW)] * 4


def test_validation_errors():
    from video_analytics_amd import augment, utils
    for bad in ((-0.1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -0.5, 0), (0, 0, 0, 0.6), (0, 0, 0, -0.1), (float("nan"), 0, 0, 0)):
        with pytest.raises(ValueError):
            utils.ColorJitter(*bad)
        with pytest.raises(ValueError):
            augment.draw_color_jitter(2, *bad)
        with pytest.raises(ValueError):
            augment.draw_image_transforms(2, 240, 320, bad)
        with pytest.raises(ValueError):
            utils.getTransforms(jitter=list(bad))
    good = augment.draw_color_jitter(3, .4, .4, .4, .1, rng=random.Random(1))
    augment.check_color_jitter(good, 3)

    def changed(i, j, v):
        t = good.clone()
        t[i, j] = v
        return t
    twice = good.clone()
    twice[1, :4] = torch.tensor([1, 2, 1, 0])
    for bad in (good[:2], good.double(), good.to(torch.int32), good.view(3, 2, 4), good.tolist(), changed(0, 0, 5), changed(0, 1, -1),
                changed(2, 3, 1.5), twice, changed(1, 4, -0.25), changed(1, 5, float("nan")), changed(1, 6, float("inf")),
                changed(0, 7, 256), changed(0, 7, -1), changed(0, 7, 3.5)):
        with pytest.raises(ValueError):
            augment.check_color_jitter(bad, 3)
    augment.check_lighting(torch.zeros(3, 3), 3)
    for bad in (torch.zeros(2, 3), torch.zeros(3, 3, dtype=torch.float64), torch.full((3, 3), float("nan")), [[0.0] * 3] * 3):
        with pytest.raises(ValueError):
            augment.check_lighting(bad, 3)


# ---- lighting: the PCA and the draws ----

def test_rgb_pca_agrees_with_numpy_eigh_of_the_float64_covariance():
    from video_analytics_amd import augment
    x = torch.from_numpy(np.random.RandomState(6).randint(0, 256, size=(5, 3, 24, 40)).astype(np.uint8))
    x[:, 1] = (x[:, 0] // 2 + x[:, 1] // 2)  # correlated channels
    check_rgb_pca(x, *augment.rgb_pca(x))
    with pytest.raises(ValueError):
        augment.rgb_pca(x.float())


def check_rgb_pca(x, val, vec):
    """(val, vec) = rgb_pca(x) against numpy.linalg.eigh of the float64 covariance, within 1e-9 relative."""
    px = x.cpu().numpy().astype(np.float64).transpose(1, 0, 2, 3).reshape(3, -1)
    cov = np.cov(px, bias=True)
    w, v = np.linalg.eigh(cov)
    assert val.dtype == torch.float64 and vec.dtype == torch.float64 and tuple(val.shape) == (3,) and tuple(vec.shape) == (3, 3)
    assert np.allclose(val.numpy(), w, rtol=1e-9, atol=0)
    for j in range(3):  # an eigenvector's sign is free
        a, b = vec.numpy()[:, j], v[:, j]
        assert min(np.abs(a - b).max(), np.abs(a + b).max()) <= 1e-9
    assert np.allclose(vec.numpy() @ np.diag(val.numpy()) @ vec.numpy().T, cov, rtol=1e-9, atol=1e-9 * np.abs(cov).max())


def test_draw_lighting_draws_three_gaussians_per_image_in_order():
    from video_analytics_amd import augment
    val = torch.tensor([3.0, 40.0, 900.0], dtype=torch.float64)
    vec = torch.tensor(np.linalg.qr(np.random.RandomState(2).standard_normal((3, 3)))[0])
    off = augment.draw_lighting(4, val, vec, alphastd=0.1, rng=random.Random(8))
    rng = random.Random(8)
    assert off.dtype == torch.float32 and tuple(off.shape) == (4, 3)
    for i in range(4):
        alpha = np.array([rng.gauss(0, 0.1) for _ in range(3)])
        want = vec.numpy() @ (alpha * val.numpy())
        assert np.allclose(off[i].numpy(), want, rtol=1e-6, atol=1e-6)
    assert float(augment.draw_lighting(2, val, vec, alphastd=0.0, rng=random.Random(1)).abs().max()) == 0.0


# ---- the golden file ----

def test_golden_file_equals_its_generator_and_the_numpy_ops():
    gen = golden_module()
    assert os.path.getsize(gen.OUT) < 256 * 1024
    want, got = np.load(gen.OUT), gen.compute()
    assert sorted(want.files) == sorted(got)
    for name in want.files:
        assert want[name].dtype == got[name].dtype and np.array_equal(want[name], got[name]), name
    assert sorted(tuple(int(c) for c in r[:4]) for r in want["table_5x7"]) == sorted(gen.ORDERS) and len(gen.ORDERS) == 24
    for h, w in gen.SIZES:
        nm, img = gen.name(h, w), gen.image(h, w)
        for i, row in enumerate(want["table_" + nm]):
            res = jitter_numpy(img, row)
            if nm in gen.STORED:
                assert np.array_equal(res, want["out_" + nm][i]), (nm, i)
            else:
                assert hashlib.sha256(res.tobytes()).digest() == want["sha_" + nm][i].tobytes(), (nm, i)
    for row, out in zip(want["table_placement"], want["out_placement"]):
        assert np.array_equal(jitter_numpy(gen.image(33, 61), row), out)
