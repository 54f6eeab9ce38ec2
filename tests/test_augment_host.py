"""Host side of the device crop and flip (video_analytics_amd/augment.py): the draw helpers replay the
random numbers of getTransforms()' RandomCrop(224) + RandomHorizontalFlip() (Sheet03/utils.py:143,145) draw for draw,
and every malformed crop table is refused before anything reaches the GPU."""
import random

import numpy as np
import pytest
import torch


def _crop_of(out, w):
    """{top, left, flip} read back from a transformed index image (img[y, x] = y*w + x)."""
    lo = int(out.min())
    return [lo // w, lo % w, int(int(out[0, 0]) != lo)]


def _host_crops(n, h, w):
    """What utils.RandomCrop(224) + utils.RandomHorizontalFlip() do to n index images, in order."""
    from video_analytics_amd import utils
    crop, flip = utils.RandomCrop(224), utils.RandomHorizontalFlip()
    img = (np.arange(h, dtype=np.int64)[:, None] * w + np.arange(w, dtype=np.int64)[None, :])
    rows = []
    for _ in range(n):
        out = flip(crop(img))
        assert out.shape == (224, 224)
        rows.append(_crop_of(out, w))
    return rows


@pytest.mark.parametrize("h,w", [(240, 320), (241, 321), (224, 224), (224, 300), (300, 224)])
def test_image_draws_replay_the_reference_transforms(h, w):
    from video_analytics_amd import augment
    random.seed(1234)
    ref = _host_crops(9, h, w)
    state = random.getstate()
    random.seed(1234)
    got = augment.draw_image_crops(9, h, w)
    assert got.dtype == torch.int32 and tuple(got.shape) == (9, 3)
    assert got.tolist() == ref
    assert random.getstate() == state


def test_exact_size_frames_draw_only_the_flip():
    from video_analytics_amd import augment
    random.seed(7)
    flips = [int(random.random() < 0.5) for _ in range(6)]
    random.seed(7)
    got = augment.draw_image_crops(6, 224, 224)
    assert got[:, :2].abs().sum() == 0 and got[:, 2].tolist() == flips


def test_flow_draws_follow_the_interleave_order():
    """TemporalDataset applies the transform to x_s, y_s, x_{s+1}, ... in that order (Sheet03/temporalModel.py:83,86),
    clip after clip: row b*2L + c of the table is channel c of clip b."""
    from video_analytics_amd import augment
    B, L = 3, 10
    random.seed(99)
    ref = []
    for _ in range(B):
        for _k in range(L):
            for _axis in ("x", "y"):
                ref.extend(_host_crops(1, 240, 320))
    state = random.getstate()
    random.seed(99)
    got = augment.draw_flow_crops(B, L, 240, 320)
    assert tuple(got.shape) == (B * 2 * L, 3) and got.tolist() == ref
    assert random.getstate() == state


def test_an_rng_argument_leaves_the_global_generator_alone():
    from video_analytics_amd import augment
    random.seed(3)
    state = random.getstate()
    a = augment.draw_flow_crops(2, 10, 241, 321, rng=random.Random(11))
    assert random.getstate() == state
    random.seed(11)
    assert a.tolist() == augment.draw_flow_crops(2, 10, 241, 321).tolist()


def test_shared_mode_draws_once_per_clip():
    from video_analytics_amd import augment
    random.seed(5)
    per_clip = augment.draw_image_crops(4, 240, 320)
    state = random.getstate()
    random.seed(5)
    got = augment.draw_flow_crops(4, 10, 240, 320, mode="shared").view(4, 20, 3)
    assert random.getstate() == state
    for b in range(4):
        assert (got[b] == per_clip[b]).all()


def test_center_mode_is_center_crop_without_draws():
    from video_analytics_amd import augment
    random.seed(8)
    state = random.getstate()
    for h, w, top, left in ((240, 320, 8, 48), (241, 321, 8, 48), (243, 326, 10, 51), (224, 224, 0, 0)):
        # int(round((h - 224) / 2)): Python's round, half to even (241: 8.5 -> 8; 243: 9.5 -> 10)
        rows = augment.draw_image_crops(3, h, w, mode="center").tolist()
        assert rows == [[top, left, 0]] * 3
        assert augment.draw_flow_crops(2, 10, h, w, mode="center").tolist() == [[top, left, 0]] * 40
    assert random.getstate() == state
    with pytest.raises(ValueError):
        augment.draw_flow_crops(1, 10, 240, 320, mode="ten_crop")
    with pytest.raises(ValueError):
        augment.draw_image_crops(1, 240, 320, mode="per_image")


def test_draw_clip_crops_draws_rgb_then_flow():
    from video_analytics_amd import augment
    random.seed(21)
    a = augment.draw_image_crops(3, 240, 320)
    b = augment.draw_flow_crops(3, 10, 256, 340)
    random.seed(21)
    ra, rb = augment.draw_clip_crops(3, 10, (240, 320), (256, 340))
    assert torch.equal(ra, a) and torch.equal(rb, b)


def test_host_validation_refuses_bad_crops():
    from video_analytics_amd import augment
    ok = augment.draw_image_crops(4, 240, 320)
    augment.check_crops(ok, 4, 240, 320, 224, "t")
    with pytest.raises(ValueError, match="smaller"):
        augment.draw_image_crops(1, 223, 320)
    with pytest.raises(ValueError, match="smaller"):
        augment.draw_flow_crops(1, 10, 240, 200)
    with pytest.raises(ValueError, match="smaller"):
        augment.check_crops(ok, 4, 240, 223, 224, "t")
    with pytest.raises(ValueError, match=r"\[4,3\]"):
        augment.check_crops(ok[:3], 4, 240, 320, 224, "t")
    with pytest.raises(ValueError, match=r"\[4,3\]"):
        augment.check_crops(ok[:, :2], 4, 240, 320, 224, "t")
    for bad in (ok.long(), ok.float(), ok.numpy()):
        with pytest.raises(ValueError, match="int32"):
            augment.check_crops(bad, 4, 240, 320, 224, "t")
    for row in ([17, 0, 0], [0, 97, 0], [-1, 0, 0], [0, -1, 1], [0, 0, 2], [0, 0, -1]):
        bad = ok.clone()
        bad[2] = torch.tensor(row, dtype=torch.int32)
        with pytest.raises(ValueError):
            augment.check_crops(bad, 4, 240, 320, 224, "t")
    edge = ok.clone()
    edge[0] = torch.tensor([16, 96, 1], dtype=torch.int32)  # the largest valid offsets
    augment.check_crops(edge, 4, 240, 320, 224, "t")


def test_torch_normalise_equals_ieee_single_arithmetic():
    """Both sides of the device/host comparisons evaluate (q/255 - m)/s as two IEEE single divisions: torch's
    ToTensor (div(255)) + Normalize on the CPU give numpy's float32 result for every u8 value."""
    from video_analytics_amd import utils
    from video_analytics_amd.parameters import NORM_MEANS_TF, NORM_STDS_TF
    q = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = np.stack([q, q, q], axis=-1)
    got = utils.Normalize(NORM_MEANS_TF, NORM_STDS_TF)(utils.ToTensor()(img)).numpy()
    for c in range(3):
        ref = (q.astype(np.float32) / np.float32(255) - np.float32(NORM_MEANS_TF[c])) / np.float32(NORM_STDS_TF[c])
        assert got[c].dtype == np.float32 and np.array_equal(got[c], ref), c
