"""Host side of ten-crop evaluation: the view table of augment.ten_crop_views against torchvision's
TenCrop order, utils.getTenCropTransforms against an explicit numpy restatement (slice, mirror, 255 - q on mirrored
x-flow images, ToTensor, Normalize), the datasets' ten-view samples, and the refusal of malformed view tables."""
import random

import numpy as np
import pytest
import torch


def _table(h, w, s=224):
    """The issue's table written out: five_crop of the image, then five_crop of its mirror, in frame coordinates."""
    ct, cl = int(round((h - s) / 2.0)), int(round((w - s) / 2.0))
    b, r = h - s, w - s
    return [[0, 0, 0], [0, r, 0], [b, 0, 0], [b, r, 0], [ct, cl, 0],
            [0, r, 1], [0, 0, 1], [b, r, 1], [b, 0, 1], [ct, r - cl, 1]]


def test_ten_crop_views_of_the_worked_cases():
    from video_analytics_amd import augment
    v = augment.ten_crop_views(240, 320)
    assert v.dtype == torch.int32 and tuple(v.shape) == (10, 3)
    assert v.tolist() == [[0, 0, 0], [0, 96, 0], [16, 0, 0], [16, 96, 0], [8, 48, 0],
                          [0, 96, 1], [0, 0, 1], [16, 96, 1], [16, 0, 1], [8, 48, 1]]
    assert augment.ten_crop_views(224, 224).tolist() == [[0, 0, f] for f in (0,) * 5 + (1,) * 5]
    odd = augment.ten_crop_views(225, 321).tolist()  # w - s = 97, h - s = 1
    assert odd[4] == [0, 48, 0] and odd[9] == [0, 49, 1]
    assert odd == _table(225, 321)


@pytest.mark.parametrize("h,w", [(240, 320), (241, 321), (224, 300), (300, 224), (256, 340)])
def test_view_four_is_the_center_crop_and_nothing_is_drawn(h, w):
    from video_analytics_amd import augment
    random.seed(99)
    state = random.getstate()
    v = augment.ten_crop_views(h, w)
    assert random.getstate() == state
    assert v.tolist() == _table(h, w)
    assert v[4].tolist() == augment.draw_image_crops(1, h, w, mode="center")[0].tolist()
    assert random.getstate() == state


def test_mirrored_views_are_the_mirror_images_five_crop():
    """View 5 + i of the image is view i of the mirrored image, mirrored back (torchvision's TenCrop)."""
    from video_analytics_amd import augment
    h, w = 241, 321
    img = np.arange(h * w, dtype=np.int64).reshape(h, w)
    mir = img[:, ::-1]
    v = augment.ten_crop_views(h, w).tolist()
    for i in range(5):
        top, left, _ = v[i]
        want = mir[top:top + 224, left:left + 224]  # five_crop of the mirror
        t2, l2, f2 = v[5 + i]
        got = img[t2:t2 + 224, l2:l2 + 224][:, ::-1]
        assert f2 == 1 and np.array_equal(got, want), i


def test_expand_views_row_order():
    from video_analytics_amd import augment
    v = augment.ten_crop_views(240, 320)
    rows = augment.expand_views(v, 3, 4)
    assert tuple(rows.shape) == (3 * 10 * 4, 3) and rows.dtype == torch.int32
    for o in range(rows.shape[0]):
        assert rows[o].tolist() == v[(o // 4) % 10].tolist()
    assert torch.equal(augment.expand_views(v, 2), torch.cat([v, v]))


def _restated(a, flowX, invert, means, stds):
    """utils.getTenCropTransforms restated: slice, mirror, 255 - q on mirrored x-flow images, ToTensor, Normalize."""
    from video_analytics_amd import augment, utils
    out = []
    for top, left, flip in augment.ten_crop_views(a.shape[0], a.shape[1]).tolist():
        v = a[top:top + 224, left:left + 224]
        if flip:
            v = v[:, ::-1]
            if flowX and invert:
                v = 255 - v
        out.append(utils.Normalize(means, stds)(utils.ToTensor()(np.ascontiguousarray(v))))
    return torch.stack(out)


def test_ten_crop_transform_equals_the_numpy_restatement():
    from PIL import Image
    from video_analytics_amd import utils
    from video_analytics_amd.parameters import NORM_MEANS_TF, NORM_STDS_TF
    rs = np.random.RandomState(4)
    rgb = rs.randint(0, 256, (240, 320, 3)).astype(np.uint8)
    fx = rs.randint(0, 256, (241, 321)).astype(np.uint8)
    random.seed(5)
    state = random.getstate()
    for invert in (False, True):
        tf = utils.getTenCropTransforms(NORM_MEANS_TF, NORM_STDS_TF, invertFlowX=invert)
        assert tf.nViews == 10
        got = tf(Image.fromarray(rgb))
        assert got.dtype == torch.float32 and tuple(got.shape) == (10, 3, 224, 224)
        assert torch.equal(got, _restated(rgb, False, invert, NORM_MEANS_TF, NORM_STDS_TF))
        for flowX in (False, True):
            got = tf(Image.fromarray(fx, mode="L"), flowX=flowX)
            assert tuple(got.shape) == (10, 1, 224, 224)
            assert torch.equal(got, _restated(fx, flowX, invert, NORM_MEANS_TF, NORM_STDS_TF))
    assert random.getstate() == state
    # the inversion touches exactly the mirrored views of x-flow images
    plain = utils.getTenCropTransforms()(fx, flowX=True)
    inv = utils.getTenCropTransforms(invertFlowX=True)(fx, flowX=True)
    assert torch.equal(plain[:5], inv[:5]) and not torch.equal(plain[5], inv[5])
    q = fx[0:224, 97:321][:, ::-1]  # view 5: top 0, left w - s, mirrored
    assert torch.equal(inv[5, 0], (torch.from_numpy((255 - q).astype(np.float32)) / 255 - 0.485) / 0.229)
    assert torch.equal(utils.getTenCropTransforms(invertFlowX=True)(fx, flowX=False), plain)


def _tree(tmp_path, L):
    from PIL import Image
    from video_analytics_amd import utils as U
    lines = ["ApplyEyeMakeup/v_ApplyEyeMakeup_g01_c01.avi\n", "ApplyEyeMakeup/v_ApplyEyeMakeup_g01_c02.avi\n",
             "Archery/v_Archery_g01_c01.avi\n"]
    lst = tmp_path / "list.txt"
    lst.write_text("".join(lines))
    (tmp_path / "classInd.txt").write_text("1 ApplyEyeMakeup\n2 ApplyLipstick\n3 Archery\n")
    rng = np.random.default_rng(0)
    for line in lines:
        _, name, _, cat, _, _ = U.videoInfo(line, "test")
        fd = tmp_path / "frames" / cat / name
        fd.mkdir(parents=True)
        for i in range(2):
            Image.fromarray(rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)).save(str(fd / ("%d.jpg" % i)), quality=90)
        od = tmp_path / "flows" / cat / name
        od.mkdir(parents=True)
        for k in range(1, L + 2):
            for prefix in ("flow_x_", "flow_y_"):
                Image.fromarray(rng.integers(0, 256, (240, 320), dtype=np.uint8), mode="L").save(
                    str(od / U.flowFileName(prefix, k)), quality=90)
    return str(lst), str(tmp_path / "classInd.txt")


def test_datasets_give_ten_views_and_keep_the_interleave(tmp_path):
    from PIL import Image
    from video_analytics_amd import utils as U
    from video_analytics_amd.spatialModel import SpatialDataset
    from video_analytics_amd.temporalModel import TemporalDataset
    L = 3
    lst, cl = _tree(tmp_path, L)
    tf = U.getTenCropTransforms(invertFlowX=True)
    sds = SpatialDataset(lst, str(tmp_path / "frames"), tf, mode="test", actionLabelLoc=cl)
    x, label, name = sds[0]
    assert tuple(x.shape) == (10, 3, 224, 224) and label == 1 and name == "v_ApplyEyeMakeup_g01_c01"
    tds = TemporalDataset(lst, str(tmp_path / "flows"), tf, flowSampleSize=L, mode="test", actionLabelLoc=cl)
    random.seed(3)
    vol, label, name = tds[2]
    assert tuple(vol.shape) == (10, 2 * L, 224, 224) and label == 3 and name == "v_Archery_g01_c01"
    random.seed(3)
    start, order = U.temporalFlowIndices(2 * (L + 1), L)
    d = tmp_path / "flows" / "Archery" / "v_Archery_g01_c01"
    for c, (ax, idx) in enumerate(order):  # x_s, y_s, x_{s+1}, ...: channel 2k is x flow
        assert (c % 2 == 0) == (ax == "x")
        img = Image.open(str(d / U.flowFileName("flow_%s_" % ax, idx)))
        assert torch.equal(vol[:, c], tf(img, flowX=(ax == "x"))[:, 0]), c
    loader = U.getDataLoader(tds, batchSize=2, nWorkers=0, shuffle=False)
    shapes = [tuple(b.shape) for b, _, _ in loader]
    assert shapes == [(2, 10, 2 * L, 224, 224), (1, 10, 2 * L, 224, 224)]
    loader = U.getDataLoader(sds, batchSize=3, nWorkers=0, shuffle=False)
    assert [tuple(b.shape) for b, _, _ in loader] == [(3, 10, 3, 224, 224)]


@pytest.mark.parametrize("bad", [
    [[0, 0, 0]],                                              # not a tensor
    torch.zeros(10, 3, dtype=torch.int64),                    # wrong dtype
    torch.zeros(10, 2, dtype=torch.int32),                    # wrong width
    torch.zeros(0, 3, dtype=torch.int32),                     # no view
    torch.zeros(2, 10, 3, dtype=torch.int32),                 # not 2-d
    torch.tensor([[17, 0, 0]], dtype=torch.int32),            # top beyond h - 224
    torch.tensor([[0, 97, 0]], dtype=torch.int32),            # left beyond w - 224
    torch.tensor([[0, -1, 0]], dtype=torch.int32),            # negative offset
    torch.tensor([[0, 0, 2]], dtype=torch.int32),             # flip not 0 / 1
])
def test_malformed_view_tables_are_refused(bad):
    from video_analytics_amd import augment
    with pytest.raises(ValueError):
        augment.check_views(bad, 240, 320, 224, "test")


def test_view_table_of_a_frame_smaller_than_the_crop_is_refused():
    from video_analytics_amd import augment
    with pytest.raises(ValueError):
        augment.ten_crop_views(223, 320)
    with pytest.raises(ValueError):
        augment.check_views(augment.ten_crop_views(240, 320), 200, 320, 224, "test")
