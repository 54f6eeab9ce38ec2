"""The JPEG kernels on hand-built streams: jpeg.decode_jpegs against PIL's recorded pixels
(tests/golden/jpeg_streams.npz) bit for bit on every case of tests/golden/make_jpeg_streams_golden.py -- the writer's own counts
assert there that each case reaches its code lengths, bit phases, segment tails, magnitudes and runs -- batches with three
table sets and with one under different restart intervals, and the status contract by construction: which bit each fault
sets, that a segment used to its last bit is clean and one byte less is not, that a bad segment or image leaves its
neighbours alone, and that every bad row of the segment table is refused before it is followed.
tests/test_jpeg_streams_host.py holds the host model to the same files."""
import numpy as np
import pytest
import torch

from test_jpeg_streams_host import GEN, GOLDEN, STATUS

pytestmark = pytest.mark.gpu


def _decode(datas, **kw):
    from video_analytics_amd import jpeg
    out, status = jpeg.decode_jpegs(datas, "cuda", **kw)
    assert status.dtype == torch.int32 and tuple(status.shape) == (len(datas),) and status.is_cuda
    return out, status


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_decode_equals_pil_bit_for_bit(name):
    data, want = GOLDEN[name]
    out, status = _decode([data], check=False)
    assert int(status[0]) == 0
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1,) + want.shape and out.is_contiguous()
    got = out[0].cpu().numpy()
    assert np.array_equal(got, want), "%d values differ from the recorded pixels" % int((got != want).sum())
    assert np.array_equal(got, GEN.pil_pixels(data)), "differs from this machine's PIL"


@pytest.mark.parametrize("prefix,sets", [("sets", 3), ("one", 1)])
def test_batches_of_three_table_sets_and_of_one_with_different_restart_intervals(prefix, sets):
    from video_analytics_amd import jpeg
    datas = [GOLDEN["%s_%d" % (prefix, i)][0] for i in range(3)]
    want = np.stack([GOLDEN["%s_%d" % (prefix, i)][1] for i in range(3)])
    hdrs = [jpeg.parse_jpeg(d) for d in datas]
    assert jpeg.pack_jpegs(hdrs)[2] == sets  # three sets: tables from global memory; one: staged in LDS
    assert len({h["restart_interval"] for h in hdrs}) == 3
    out, status = _decode(datas, check=False)
    assert not status.any() and np.array_equal(out.cpu().numpy(), want)
    flat = torch.full((want.size + 1,), 9, dtype=torch.uint8, device="cuda")
    out, status = _decode(datas, out=flat[1:].view(want.shape), check=False)  # one byte past an aligned address: byte stores
    assert out.data_ptr() == flat.data_ptr() + 1 and not status.any()
    assert np.array_equal(out.cpu().numpy(), want) and int(flat[0]) == 9


def test_gray_streams_into_an_unaligned_out():
    for name in ("phases_gray_32x64", "runs_gray_32x56", "tails_gray_8x64"):
        data, want = GOLDEN[name]
        flat = torch.full((want.size + 1,), 9, dtype=torch.uint8, device="cuda")
        out, status = _decode([data], out=flat[1:].view((1,) + want.shape), check=False)
        assert int(status[0]) == 0 and np.array_equal(out[0].cpu().numpy(), want) and int(flat[0]) == 9, name


# ---- the status, by construction (make_jpeg_streams_golden.status_streams) ----

@pytest.mark.parametrize("name", sorted(STATUS))
def test_each_fault_sets_its_one_bit(name):
    """Sixteen 1-bits where a code is due: bad code; three ZRLs and run 15: bad run; a segment that ends on its last bit: clean;
    the same without its last byte: out of bits.  The tables give the zero bits behind the segment's end the codes of
    category 0 and EOB, so nothing else can be set."""
    data, want = STATUS[name]
    out, status = _decode([data], check=False)
    assert int(status[0]) == want
    if want == 0:
        assert np.array_equal(out[0].cpu().numpy(), GEN.pil_pixels(data))
    else:
        with pytest.raises(ValueError, match="image 0 did not decode"):
            _decode([data])


@pytest.mark.parametrize("name", [n for n in sorted(STATUS) if STATUS[n][1] != 0])
def test_a_corrupt_image_leaves_its_neighbours_alone(name):
    if name.startswith("rows"):
        outer = [STATUS["rows_good"][0], STATUS["rows_good"][0]]
        want = GEN.pil_pixels(outer[0])
        want = [want, want]
    else:
        outer = [STATUS["exact"][0], GOLDEN["ac256_gray_8x16"][0]]  # 8x16 gray like the corrupt one; another table set
        want = [GEN.pil_pixels(outer[0]), GOLDEN["ac256_gray_8x16"][1]]
    out, status = _decode([outer[0], STATUS[name][0], outer[1]], check=False)
    assert status.cpu().tolist() == [0, STATUS[name][1], 0]
    assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[2].cpu().numpy(), want[1])


@pytest.mark.parametrize("name", ["rows_bad_code", "rows_bad_run"])
def test_a_corrupt_segment_leaves_the_other_segments_of_its_image_alone(name):
    """Gray 24x24 with a restart per MCU row (no upsampling crosses the rows): the middle segment is corrupt in its second
    block; the block rows of the other two segments are the intact file's."""
    good = GEN.pil_pixels(STATUS["rows_good"][0])
    out, status = _decode([STATUS[name][0]], check=False)
    got = out[0].cpu().numpy()
    assert int(status[0]) == STATUS[name][1]
    assert np.array_equal(got[:8], good[:8]) and np.array_equal(got[16:], good[16:])


# ---- bad rows of the segment table: refused before anything is read through them ----

def _packed_batch(prefix):
    """The packed upload of a batch of three (7 segments: 4 + 2 + 1 or 2 + 1 + 4) with its tables as writable int32 views."""
    from video_analytics_amd import jpeg
    hdrs = [jpeg.parse_jpeg(GOLDEN["%s_%d" % (prefix, i)][0]) for i in range(3)]
    packed, nseg, nsets = jpeg.pack_jpegs(hdrs)
    buf = np.frombuffer(packed, dtype=np.uint8).copy()
    off_seg = 48  # three image rows of 16 bytes
    off_data = off_seg + 32 * nseg + nsets * jpeg.SET_BYTES
    img = buf[:48].view(np.int32).reshape(3, 4)
    seg = buf[off_seg:off_seg + 32 * nseg].view(np.int32).reshape(nseg, 8)
    assert nseg == 7 and img[:, 2].tolist() == [len(h["segments"]) for h in hdrs] and (seg[:, 1] % 4 == 0).all()
    return buf, img, seg, len(buf) - off_data, nseg, nsets, hdrs[0]["mcus"]


def _launch(buf, nseg, nsets):
    from video_analytics_amd import jpeg
    device = torch.device("cuda", torch.cuda.current_device())
    out = torch.full((3, 3, 19, 30), 7, dtype=torch.uint8, device=device)
    status = torch.full((3,), -1, dtype=torch.int32, device=device)
    jpeg.launch(jpeg.upload(buf.tobytes(), device), (3, 30, 19, 3, 2, 2), nseg, nsets, out, status)
    return out.cpu().numpy(), status.cpu().tolist()


POKES = {
    "an offset that is no multiple of 4": lambda row, data_bytes, mcus: row.__setitem__(1, row[1] + 2),
    "a negative offset": lambda row, data_bytes, mcus: row.__setitem__(1, -4),
    "a negative byte count": lambda row, data_bytes, mcus: row.__setitem__(2, -1),
    "the most negative byte count": lambda row, data_bytes, mcus: row.__setitem__(2, -2 ** 31),
    "a length one byte past the data": lambda row, data_bytes, mcus: row.__setitem__(2, data_bytes - row[1] + 1),
    "the largest length": lambda row, data_bytes, mcus: row.__setitem__(2, 2 ** 31 - 1),
    "an offset at the end of the data": lambda row, data_bytes, mcus: row.__setitem__(1, data_bytes),
    "first + count one past the MCUs": lambda row, data_bytes, mcus: row.__setitem__(4, mcus - row[3] + 1),
    "the largest count": lambda row, data_bytes, mcus: row.__setitem__(4, 2 ** 31 - 1),
    "a negative first MCU": lambda row, data_bytes, mcus: row.__setitem__(3, -1),
    "a negative count": lambda row, data_bytes, mcus: row.__setitem__(4, -1),
}


@pytest.mark.parametrize("prefix", ["sets", "one"])
@pytest.mark.parametrize("poke", sorted(POKES))
def test_a_bad_segment_row_is_refused_and_named(prefix, poke):
    """Every value poked here is one k_jpeg_entropy compares before it forms an address from it.  The row is the LAST segment
    of the middle image: that image reports exactly STATUS_BAD_SEGMENT, the other two decode."""
    from video_analytics_amd import jpeg
    buf, img, seg, data_bytes, nseg, nsets, mcus = _packed_batch(prefix)
    row = seg[int(img[1, 1] + img[1, 2] - 1)]
    assert row[0] == 1
    before = row.copy()
    POKES[poke](row, data_bytes, mcus)
    assert (row != before).sum() == 1
    out, status = _launch(buf, nseg, nsets)
    assert status == [0, jpeg.STATUS_BAD_SEGMENT, 0]
    for i in (0, 2):
        assert np.array_equal(out[i], GOLDEN["%s_%d" % (prefix, i)][1]), i


@pytest.mark.parametrize("prefix", ["sets", "one"])
def test_a_table_set_index_past_the_sets_is_refused(prefix):
    from video_analytics_amd import jpeg
    buf, img, seg, data_bytes, nseg, nsets, mcus = _packed_batch(prefix)
    for bad in (nsets, -1):
        img[1, 0] = bad
        out, status = _launch(buf, nseg, nsets)
        assert status == [0, jpeg.STATUS_BAD_SEGMENT, 0], bad
        for i in (0, 2):
            assert np.array_equal(out[i], GOLDEN["%s_%d" % (prefix, i)][1]), (bad, i)


@pytest.mark.parametrize("prefix", ["sets", "one"])
def test_a_segment_of_no_image_reports_nowhere(prefix):
    """A segment row whose image index is n (or negative) has no status word to report to: nothing is set and the other
    images are whole; its own image misses that segment's blocks, which is all that differs."""
    buf, img, seg, data_bytes, nseg, nsets, mcus = _packed_batch(prefix)
    whole, clean = _launch(buf, nseg, nsets)
    assert clean == [0, 0, 0] and all(np.array_equal(whole[i], GOLDEN["%s_%d" % (prefix, i)][1]) for i in range(3))
    for bad in (3, -1):
        seg[int(img[1, 1]), 0] = bad
        out, status = _launch(buf, nseg, nsets)
        assert status == [0, 0, 0], bad
        assert np.array_equal(out[0], whole[0]) and np.array_equal(out[2], whole[2]) and not np.array_equal(out[1], whole[1])
