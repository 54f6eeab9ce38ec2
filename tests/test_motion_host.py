"""Host side of the motion inputs: the gray-frame reordering of bi-directional flow, the refusal of bad
motion options before anything reaches the GPU, and the numpy float32 restatements of S11 (field means) and S12 (trajectory
stacking, mean subtraction) that tests/test_motion_gpu.py holds the kernels to, checked here against independent float64
witnesses (math.fsum; scipy.ndimage.map_coordinates)."""
import math

import numpy as np
import pytest
import torch

F32 = np.float32


def s11_means(flow):
    """S11 restated: flow float32 [N,2,h,w] -> float32 [N,2].  Clamp to [-32768, 32768] (a NaN becomes -32768), scale by
    2^16 to an exact integer, sum in int64, divide once in float64, round to float32."""
    N, _, h, w = flow.shape
    a = np.fmin(np.fmax(flow, F32(-32768.0)), F32(32768.0))
    q = np.rint(a * F32(65536.0)).astype(np.int64)
    s = q.reshape(N, 2, h * w).sum(axis=2, dtype=np.int64)
    return (s.astype(np.float64) / (np.float64(h * w) * 65536.0)).astype(np.float32)


def s12_bilinear(f, px, py):
    """S12's bilinear sample of plane f [h,w] at float32 positions, in float32 with every product rounded on its own."""
    h, w = f.shape
    xc = np.fmin(np.fmax(px, F32(0.0)), F32(w - 1))
    yc = np.fmin(np.fmax(py, F32(0.0)), F32(h - 1))
    x0 = np.floor(xc).astype(np.int64)
    y0 = np.floor(yc).astype(np.int64)
    x1 = np.minimum(x0 + 1, w - 1)
    y1 = np.minimum(y0 + 1, h - 1)
    ax = xc - x0.astype(np.float32)
    ay = yc - y0.astype(np.float32)
    a, b, c, d = f[y0, x0], f[y0, x1], f[y1, x0], f[y1, x1]
    top = a + ax * (b - a)
    bot = c + ax * (d - c)
    return top + ay * (bot - top)


def s12_motion(flow, chain_len, trajectory, means=None):
    """S12 restated: flow float32 [N,2,h,w] of chains of chain_len pairs -> float32 of the same shape."""
    flow = np.asarray(flow, dtype=np.float32)
    N, _, h, w = flow.shape
    if not trajectory:
        return flow - means[:, :, None, None]
    out = np.empty_like(flow)
    for b in range(N // chain_len):
        py, px = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
        for k in range(chain_len):
            n = b * chain_len + k
            dx = s12_bilinear(flow[n, 0], px, py)
            dy = s12_bilinear(flow[n, 1], px, py)
            out[n, 0] = dx if means is None else dx - means[n, 0]
            out[n, 1] = dy if means is None else dy - means[n, 1]
            px = px + dx
            py = py + dy
    return out


def _trajectory_f64(flow, chain_len):
    """Independent float64 witness of trajectory stacking: scipy's linear interpolation with edge replication."""
    from scipy.ndimage import map_coordinates
    flow = flow.astype(np.float64)
    N, _, h, w = flow.shape
    out = np.empty_like(flow)
    for b in range(N // chain_len):
        py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        for k in range(chain_len):
            n = b * chain_len + k
            d = [map_coordinates(flow[n, c], [py, px], order=1, mode="nearest") for c in (0, 1)]
            out[n, 0], out[n, 1] = d
            px, py = px + d[0], py + d[1]
    return out


def smooth_flow(N, h, w, phase=0.0):
    """A smooth fractional field: 1.5 + 3 sin(x/9 + n) in x, -0.75 + 2 cos(y/7 + x/22 + n) in y (trajectories stay smooth)."""
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    fl = np.empty((N, 2, h, w), dtype=np.float32)
    for n in range(N):
        fl[n, 0] = 1.5 + 3.0 * np.sin(x / 9.0 + n + phase)
        fl[n, 1] = -0.75 + 2.0 * np.cos(y / 7.0 + 0.5 * x / 11.0 + n + phase)
    return fl


# ---- S13: the gray frames of bi-directional flow ----

@pytest.mark.parametrize("L", [2, 4, 10])
def test_bidirectional_sequences_are_forward_then_backward_from_tau(L):
    from video_analytics_amd import flow as vflow
    B, H, W = 3, 5, 7
    gray = torch.arange(B * (L + 1), dtype=torch.float32).view(B, L + 1, 1, 1).expand(B, L + 1, H, W).contiguous()
    seq = vflow.bidirectional_sequences(gray)
    h = L // 2
    assert tuple(seq.shape) == (2 * B, h + 1, H, W) and seq.dtype == gray.dtype
    for b in range(B):
        fwd = seq[2 * b, :, 0, 0].tolist()
        bwd = seq[2 * b + 1, :, 0, 0].tolist()
        base = b * (L + 1)
        assert fwd == [base + h + j for j in range(h + 1)]   # tau ... tau + L/2
        assert bwd == [base + h - j for j in range(h + 1)]   # tau ... tau - L/2
        assert torch.equal(seq[2 * b + 1], gray[b, :h + 1].flip(0))
    u8 = vflow.bidirectional_sequences(gray.to(torch.uint8))
    assert u8.dtype == torch.uint8 and torch.equal(u8.float(), seq)


@pytest.mark.parametrize("F", [2, 4, 1])
def test_bidirectional_sequences_refuse_an_odd_number_of_pairs(F):
    from video_analytics_amd import flow as vflow
    with pytest.raises(ValueError):
        vflow.bidirectional_sequences(torch.zeros(2, F, 4, 4))
    with pytest.raises(ValueError):
        vflow.bidirectional_sequences(torch.zeros(3, 4, 4))


# ---- option checks: before anything reaches the GPU ----

@pytest.fixture
def no_gpu_calls(monkeypatch):
    """Every path to the device raises AssertionError: a ValueError seen with it comes from a host check."""
    from video_analytics_amd import _ffi
    from video_analytics_amd import flow as vflow

    def boom(*a, **k):
        raise AssertionError("reached the GPU")
    for mod, name in ((_ffi, "ctx"), (_ffi, "lib"), (vflow, "tvl1_flow"), (vflow, "tvl1_flow_concurrent")):
        monkeypatch.setattr(mod, name, boom)


@pytest.mark.parametrize("kw", [dict(motion="optical"), dict(motion="trajectory+bidirectional"),
                                dict(motion=("trajectory", "bidirectional")), dict(motion=None),
                                dict(motion="stack", mean_flow="yes"), dict(motion="bidirectional", L=9),
                                dict(motion="bidirectional", L=1)])
def test_flow_volumes_refuse_bad_motion_options_on_the_host(no_gpu_calls, kw):
    from video_analytics_amd import augment
    from video_analytics_amd.temporalModel import flowVolumesFromFrames
    kw = dict(kw)
    L = kw.pop("L", 10)
    gray = torch.zeros(2, L + 1, 240, 320, dtype=torch.uint8)
    for extra in (dict(), dict(views=augment.ten_crop_views(240, 320)), dict(invert_flow_x=True)):
        with pytest.raises(ValueError):
            flowVolumesFromFrames(gray, flowSampleSize=L, **kw, **extra)


def test_trajectory_with_bidirectional_is_named_in_the_error(no_gpu_calls):
    from video_analytics_amd import flow as vflow
    with pytest.raises(ValueError, match="bi-directional"):
        vflow.check_motion("trajectory+bidirectional", False, 10, "x")
    for ok in ("stack", "trajectory", "bidirectional"):
        vflow.check_motion(ok, True, 10, "x")
        vflow.check_motion(ok, False, 10, "x")


def test_flow_helpers_refuse_bad_arguments_on_the_host(no_gpu_calls):
    from video_analytics_amd import flow as vflow
    cpu = torch.zeros(4, 2, 8, 8)
    for f in (lambda: vflow.flow_field_means(cpu), lambda: vflow.motion_field(cpu, 2, trajectory=True),
              lambda: vflow.flow_field_means(torch.zeros(4, 3, 8, 8))):
        with pytest.raises(ValueError):
            f()


# ---- S12 restated ----

def test_s12_restatement_is_the_identity_on_zero_flow():
    fl = np.zeros((6, 2, 9, 13), dtype=np.float32)
    for L in (1, 3, 6):
        out = s12_motion(fl, L, True)
        assert np.array_equal(out, fl) and not np.signbit(out).any()
    m = np.zeros((6, 2), dtype=np.float32)
    assert np.array_equal(s12_motion(fl, 3, False, m), fl)


def test_s12_restatement_returns_the_raw_field_at_the_first_pair():
    rs = np.random.RandomState(0)
    fl = (rs.standard_normal((10, 2, 17, 23)) * 12).astype(np.float32)
    out = s12_motion(fl, 5, True)
    assert np.array_equal(out[0::5], fl[0::5])
    assert not np.array_equal(out[1::5], fl[1::5])
    m = s11_means(fl)
    sub = s12_motion(fl, 5, True, m)
    assert np.array_equal(sub, out - m[:, :, None, None])
    assert np.array_equal(s12_motion(fl, 5, False, m), fl - m[:, :, None, None])


def test_s12_restatement_follows_an_integer_translation_and_clamps_at_the_border():
    """A uniform (+1, 0) px field: after k pairs the trajectory of x is at x + k, clamped to w - 1 -- whose sample is 1."""
    N, h, w = 4, 3, 6
    fl = np.zeros((N, 2, h, w), dtype=np.float32)
    fl[:, 0] = 1.0
    fl[2, 0, :, 4:] = 5.0  # pair 2 reads x + 2: the columns x = 2, 3 and the clamped ones
    out = s12_motion(fl, N, True)
    for x in range(w):
        assert out[2, 0, 0, x] == (5.0 if min(x + 2, w - 1) >= 4 else 1.0), x


@pytest.mark.parametrize("h,w,L", [(48, 64, 10), (24, 31, 5)])
def test_s12_restatement_agrees_with_a_float64_witness_on_smooth_fields(h, w, L):
    fl = smooth_flow(2 * L, h, w)
    got = s12_motion(fl, L, True).astype(np.float64)
    ref = _trajectory_f64(fl, L)
    assert np.abs(got - ref).max() < 1e-4, np.abs(got - ref).max()
    # the trajectories really move (and leave the frame): pair L-1 differs from the flow sampled in place
    assert np.abs(got[L - 1] - fl[L - 1]).max() > 0.5


# ---- S11 restated ----

def test_s11_restatement_agrees_with_fsum_and_clamps():
    rs = np.random.RandomState(3)
    h, w = 37, 53
    fl = (rs.standard_normal((3, 2, h, w)) * 12).astype(np.float32)
    fl[0, 0, 5, 7] = 1e5
    fl[0, 1, 9, 11] = -1e5
    fl[1, 0, :4] = 2.5e4
    fl[2, 1] = F32(-0.7)  # a constant plane
    m = s11_means(fl)
    assert m.dtype == np.float32 and m.shape == (3, 2)
    for n in range(3):
        for c in range(2):
            v = np.clip(fl[n, c].astype(np.float64), -32768.0, 32768.0).ravel()
            ref = math.fsum(v.tolist()) / v.size
            tol = 2.0 ** -17 + float(np.spacing(np.float32(abs(ref))))
            assert abs(float(m[n, c]) - ref) <= tol, (n, c, float(m[n, c]), ref)
    assert m[2, 1] == F32(-0.7) or abs(float(m[2, 1]) + 0.7) <= 2.0 ** -17  # within the fixed point's resolution
    nan = fl.copy()
    nan[0, 0, 0, 0] = np.nan
    ref = fl.copy()
    ref[0, 0, 0, 0] = -32768.0
    assert np.array_equal(s11_means(nan), s11_means(ref))
