"""Every conv kernel instantiation of the model's dispatch, one layer at a time, against a float64 reference.

``va_conv3x3_layer`` (include/va.h, testing entry points) runs ONE 3x3 conv layer through ``launch_conv_ex`` (fp32) /
``launch_conv_bf16`` (bf16) -- the code the forward pass and the training step use -- and reports the kernel
instantiation it launched.  Each case of ``CASES`` names the instantiation it must reach, so a change of the dispatch
fails here instead of silently dropping a kernel out of coverage; together the cases reach all 29 instantiations of a
default build (``INSTANTIATIONS``; ``test_every_launched_kernel_family_has_layer_cases`` scans vgg.hip for new families).

Reference: the same layer in float64 (``F.unfold`` + a float64 matmul, on the GPU for the 224 x 224 cases), with the
magnitude sum S = sum |x w| + |b| of every output.  bf16 operands are rounded to bf16 first, so every product is exact and
the reference answers the same question exactly.  Per case:
  * fp32 output: r = |got - ref| / (2^-24 S) stays below C_F32 (fp32 accumulation of exact products: a lost product,
    tap or K chunk gives r in the thousands);
  * bf16 output: |got - ref| <= ulp_bf16(|ref| + d) / 2 + d, d = C_F32 2^-24 S (fp32 accumulation, then ONE rounding);
  * ReLU zeros are exact zeros (where the pre-activation is below -d), and so are masked outputs;
  * no stray writes: ``out`` starts as NaN between canary blocks, ``in`` sits between NaN guard blocks (the bf16 kernels
    address it through buffer resources that start before it); afterwards every output is finite and the canaries hold;
  * two launches give bit-identical outputs, and kernels that add the same products in the same order agree bit for bit
    (the ``runs`` of a case: e.g. bf16 variants 0, 1, 2, 5, 7 on a layer with 64 input channels).

Findings pinned here:
  * k_conv3x3_img14 staged its epilogue tile in brick buffer 0, which with an ODD number of K chunks is the last chunk's
    buffer, read by the other computing waves without a barrier in between (a race).  It now stages in the buffer the
    last chunk did not use; the odd-chunk cases (fp32 cin 32 / 96, bf16 cin 64 / 192, no pooling) hold that.
  * Pooling with an odd hw: the pooling epilogues wrote the window whose origin lies in the image, i.e. one column / row
    beyond the (hw / 2)-wide output, pooling a pixel outside the image.  Choice made: ``va_conv3x3_layer`` REJECTS pooling
    with an odd hw (ValueError, ``REJECTED``); the model's layers all have even sizes.
"""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U = 2.0 ** -24
# Largest normalised fp32 error r = |got - ref| / (2^-24 S) allowed (also the constant of the bf16 rule).
# Measured on the MI355X over all fp32-output cases: worst r = 6.4 (f32_mfma_wide_hw224_cin16), 3.1 .. 6.4 per case;
# C_F32 = 25 (3.9x headroom).
C_F32 = 25.0


def _c(dtype, hw, cin, cout, pool, B, runs, linear=False, mask=False, out_f32=False):
    return dict(dtype=dtype, hw=hw, cin=cin, cout=cout, pool=pool, B=B, runs=runs, linear=linear, mask=mask, out_f32=out_f32)


def _img14(T, p):
    return "k_conv3x3_img14<%s,%s>" % (T, p)


def _dma(nt, p, nb):
    return "k_conv3x3_dma_f32<%d,%s,%d>" % (nt, p, nb)


def _mfma(nt, p):
    return "k_conv3x3_mfma<2,2,2,%d,%s,16>" % (nt, p)


def _bf(nt, p, f32, nb):
    return "k_conv3x3_mfma_bf16<%d,%s,%s,%d>" % (nt, p, f32, nb)


def _pp(nt, p):
    return "k_conv3x3_pp_bf16<%d,%s>" % (nt, p)


def _ws(p):
    return "k_conv3x3_ws_bf16<%s>" % p


T, F_ = "true", "false"

# id -> case.  runs: (kernel_opt, expected instantiation); all runs of a case take the same input and must agree bit for bit.
# fp32 kernel_opt = VA_OPT_F32_CONV_KERNEL; bf16 kernel_opt = VA_OPT_BF16_VARIANT.  Grids: 128-pixel bricks x 64 channels
# (VA_RING_MAXGRID*: the DMA ring below 1024 of them), 128-channel register-staged tiles from 512 workgroups (VA_WIDE_MIN).
CASES = {
    # ---- fp32: one image x 64 channels per workgroup on 14 x 14 (k_conv3x3_img14<float>: chunk-major K order)
    "f32_img14_nopool_b3": _c("f32", 14, 64, 128, False, 3, [(1, _img14("float", F_))]),
    "f32_img14_pool_b5_c192": _c("f32", 14, 64, 192, True, 5, [(1, _img14("float", T))]),
    "f32_img14_pool_b1": _c("f32", 14, 128, 64, True, 1, [(1, _img14("float", T))]),
    "f32_img14_nopool_b33": _c("f32", 14, 64, 64, False, 33, [(1, _img14("float", F_))]),
    "f32_img14_odd_chunks_1": _c("f32", 14, 32, 64, False, 3, [(1, _img14("float", F_))]),
    "f32_img14_odd_chunks_3": _c("f32", 14, 96, 128, False, 2, [(1, _img14("float", F_))]),
    # ---- fp32 LDS-DMA kernel: ring (small grids), 128-channel tiles, 64-channel tiles; tap-major like k_conv3x3_mfma
    "f32_ring_nopool_hw28": _c("f32", 28, 64, 128, False, 3, [(1, _dma(1, F_, 3)), (0, _mfma(1, F_))]),
    "f32_ring_pool_hw56": _c("f32", 56, 32, 64, True, 1, [(1, _dma(1, T, 3)), (0, _mfma(1, T))]),
    "f32_ring_nopool_hw13": _c("f32", 13, 32, 64, False, 3, [(1, _dma(1, F_, 3))]),
    "f32_ring_nopool_hw27": _c("f32", 27, 64, 64, False, 1, [(1, _dma(1, F_, 3))]),
    "f32_ring_nopool_hw7_b5": _c("f32", 7, 64, 128, False, 5, [(1, _dma(1, F_, 3))]),
    "f32_ring_pool_hw28_b5": _c("f32", 28, 32, 320, True, 5, [(1, _dma(1, T, 3))]),
    "f32_wide_nopool": _c("f32", 28, 32, 384, False, 33, [(1, _dma(2, F_, 1)), (0, _mfma(2, F_))]),
    "f32_wide_pool": _c("f32", 56, 32, 384, True, 8, [(1, _dma(2, T, 1)), (0, _mfma(2, T))]),
    "f32_single_pool_c320": _c("f32", 28, 32, 320, True, 33, [(1, _dma(1, T, 1))]),
    "f32_single_nopool_c192": _c("f32", 112, 32, 192, False, 4, [(1, _dma(1, F_, 1))]),
    # ---- fp32 register-staged kernel (VA_OPT_F32_CONV_KERNEL = 0 everywhere; cin_pad 16 (the RGB first layer) always)
    "f32_mfma_wide_hw224_cin16": _c("f32", 224, 16, 256, False, 1, [(1, _mfma(2, F_)), (0, _mfma(2, F_))]),
    "f32_mfma_narrow_pool_cin16": _c("f32", 112, 16, 64, True, 2, [(1, _mfma(1, T))]),
    "f32_mfma_narrow_pool_c192": _c("f32", 28, 64, 192, True, 3, [(0, _mfma(1, T))]),
    "f32_mfma_hw14_nopool": _c("f32", 14, 64, 128, False, 3, [(0, _mfma(1, F_))]),
    "f32_mfma_hw14_pool_b33": _c("f32", 14, 512, 64, True, 33, [(0, _mfma(1, T))]),
    # ---- fp32 training forms: dgrad (linear, mask), and linear with pooling
    "f32_dgrad_hw28": _c("f32", 28, 128, 64, False, 3, [(1, _dma(1, F_, 3)), (0, _mfma(1, F_))], linear=True, mask=True),
    "f32_dgrad_hw14": _c("f32", 14, 64, 64, False, 2, [(1, _dma(1, F_, 3)), (0, _mfma(1, F_))], linear=True, mask=True),
    "f32_dgrad_hw56_cin16": _c("f32", 56, 16, 64, False, 1, [(1, _mfma(1, F_))], linear=True, mask=True),
    "f32_mask_relu_hw28": _c("f32", 28, 32, 64, False, 2, [(1, _dma(1, F_, 3))], mask=True),
    "f32_linear_pool_hw28": _c("f32", 28, 64, 128, True, 3, [(1, _dma(1, T, 3)), (0, _mfma(1, T))], linear=True),
    # ---- bf16: two-group kernel (variant 5 on every layer >= 28 x 28 with >= 128 channels; the default at 28 x 28 / B = 33)
    "bf_pp4_nopool": _c("bf16", 28, 64, 256, False, 3, [(5, _pp(4, F_)), (1, _bf(1, F_, F_, 1)), (2, _bf(1, F_, F_, 3))]),
    "bf_pp4_pool": _c("bf16", 28, 64, 256, True, 3, [(5, _pp(4, T)), (0, _bf(1, T, F_, 3))]),
    "bf_pp4_default_b33": _c("bf16", 28, 64, 512, False, 33, [(0, _pp(4, F_)), (2, _bf(1, F_, F_, 3))]),
    "bf_pp2_pool_c384": _c("bf16", 56, 64, 384, True, 1, [(5, _pp(2, T)), (1, _bf(1, T, F_, 1))]),
    "bf_pp2_nopool_cin128": _c("bf16", 28, 128, 128, False, 3, [(5, _pp(2, F_)), (0, _bf(1, F_, F_, 3))]),
    # ---- bf16 one image per workgroup on 14 x 14 (chunk-major: its own group; variants 1, 2 keep the tap-major kernel)
    "bf_img14_nopool": _c("bf16", 14, 128, 128, False, 3, [(0, _img14("__bf16", F_)), (5, _img14("__bf16", F_)),
                                                           (7, _img14("__bf16", F_))]),
    "bf_img14_pool_f32_c192": _c("bf16", 14, 128, 192, True, 5, [(0, _img14("__bf16", T))], out_f32=True),
    "bf_img14_odd_chunks_1": _c("bf16", 14, 64, 64, False, 5, [(0, _img14("__bf16", F_))]),
    "bf_img14_odd_chunks_3": _c("bf16", 14, 192, 128, False, 3, [(0, _img14("__bf16", F_))]),
    "bf_img14_b33": _c("bf16", 14, 128, 64, False, 33, [(0, _img14("__bf16", F_))]),
    "bf_hw14_tapmajor_pool_f32": _c("bf16", 14, 128, 64, True, 5, [(1, _bf(1, T, T, 1)), (2, _bf(1, T, T, 3))], out_f32=True),
    "bf_hw14_tapmajor_nopool": _c("bf16", 14, 64, 128, False, 3, [(1, _bf(1, F_, F_, 1)), (2, _bf(1, F_, F_, 3))]),
    # ---- bf16 weights-resident kernel (64 input channels, hw % 16 == 0): bit-equal to the tap-major kernels
    "bf_ws_nopool_c64": _c("bf16", 32, 64, 64, False, 2, [(0, _ws(F_)), (7, _ws(F_)), (1, _bf(1, F_, F_, 1)),
                                                          (2, _bf(1, F_, F_, 3))]),
    "bf_ws_pool_c128": _c("bf16", 32, 64, 128, True, 3, [(7, _ws(T)), (0, _bf(1, T, F_, 3)), (1, _bf(1, T, F_, 1)),
                                                         (2, _bf(1, T, F_, 3)), (5, _pp(2, T))]),
    "bf_ws_pool_c192_hw48": _c("bf16", 48, 64, 192, True, 1, [(7, _ws(T)), (1, _bf(1, T, F_, 1))]),
    # ---- bf16 tap-major kernel: ring / 128-channel tiles / 64-channel tiles x (pool, pool + fp32 output, no pool)
    "bf_ring_pool": _c("bf16", 28, 64, 128, True, 3, [(2, _bf(1, T, F_, 3)), (1, _bf(1, T, F_, 1))]),
    "bf_ring_pool_f32": _c("bf16", 28, 128, 128, True, 3, [(0, _bf(1, T, T, 3)), (1, _bf(1, T, T, 1))], out_f32=True),
    "bf_ring_nopool_hw13": _c("bf16", 13, 64, 64, False, 3, [(2, _bf(1, F_, F_, 3)), (1, _bf(1, F_, F_, 1)),
                                                             (0, _bf(1, F_, F_, 3))]),
    "bf_ring_nopool_hw7_b5": _c("bf16", 7, 128, 64, False, 5, [(0, _bf(1, F_, F_, 3))]),
    "bf_wide_nopool": _c("bf16", 28, 64, 384, False, 33, [(0, _bf(2, F_, F_, 1)), (1, _bf(1, F_, F_, 1)),
                                                          (5, _pp(2, F_))]),
    "bf_wide_pool": _c("bf16", 28, 64, 384, True, 33, [(0, _bf(2, T, F_, 1)), (2, _bf(1, T, F_, 3))]),
    "bf_wide_pool_f32": _c("bf16", 28, 64, 384, True, 33, [(0, _bf(2, T, T, 1)), (1, _bf(1, T, T, 1))], out_f32=True),
    "bf_single_nopool_hw27": _c("bf16", 27, 64, 64, False, 3, [(1, _bf(1, F_, F_, 1))]),
    "bf_single_pool_c320": _c("bf16", 28, 64, 320, True, 33, [(0, _bf(1, T, F_, 1))]),
    "bf_single_pool_f32_c320": _c("bf16", 28, 64, 320, True, 33, [(0, _bf(1, T, T, 1))], out_f32=True),
}

# the instantiations a default build can launch from launch_conv_ex (12) and launch_conv_bf16 (17)
INSTANTIATIONS = sorted(
    [_img14("float", p) for p in (T, F_)] + [_dma(nt, p, nb) for nt, nb in ((1, 3), (2, 1), (1, 1)) for p in (T, F_)]
    + [_mfma(nt, p) for nt in (1, 2) for p in (T, F_)]
    + [_pp(nt, p) for nt in (2, 4) for p in (T, F_)] + [_img14("__bf16", p) for p in (T, F_)] + [_ws(p) for p in (T, F_)]
    + [_bf(nt, p, f, nb) for nt, nb in ((1, 3), (2, 1), (1, 1)) for p, f in ((T, F_), (T, T), (F_, F_))])

# shapes the entry refuses (ValueError): id -> (dtype, hw, cin, cout, pool, B, kernel_opt, linear, mask, out_f32)
REJECTED = {
    "f32_cin_not_16": ("f32", 14, 24, 64, False, 1, 1, False, False, False),
    "bf16_cin_not_64": ("bf16", 14, 32, 64, False, 1, 0, False, False, False),
    "cout_not_64": ("f32", 14, 64, 96, False, 1, 1, False, False, False),
    "bf16_cout_not_64": ("bf16", 28, 64, 160, False, 1, 0, False, False, False),
    "out_f32_without_pool": ("bf16", 14, 64, 64, False, 1, 0, False, False, True),
    "mask_with_pool": ("f32", 28, 64, 64, True, 1, 1, False, True, False),
    "mask_with_bf16": ("bf16", 28, 64, 64, False, 1, 0, False, True, False),
    "linear_with_bf16": ("bf16", 28, 64, 64, False, 1, 0, True, False, False),
    "f32_pool_odd_hw": ("f32", 13, 32, 64, True, 1, 1, False, False, False),
    "f32_pool_odd_hw_regstaged": ("f32", 27, 16, 64, True, 1, 0, False, False, False),
    "bf16_pool_odd_hw": ("bf16", 13, 64, 64, True, 1, 0, False, False, False),
    "bf16_pool_odd_hw_f32_out": ("bf16", 27, 64, 64, True, 1, 1, False, False, True),
    "f32_bad_kernel_opt": ("f32", 28, 32, 64, False, 1, 2, False, False, False),
    "bf16_bad_variant": ("bf16", 28, 64, 64, False, 1, 3, False, False, False),
}


# ------------------------------------------------------------------------------------------ reference (any device) ----

def _pool2(t):
    """2x2 max-pool, stride 2, of an NCHW tensor with even H, W (plain reshape + max: no vendor kernel)."""
    B, C, H, W = t.shape
    return t.reshape(B, C, H // 2, 2, W // 2, 2).amax(dim=(3, 5))


def reference_layer(x, w, b, pool=False, linear=False, mask=None, chunk_px=1 << 16):
    """float64 3x3 conv (stride 1, zero padding 1) + bias, ReLU unless ``linear``, zeroed where ``mask <= 0``, 2x2 max-pool.
    x: NHWC [B][hw][hw][cin]; w: [cout][9][cin] (tap 3 ky + kx); b: [cout]; mask: NHWC like the unpooled output.
    Returns NHWC (out, pre, S): the layer's output, the pooled pre-activation (conv + bias, before ReLU and mask) and the
    pooled magnitude sum S = sum |x w| + |b|, all float64 on x's device."""
    x, w, b = x.double(), w.double(), b.double()
    B, hw, _, cin = x.shape
    cout = w.shape[0]
    wm = w.permute(0, 2, 1).reshape(cout, cin * 9)  # F.unfold's K order: channel outer, then ky, kx
    wa = wm.abs()
    per = max(1, chunk_px // (hw * hw))
    ys, ss = [], []
    for i in range(0, B, per):
        cols = torch.nn.functional.unfold(x[i:i + per].permute(0, 3, 1, 2), 3, padding=1)  # [n][cin*9][hw*hw]
        ys.append(torch.matmul(wm, cols))
        ss.append(torch.matmul(wa, cols.abs()))
    pre = (torch.cat(ys) + b[:, None]).reshape(B, cout, hw, hw)
    s = (torch.cat(ss) + b.abs()[:, None]).reshape(B, cout, hw, hw)
    out = pre if linear else pre.clamp_min(0.0)
    if mask is not None:
        out = torch.where(mask.double().permute(0, 3, 1, 2) > 0, out, torch.zeros_like(out))
    if pool:
        out, pre, s = _pool2(out), _pool2(pre), _pool2(s)
    nhwc = (0, 2, 3, 1)
    return out.permute(*nhwc).contiguous(), pre.permute(*nhwc).contiguous(), s.permute(*nhwc).contiguous()


def test_reference_helper_agrees_with_conv2d_and_max_pool2d():
    """CPU: the helper against torch's float64 conv2d / max_pool2d on small shapes, with and without pool, linear, mask."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    for hw, cin, cout, B in ((6, 5, 4, 2), (8, 3, 7, 1), (5, 2, 3, 3)):
        x = torch.randn(B, hw, hw, cin, generator=g, dtype=torch.float64)
        w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
        b = torch.randn(cout, generator=g, dtype=torch.float64)
        wp = w.permute(0, 2, 3, 1).reshape(cout, 9, cin)
        conv = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1)
        mag = F.conv2d(x.abs().permute(0, 3, 1, 2), w.abs(), b.abs(), padding=1)
        m = torch.randn(B, hw, hw, cout, generator=g, dtype=torch.float64)
        for pool in ((False, True) if hw % 2 == 0 else (False,)):
            for linear in (False, True):
                for mask in ((None, m) if not pool else (None,)):
                    want = conv if linear else F.relu(conv)
                    if mask is not None:
                        want = want * (mask.permute(0, 3, 1, 2) > 0)
                    pre, s = conv, mag
                    if pool:
                        want, pre, s = F.max_pool2d(want, 2), F.max_pool2d(pre, 2), F.max_pool2d(s, 2)
                    got, gpre, gs = reference_layer(x, wp, b, pool, linear, mask, chunk_px=2 * hw * hw)
                    for a, r in ((got, want), (gpre, pre), (gs, s)):
                        assert torch.allclose(a, r.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12), (hw, pool, linear, mask is None)
                    assert bool((gs >= got.abs() - 1e-12).all())


# ------------------------------------------------------------------------------------------------ coverage (CPU) ----

def _launcher_body(src, name):
    i = src.index("\nint %s(" % name)
    j = src.index("\n}\n", i)
    return src[i:j]


def test_every_launched_kernel_family_has_layer_cases():
    """CPU: every k_conv3x3_* family that launch_conv_ex / launch_conv_bf16 launch has cases
    here, and the case table reaches exactly the 29 instantiations of a default build."""
    src = open(os.path.join(ROOT, "video_analytics_amd", "csrc", "vgg.hip")).read()
    found = set()
    for fn in ("launch_conv_ex", "launch_conv_bf16"):
        found |= set(re.findall(r"\b(k_conv3x3_\w+)\s*<[^;]*?>\s*<<<", _launcher_body(src, fn)))
    assert len(found) >= 6, found
    expected = {name for c in CASES.values() for _, name in c["runs"]}
    families = {n.split("<")[0] for n in expected}
    assert found <= families, found - families
    assert sorted(expected) == INSTANTIATIONS and len(INSTANTIATIONS) == 29


# --------------------------------------------------------------------------------------------------- GPU cases ----

CANARY = 4096  # bytes of canary / guard before and after each tensor (>= 4 KB)


def _guarded(n, dtype, fill, guard_elems, device):
    """A flat tensor of n elements between two guard blocks of guard_elems elements, all in ONE allocation."""
    buf = torch.empty(n + 2 * guard_elems, dtype=dtype, device=device)
    buf.fill_(fill)
    return buf, buf[guard_elems:guard_elems + n]


def _make_inputs(case, seed):
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, hw, cin, cout = case["B"], case["hw"], case["cin"], case["cout"]
    tdt = torch.bfloat16 if case["dtype"] == "bf16" else torch.float32
    x = torch.randn(B, hw, hw, cin, generator=g)
    w = torch.randn(cout, 9, cin, generator=g) / (9.0 * cin) ** 0.5  # distinct per tap and channel
    b = torch.randn(cout, generator=g) * 0.5                           # distinct per output channel
    x, w = x.to(tdt), w.to(tdt)  # (bf16: the reference takes the rounded operands)
    es = x.element_size()
    # in: NaN guards on both sides, >= 4 KB and >= the (hw + 1) pixels the bf16 buffer resources reach before / after it
    gi = max(CANARY // es, (hw + 1) * cin)
    gi = (gi + 63) // 64 * 64
    in_buf, xin = _guarded(x.numel(), tdt, float("nan"), gi, dev)
    xin.copy_(x.reshape(-1).to(dev))
    mask = None
    hwo = hw // 2 if case["pool"] else hw
    if case["mask"]:
        mask = torch.randn(B, hwo, hwo, cout, generator=g)
        mask[mask.abs() < 0.3] = 0.0  # (exact zeros as well as negative values: both zero the output)
        mask = mask.to(dev)
    return dict(x=x.to(dev), w=w.to(dev), b=b.to(dev), mask=mask, in_buf=in_buf, xin=xin.view(B, hw, hw, cin), gi=gi)


def _run(case, inp, opt, zeros, finite=True):
    """One launch into a NaN-filled output between canaries; returns (name, out copy) after checking the canaries.
    ``finite=False`` (tests/test_nonfinite_gpu.py plants NaN / infinity on purpose) skips only the last assertion."""
    from video_analytics_amd import vgg
    B, hw, cout = case["B"], case["hw"], case["cout"]
    hwo = hw // 2 if case["pool"] else hw
    odt = torch.float32 if (case["dtype"] == "f32" or case["out_f32"]) else torch.bfloat16
    n = B * hwo * hwo * cout
    go = CANARY // (4 if odt == torch.float32 else 2)
    buf = torch.empty(n + 2 * go, dtype=odt, device="cuda")
    ibuf = buf.view(torch.int32 if odt == torch.float32 else torch.int16)
    canary = torch.randint(-30000, 30000, (2 * go,), dtype=ibuf.dtype, device="cuda")
    ibuf[:go] = canary[:go]
    ibuf[go + n:] = canary[go:]
    buf[go:go + n] = float("nan")
    out = buf[go:go + n].view(B, hwo, hwo, cout)
    ity = torch.int32 if inp["in_buf"].dtype == torch.float32 else torch.int16
    in_before = inp["in_buf"].view(ity).clone()
    name = vgg.conv3x3_layer(inp["xin"], inp["w"], inp["b"], out, kernel_opt=opt, pool=case["pool"], linear=case["linear"],
                             mask=inp["mask"], zeros=zeros)
    torch.cuda.synchronize()
    assert torch.equal(ibuf[:go], canary[:go]) and torch.equal(ibuf[go + n:], canary[go:]), (name, "write outside out")
    assert torch.equal(inp["in_buf"].view(ity), in_before), (name, "write into `in` or its guards")
    assert not finite or bool(torch.isfinite(out).all()), (name, "output not written everywhere (or NaN read from outside `in`)")
    return name, out.clone()


def _check_against_reference(case, got, ref, pre, s, label):
    got = got.double()
    d = C_F32 * U * s
    err = (got - ref).abs()
    r = 0.0
    if case["dtype"] == "f32" or case["out_f32"]:
        r = float((err / (U * s)).max())
        assert r < C_F32, (label, "normalised fp32 error", r)
    else:
        _, ex = torch.frexp(ref.abs() + d)
        half_ulp = torch.ldexp(torch.ones_like(ref), ex - 9)  # ulp_bf16(v) = 2^(e - 8) for v = m 2^e, m in [0.5, 1)
        bad = err > half_ulp + d
        assert not bool(bad.any()), (label, "bf16 rounding bound", int(bad.sum()), float(err.max()))
    if not case["linear"]:
        neg = pre < -d
        assert bool((got[neg] == 0).all()), (label, "ReLU zeros are not exact")
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(CASES))
def test_conv_layer_against_float64(cid):
    case = CASES[cid]
    inp = _make_inputs(case, seed=sum(map(ord, cid)))
    zeros = torch.zeros(64, dtype=torch.float32, device="cuda")
    ref, pre, s = reference_layer(inp["x"], inp["w"], inp["b"], case["pool"], case["linear"], inp["mask"])
    first = None
    worst = 0.0
    for opt, want in case["runs"]:
        name, out1 = _run(case, inp, opt, zeros)
        assert name == want, (cid, opt, name, want)
        _, out2 = _run(case, inp, opt, zeros)  # the second of exactly two launches
        assert torch.equal(out1.view(torch.uint8), out2.view(torch.uint8)), (cid, name, "not deterministic")
        worst = max(worst, _check_against_reference(case, out1, ref, pre, s, (cid, name)))
        if case["mask"]:
            zero = inp["mask"] <= 0
            assert bool((out1[zero] == 0).all()), (cid, name, "masked outputs are not exact zeros")
        if first is None:
            first = (name, out1)
        else:  # the same products in the same order: bit for bit
            assert torch.equal(out1.view(torch.uint8), first[1].view(torch.uint8)), (cid, name, "differs from", first[0])
    if case["dtype"] == "f32" or case["out_f32"]:
        print("%s: worst normalised fp32 error %.3g" % (cid, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("rid", sorted(REJECTED))
def test_unsupported_layer_shapes_are_rejected(rid):
    from video_analytics_amd import vgg
    dt, hw, cin, cout, pool, B, opt, linear, mask, out_f32 = REJECTED[rid]
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    hwo = hw // 2 if pool else hw
    x = torch.zeros(B, hw, hw, cin, dtype=tdt, device="cuda")
    w = torch.zeros(cout, 9, cin, dtype=tdt, device="cuda")
    b = torch.zeros(cout, dtype=torch.float32, device="cuda")
    out = torch.full((B, hwo, hwo, cout), float("nan"), dtype=torch.float32 if out_f32 or dt == "f32" else tdt, device="cuda")
    m = torch.ones(B, hwo, hwo, cout, device="cuda") if mask else None
    with pytest.raises(ValueError):
        vgg.conv3x3_layer(x, w, b, out, kernel_opt=opt, pool=pool, linear=linear, mask=m)
    torch.cuda.synchronize()
    assert bool(out.isnan().all())  # nothing was launched


@pytest.mark.gpu
def test_layer_entry_rejects_batch_below_one_and_bf16_offsets_beyond_2gib():
    """Checked before anything is launched, so small tensors stand in for the ones the shapes describe."""
    from video_analytics_amd import _ffi
    L = _ffi.lib()
    t = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    p, z = _ffi.ptr(t), _ffi.ptr(t)
    name = ctypes.create_string_buffer(64)
    args = lambda dt, opt, hw, cin, cout, B: (_ffi.ctx(0), dt, opt, hw, cin, cout, 0, 0, 0, B, p, p, p, None, z, p, name,
                                              len(name), _ffi.stream_ptr())
    for B in (0, -1):
        assert L.va_conv3x3_layer(*args(0, 1, 14, 64, 64, B)) == _ffi.VA_ERR_INVALID
        assert L.va_conv3x3_layer(*args(1, 0, 14, 64, 64, B)) == _ffi.VA_ERR_INVALID
    # 340 images x 224 x 224 x 64 bf16 channels: 2.18 GB, beyond the 32-bit byte offsets of the bf16 staging
    with pytest.raises(ValueError, match="split the batch"):
        _ffi.check(L.va_conv3x3_layer(*args(1, 0, 224, 64, 64, 340)))
    torch.cuda.synchronize()
    assert name.value == b""
