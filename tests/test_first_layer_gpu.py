"""The model's first stage -- input conversion + conv layer 0 -- on every path the dispatch has, against a float64 reference.

``va_vgg16_first_layer`` (include/va.h, testing entry points) runs the function ``va_vgg16_forward`` runs first
(``run_first_stage`` in csrc/vgg.hip) and reports the kernel instantiations it launched.  ``va_conv3x3_layer``
(tests/test_conv_layers_gpu.py) takes an NHWC input that is already padded, so it reaches none of this:
  * bf16, c_in <= 21: ``k_conv1_fused_bf16<float|u8>`` + ``k_pack_conv_w_bf16_f1`` (the default), and under
    VA_OPT_BF16_FIRST_LAYER = 0 -- or whenever x is not 16-byte aligned -- ``k_nchw_to_nhwc_xcol`` +
    ``k_pack_conv_w_bf16_xcol`` + the taps_x = 1 form of ``k_conv3x3_mfma_bf16``;
  * bf16, 22 <= c_in <= 64: ``k_nchw_to_nhwc_pad<.., __bf16>`` + ``k_pack_conv_w_bf16`` at Cin < 64 + the 64-channel kernels;
  * fp32: ``k_nchw_to_nhwc_pad<.., float>`` + ``k_pack_conv_w`` at cin_pad 16, 32, 48, 64.
Each case of ``CASES`` names the ``info`` string every run must report (``%s``: the input type), so a change of the
dispatch fails here; ``test_every_first_stage_instantiation_has_cases`` scans ``run_first_stage`` for its launches.

Reference: ``reference_layer`` of test_conv_layers_gpu.py in float64 on the NCHW input moved to NHWC.  bf16 models: the
operands are rounded to bf16 (nearest even) first, so every product is exact.  u8 input: the operand is
((q / 255 - mean_c) / std_c) in float64 with the float32 mean / std the model was given; the kernels evaluate it in f32 with
three roundings, at most e(q, c) = 2^-22 (q / 255 + |mean_c|) / std_c away.  fp32 models: sum |w| e is added to the allowed
error.  bf16 models: a pair (q, c) whose float64 value lies within e of a bf16 rounding boundary is ambiguous and is not
drawn (the neighbouring q replaces it; at most 2 % of a channel's 256 values, asserted on the CPU).

Per run: ``info`` as named; two launches bit-identical; canaries around ``out`` and ``staged`` hold, x and its guards are
unchanged; ``out`` finite; the fp32 / bf16 bound and exact ReLU zeros of ``_check_against_reference``; ``staged`` element
for element (pad paths: the input, zeros from c_in on; xcol: channel kx C + c = pixel x + kx - 1, zero outside the row and
from 3 C on; fused: untouched).  Bit-equalities: fused == xcol where no channel is padded (c_in % 4 == 0); bf16 variants
0, 1, 2; fp32 kernel 0 == 1; u8 input == the f32 input carrying the numpy-f32 evaluation of the same values (bf16 paths).

Measured on the MI355X: worst normalised fp32 error r = 12.0 (f32_c33; 4.1 .. 12.0 per fp32 case) against C_F32 = 25.

Findings pinned here:
  * ReLU by fmaxf(v, 0) answers 0 for a NaN: a NaN input pixel left k_conv1_fused_bf16 as a plausible 0.  The kernel now
    keeps the NaN (same bits otherwise); ``test_fused_first_layer_confines_a_nan`` holds the 3 x 3 NaN outputs.  The
    staged path's kernels keep it too (tests/test_nonfinite_gpu.py: every conv epilogue); the same test holds its reach.
  * k_conv1_fused_bf16 multiplies the tail of a 16-element K block -- channels of the pixel AFTER the three taps --
    with zero weights.  Finite inputs are unaffected; a NaN / infinity at (y, x) also turns column x - 2 of rows
    y - 1 .. y + 1 into NaN and, when x % 16 == 15 (patch column 0 of the brick to the right, which follows patch column
    17 of the row above in LDS), column x + 16 of rows y - 2 .. y.  Documented in va.h and at the kernel;
    ``test_fused_first_layer_confines_a_nan`` holds the reach to exactly that.
  * At batch <= 2 the staged xcol path runs the DMA-ring form (<1,false,false,3>) of k_conv3x3_mfma_bf16; the form the
    benchmark's batch takes (<1,false,false,1>, from 1024 workgroups) needs batch 3: cases ``bf16_c3_b3``, ``bf16_c20_b3``.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_conv_layers_gpu import C_F32, CANARY, U, _check_against_reference, _guarded, reference_layer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = 224
OPT_VARIANT, OPT_F32, OPT_FIRST = 1, 2, 4  # _ffi.VA_OPT_BF16_VARIANT, VA_OPT_F32_CONV_KERNEL, VA_OPT_BF16_FIRST_LAYER

FUSED = "k_conv1_fused_bf16<%s>"
XCOL = "k_nchw_to_nhwc_xcol<%s>+"
PAD_BF = "k_nchw_to_nhwc_pad<%s,__bf16>+"
PAD_F32 = "k_nchw_to_nhwc_pad<%s,float>+"
BF_RING, BF_SINGLE, BF_WS = ("k_conv3x3_mfma_bf16<1,false,false,3>", "k_conv3x3_mfma_bf16<1,false,false,1>",
                             "k_conv3x3_ws_bf16<false>")
F32_DMA, F32_MFMA = "k_conv3x3_dma_f32<1,false,3>", "k_conv3x3_mfma<2,2,2,1,false,16>"


def _cases():
    """id -> dict(dtype, cin, B, runs, equal).  runs: ({option: value}, info with %s for the input type); ``equal``: all
    runs add the same products in the same order and must agree bit for bit.  224 x 224 x 64 channels are 392 workgroups
    of 128 pixels per image: below 1024 (batch 1, 2) the automatic choice is the DMA ring, from batch 3 the single buffer."""
    cases = {}
    for c in (1, 2, 3, 4, 5, 8, 12, 15, 16, 20, 21):  # Cp 4 .. 24, KROW 16 .. 80
        cases["bf16_c%d" % c] = dict(dtype="bf16", cin=c, B=2, equal=c % 4 == 0,
                                     runs=[({OPT_FIRST: 1}, FUSED), ({OPT_FIRST: 0}, XCOL + BF_RING)])
    for c in (3, 20):
        cases["bf16_c%d_b3" % c] = dict(dtype="bf16", cin=c, B=3, equal=True, runs=[({OPT_FIRST: 0}, XCOL + BF_SINGLE)])
    for c in (22, 24, 33, 63, 64):
        runs = [({OPT_VARIANT: 0}, PAD_BF + BF_WS)]
        if c == 24:
            runs += [({OPT_VARIANT: 1}, PAD_BF + BF_SINGLE), ({OPT_VARIANT: 2}, PAD_BF + BF_RING)]
        cases["bf16_c%d" % c] = dict(dtype="bf16", cin=c, B=1, equal=True, runs=runs)
    for c in (1, 3, 15, 16, 17, 20, 32, 33, 48, 63, 64):  # cin_pad 16, 32, 48, 64; the LDS-DMA kernel takes multiples of 32
        cpad = (c + 15) // 16 * 16
        runs = [({OPT_F32: 1}, PAD_F32 + (F32_DMA if cpad % 32 == 0 else F32_MFMA))]
        if c in (3, 32, 64):
            runs.append(({OPT_F32: 0}, PAD_F32 + F32_MFMA))
        cases["f32_c%d" % c] = dict(dtype="f32", cin=c, B=2 if c <= 21 else 1, equal=True, runs=runs)
    return cases


CASES = _cases()
KINDS = ("float", "u8")

# every input-stage instantiation run_first_stage can launch
INSTANTIATIONS = sorted(["k_conv1_fused_bf16<%s>" % k for k in KINDS] + ["k_nchw_to_nhwc_xcol<%s>" % k for k in KINDS]
                        + ["k_nchw_to_nhwc_pad<%s,%s>" % (k, t) for k in KINDS for t in ("float", "__bf16")])

# pixels with emphasis: corners, edge midpoints, and the seams of the fused kernel's 16 x 16 bricks next to the borders
_S, _E = (15, 16, 207, 208), (0, 223)
SPECIAL = sorted(set([(y, x) for y in _E for x in _E] + [(0, 112), (223, 112), (112, 0), (112, 223)]
                     + [(y, x) for y in _S for x in _S] + [(y, x) for y in _E for x in _S] + [(y, x) for y in _S for x in _E]
                     + [(y, 100) for y in _S] + [(100, x) for x in _S]))


# ------------------------------------------------------------------------------------- inputs and operands (CPU) ----

def _rne_bf16(v):
    """float64 numpy -> the nearest bf16 value (ties to even), as float64 (normal range)."""
    a = np.abs(v)
    _, ex = np.frexp(a)
    ulp = np.ldexp(1.0, ex - 8)  # a = m 2^ex, m in [0.5, 1): 8 significant bits
    return np.sign(v) * np.rint(a / ulp) * ulp


def _norm(cin):
    """float32 mean / std per channel: the project's for RGB, seeded distinct values otherwise."""
    if cin == 3:
        from video_analytics_amd.parameters import NORM_MEANS_TF, NORM_STDS_TF
        return np.array(NORM_MEANS_TF, dtype=np.float32), np.array(NORM_STDS_TF, dtype=np.float32)
    g = np.random.RandomState(1000 + cin)
    return (0.3 + 0.3 * g.rand(cin)).astype(np.float32), (0.15 + 0.2 * g.rand(cin)).astype(np.float32)


def _u8_tables(mean, std):
    """[C][256] float64: the normalised value v, the bound e of its f32 evaluation, and the ambiguous (q, c) pairs."""
    q = np.arange(256, dtype=np.float64)[None, :]
    m, s = mean.astype(np.float64)[:, None], std.astype(np.float64)[:, None]
    v = (q / 255.0 - m) / s
    e = 2.0 ** -22 * (q / 255.0 + np.abs(m)) / s
    amb = _rne_bf16(v - e) != _rne_bf16(v + e)
    return v, e, amb


def _u8_f32_eval(q, mean, std):
    """The expression in numpy float32 (three roundings, like the kernels)."""
    c = (slice(None), None, None)
    return (q.astype(np.float32) / np.float32(255.0) - mean[c]) / std[c]


def _u8_image(B, C, seed, amb=None):
    g = np.random.RandomState(seed)
    q = g.randint(0, 256, size=(B, C, HW, HW)).astype(np.uint8)
    for (y, x) in SPECIAL:  # the extremes: the largest normalised magnitudes
        q[:, :, y, x] = g.choice(np.array([0, 255], dtype=np.uint8), size=(B, C))
    if amb is not None:
        for c in range(C):
            for bad in np.flatnonzero(amb[c]):
                repl = next(r for d in range(1, 256) for r in (bad + d, bad - d) if 0 <= r <= 255 and not amb[c][r])
                q[:, c][q[:, c] == bad] = repl
    assert q.min() == 0 and q.max() == 255
    return q


def _bf16_ties():
    """f32 values half-way between two neighbouring bf16 numbers: even and odd lower neighbour, three binades, both signs."""
    t = [((128 + k) / 128.0 + 2.0 ** -8) * 2.0 ** ex for k in (0, 1, 2, 3, 64, 65, 126, 127) for ex in (-2, 0, 1)]
    return torch.tensor(t + [-v for v in t], dtype=torch.float32)


def _f32_image(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, HW, HW, generator=g) * 0.8).clamp_(-2.5, 2.5)
    flat = x.view(-1)
    ties = _bf16_ties()
    assert torch.equal(ties, ties.double().float()) and not torch.equal(ties.bfloat16().float(), ties)
    pos = torch.randperm(flat.numel(), generator=g)[:ties.numel() * 40 + 2000]
    flat[pos[:ties.numel() * 40]] = ties.repeat(40)
    flat[pos[ties.numel() * 40:]] = 0.0
    for (y, xx) in SPECIAL:  # one tap from here outweighs everything else in its neighbours' sums
        v = torch.randn(B, C, generator=g) * 8.0
        x[:, :, y, xx] = v + torch.sign(v) * 24.0
    return x


def _weights(cin, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(64, cin, 3, 3, generator=g) / (9.0 * cin) ** 0.5  # distinct per output channel, input channel and tap
    b = torch.randn(64, generator=g) * 0.5                             # distinct per output channel
    return w, b


def test_at_most_two_percent_of_a_channels_u8_values_are_ambiguous():
    """CPU: the exclusion of test_first_layer_against_float64 stays a small one, and never takes both extremes away."""
    for cid, case in sorted(CASES.items()):
        if case["dtype"] != "bf16":
            continue
        mean, std = _norm(case["cin"])
        assert len(set(mean.tolist())) == case["cin"] and len(set(std.tolist())) == case["cin"]
        v, e, amb = _u8_tables(mean, std)
        assert float(e.max()) < 2.0 ** -18 and float(np.abs(v).max()) < 8.0
        assert int(amb.sum(axis=1).max()) <= 0.02 * 256, (cid, amb.sum(axis=1))
        q = _u8_image(1, case["cin"], 5, amb)
        assert not amb[np.arange(case["cin"])[None, :, None, None], q].any()


def test_bf16_rounding_helper_is_round_to_nearest_even():
    """CPU: _rne_bf16 against torch's float32 -> bfloat16 on random values and on exact ties."""
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(100000, generator=g) * 3.0, _bf16_ties(), torch.zeros(1)])
    assert np.array_equal(_rne_bf16(x.double().numpy()), x.bfloat16().double().numpy())
    assert _rne_bf16(np.array([1.0 + 2.0 ** -8 + 2.0 ** -40]))[0] == 1.0 + 2.0 ** -7  # (no double rounding through f32)


# ------------------------------------------------------------------------------------------------ coverage (CPU) ----

def _function_body(src, head):
    i = src.index(head)
    return src[i:src.index("\n}\n", i)]


def test_every_first_stage_instantiation_has_cases():
    """CPU: every input-stage kernel run_first_stage launches, with its template arguments, is reached by a named case;
    va_vgg16_forward and va_vgg16_first_layer both go through run_first_stage and launch no such kernel themselves."""
    src = open(os.path.join(ROOT, "video_analytics_amd", "csrc", "vgg.hip")).read()
    body = _function_body(src, "\nstatic int run_first_stage(")
    found = set()
    for name, targs in re.findall(r"\b(k_conv1_fused_bf16|k_nchw_to_nhwc_\w+)\s*<([^<>;]*?)>\s*<<<", body):
        found.add("%s<%s>" % (name, ",".join(a.strip().replace("unsigned char", "u8") for a in targs.split(","))))
    reached = {(info % k).split("+")[0] for c in CASES.values() for _, info in c["runs"] for k in KINDS}
    assert sorted(found) == INSTANTIATIONS and sorted(reached) == INSTANTIATIONS and len(INSTANTIATIONS) == 8
    assert "launch_conv_bf16(" in body and "launch_conv_ex(" in body
    for fn in ('\nextern "C" int va_vgg16_forward(', '\nextern "C" int va_vgg16_first_layer('):
        b = _function_body(src, fn)
        assert "run_first_stage(" in b and not re.search(r"k_conv1_fused_bf16|k_nchw_to_nhwc_(pad|xcol)", b), fn
    # the conv kernels behind the conversions: every form named here is one test_conv_layers_gpu.py knows
    from test_conv_layers_gpu import INSTANTIATIONS as CONV
    assert {info.split("+")[1] for c in CASES.values() for _, info in c["runs"] if "+" in info} <= set(CONV)
    assert {c["cin"] for c in CASES.values() if c["dtype"] == "bf16" and c["runs"][0][1] == FUSED} == {1, 2, 3, 4, 5, 8, 12, 15, 16, 20, 21}
    assert {(c["cin"] + 15) // 16 * 16 for c in CASES.values() if c["dtype"] == "f32"} == {16, 32, 48, 64}


# --------------------------------------------------------------------------------------------------- GPU cases ----

@pytest.fixture(scope="module")
def rest():
    """The 12 other conv layers and the classifier as zero tensors on the device, shared by every model of the module."""
    couts = [64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512]
    z = lambda *s: torch.zeros(*s, device="cuda")
    fcs = [(4096, 512 * 49), (4096, 4096), (16, 4096), (1, 16)]
    return dict(cw=[z(couts[i], couts[i - 1], 3, 3) for i in range(1, 13)], cb=[z(couts[i]) for i in range(1, 13)],
                fw=[z(*s) for s in fcs], fb=[z(s[0]) for s in fcs])


def _model(rest, dtype, w, b, mean=None, std=None):
    from video_analytics_amd import vgg
    return vgg.Vgg16Stream([w.cuda()] + rest["cw"], [b.cuda()] + rest["cb"], rest["fw"], rest["fb"], 1, 16,
                           None if mean is None else mean.tolist(), None if std is None else std.tolist(), dtype=dtype)


def _place(x, shift=0):
    """x (CPU, NCHW f32 / u8) on the device between guard blocks (NaN / 255), `shift` elements past a 16-byte boundary."""
    x = x if isinstance(x, torch.Tensor) else torch.from_numpy(x)
    g = CANARY // x.element_size()
    buf, _ = _guarded(x.numel() + 16, x.dtype, float("nan") if x.dtype == torch.float32 else 255, g, "cuda")
    view = buf[g + shift:g + shift + x.numel()]
    view.copy_(x.reshape(-1).cuda())
    assert view.data_ptr() % 16 == (shift * x.element_size()) % 16
    return buf, view.view(x.shape)


STAGED_FILL = 0x7FA5  # a NaN in bf16, and (twice) in f32
STAGED_GUARD = 16384  # elements: beyond the (224 + 1) pixels x 64 channels the bf16 buffer resources reach around `staged`


def _run(model, xbuf, x, cpad):
    """One launch into NaN-filled `out` and pattern-filled `staged`, both between canaries.  Returns (info, out, staged)
    after checking the canaries, the input and that every output is finite."""
    B = x.shape[0]
    bf = model.dtype == "bf16"
    odt, ity = (torch.bfloat16, torch.int16) if bf else (torch.float32, torch.int32)
    bufs = []
    for n, guard in ((B * HW * HW * 64, CANARY // (2 if bf else 4)), (B * HW * HW * cpad, STAGED_GUARD)):
        buf = torch.empty(n + 2 * guard, dtype=odt, device="cuda")
        ibuf = buf.view(ity)
        canary = torch.randint(-30000, 30000, (2 * guard,), dtype=ity, device="cuda")
        ibuf[:guard] = canary[:guard]
        ibuf[guard + n:] = canary[guard:]
        bufs.append((buf, ibuf, canary, guard, n))
    (obuf, _, _, go, no), (sbuf, isbuf, _, gs, ns) = bufs
    obuf[go:go + no] = float("nan")
    isbuf[gs:gs + ns] = STAGED_FILL if bf else (STAGED_FILL << 16 | STAGED_FILL)
    out = obuf[go:go + no].view(B, HW, HW, 64)
    staged = sbuf[gs:gs + ns].view(B, HW * HW, cpad)
    xity = torch.int32 if xbuf.dtype == torch.float32 else torch.uint8
    before = xbuf.view(xity).clone()
    info = model.first_layer(x, staged, out)
    torch.cuda.synchronize()
    for (_, ibuf, canary, guard, n), what in zip(bufs, ("out", "staged")):
        assert torch.equal(ibuf[:guard], canary[:guard]) and torch.equal(ibuf[guard + n:], canary[guard:]), (info, "write outside " + what)
    assert torch.equal(xbuf.view(xity), before), (info, "write into x or its guards")
    return info, out.clone(), staged.clone()


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _check_staged(info, staged, op, e, cin, cpad, bf):
    """op: the operand NHWC [B][224][224][cin] float64 (bf16 models: already rounded); e: the u8 bound, NHWC, or None."""
    B = op.shape[0]
    ity = torch.int16 if bf else torch.int32
    st = staged.view(B, HW, HW, cpad)
    if info.startswith("k_conv1_fused_bf16"):
        assert bool((staged.view(ity) == STAGED_FILL).all()), (info, "the fused path wrote into staged")
        return
    if info.startswith("k_nchw_to_nhwc_xcol"):
        p = torch.nn.functional.pad(op, (0, 0, 1, 1))  # one zero pixel left and right of every row
        want = torch.cat([p[:, :, kx:kx + HW, :] for kx in range(3)] + [torch.zeros(B, HW, HW, 64 - 3 * cin, dtype=op.dtype, device=op.device)], dim=3)
        assert bool((want[:, :, 0, :cin] == 0).all()) and bool((want[:, :, -1, 2 * cin:] == 0).all())
        n = 3 * cin
    else:
        want = torch.cat([op, torch.zeros(B, HW, HW, cpad - cin, dtype=op.dtype, device=op.device)], dim=3)
        n = cin
    assert bool((st[..., n:].contiguous().view(ity) == 0).all()), (info, "padded channels of staged are not exact zeros")
    if e is None or bf:  # bit for bit: the f32 input itself, its bf16 rounding, or the unambiguous u8 values
        assert torch.equal(st.view(ity), want.to(st.dtype).view(ity)), (info, "staged differs", int((st.double() != want).sum()))
    else:
        assert bool(((st[..., :cin].double() - op).abs() <= e).all()), (info, "staged beyond the bound of the f32 expression")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(CASES))
def test_first_layer_against_float64(cid, rest):
    case = CASES[cid]
    cin, B, bf = case["cin"], case["B"], case["dtype"] == "bf16"
    cpad = 64 if bf else (cin + 15) // 16 * 16
    seed = sum(map(ord, cid))
    w, b = _weights(cin, seed)
    mean, std = _norm(cin)
    v, e, amb = _u8_tables(mean, std)
    m = _model(rest, case["dtype"], w, b, mean, std)
    wd = (w.bfloat16() if bf else w).double().permute(0, 2, 3, 1).reshape(64, 9, cin).cuda()
    bd = b.double().cuda()
    chan = torch.arange(cin, device="cuda")[None, :, None, None]
    q = _u8_image(B, cin, seed + 1, amb if bf else None)
    if bf:
        assert not amb[np.arange(cin)[None, :, None, None], q].any()
    refcase = dict(dtype=case["dtype"], out_f32=False, linear=False)
    worst = 0.0
    u8_out = {}
    for kind in KINDS:
        if kind == "float":
            xc = _f32_image(B, cin, seed + 2)
            op = (xc.bfloat16() if bf else xc).double().cuda().permute(0, 2, 3, 1).contiguous()
            eimg = None
        else:
            xc = q
            table = torch.from_numpy(_rne_bf16(v) if bf else v).cuda()
            op = table[chan, torch.from_numpy(q).cuda().long()].permute(0, 2, 3, 1).contiguous()
            eimg = torch.from_numpy(e).cuda()[chan, torch.from_numpy(q).cuda().long()].permute(0, 2, 3, 1).contiguous()
        ref, pre, s = reference_layer(op, wd, bd)
        if eimg is not None and not bf:  # d + sum |w| e: fold the second term into the magnitude sum (d = C_F32 U s)
            _, esum, _ = reference_layer(eimg, wd.abs(), torch.zeros_like(bd))
            s = s + esum / (C_F32 * U)
        xbuf, x = _place(xc)
        first = None
        for opts, want in case["runs"]:
            for o, val in opts.items():
                m.set_option(o, val)
            info, out1, st1 = _run(m, xbuf, x, cpad)
            assert info == want % kind, (cid, opts, info)
            assert bool(torch.isfinite(out1).all()), (cid, info, "output not written everywhere, or a value from outside x")
            _, out2, st2 = _run(m, xbuf, x, cpad)
            assert torch.equal(_bits(out1), _bits(out2)) and torch.equal(_bits(st1), _bits(st2)), (cid, info, "not deterministic")
            worst = max(worst, _check_against_reference(refcase, out1, ref, pre, s, (cid, info)))
            _check_staged(info, st1, op, eimg, cin, cpad, bf)
            if first is None:
                first = (info, out1)
            elif case["equal"]:  # the same products in the same order: bit for bit
                assert torch.equal(_bits(out1), _bits(first[1])), (cid, info, "differs from", first[0])
            if kind == "u8":
                u8_out[want] = out1
        del ref, pre, s, op
    if bf:  # the same values as f32 input: every conversion rounds them to the same bf16 numbers
        xbuf, x = _place(_u8_f32_eval(q, mean, std))
        for opts, want in case["runs"]:
            for o, val in opts.items():
                m.set_option(o, val)
            info, out1, _ = _run(m, xbuf, x, cpad)
            assert info == want % "float"
            assert torch.equal(_bits(out1), _bits(u8_out[want])), (cid, info, "u8 and f32 inputs of the same values differ")
    else:
        print("%s: worst normalised fp32 error %.3g" % (cid, worst))
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cin", [3, 5, 8, 20])
def test_unaligned_input_takes_the_staged_path(cin, rest):
    """x that is not 16-byte aligned: the fused kernel (four pixels per load) is not used; the result is the staged path's."""
    w, b = _weights(cin, 300 + cin)
    mean, std = _norm(cin)
    m = _model(rest, "bf16", w, b, mean, std)
    for kind, xc in (("float", _f32_image(2, cin, 310 + cin)), ("u8", _u8_image(2, cin, 320 + cin))):
        xbuf, x = _place(xc)
        ubuf, xu = _place(xc, shift=1)  # 4 bytes (f32) / 1 byte (u8) past a 16-byte boundary
        assert xu.data_ptr() % 16 != 0 and torch.equal(_bits(x), _bits(xu))
        m.set_option(OPT_FIRST, 1)
        fused_info, fused, _ = _run(m, xbuf, x, 64)
        info, got, _ = _run(m, ubuf, xu, 64)
        m.set_option(OPT_FIRST, 0)
        staged_info, want, _ = _run(m, xbuf, x, 64)
        assert fused_info == FUSED % kind and staged_info == (XCOL + BF_RING) % kind
        assert info == staged_info, (kind, info)
        assert torch.equal(_bits(got), _bits(want)), (kind, "unaligned run differs from the staged path")
        if cin % 4 == 0:
            assert torch.equal(_bits(got), _bits(fused)), (kind, "unaligned run differs from the fused path")
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cin", [3, 5, 20])
def test_fused_first_layer_confines_a_nan(cin, rest):
    """One NaN in one interior pixel of channel 0 of image 1.  Outside rows y - 1 .. y + 1 and columns x - 2 .. x + 2 of
    that image the output is bit-identical to the clean run, inside the 3 x 3 neighbourhood it is NaN (x % 16 = 5).  At
    x % 16 == 15 the zero-weight tail of the brick to the right also reads it: column x + 16 of rows y - 2 .. y.
    The staged path (unaligned x) confines the same NaN to exactly the 3 x 3 neighbourhood."""
    w, b = _weights(cin, 400 + cin)
    m = _model(rest, "bf16", w, b)
    xc = _f32_image(2, cin, 410 + cin)
    xbuf, x = _place(xc)
    info, clean, _ = _run(m, xbuf, x, 64)
    assert info == FUSED % "float" and bool(torch.isfinite(clean).all())
    for (y, xx) in ((100, 37), (100, 47)):
        xn = xc.clone()
        xn[1, 0, y, xx] = float("nan")
        nbuf, xd = _place(xn)
        info, got, _ = _run(m, nbuf, xd, 64)
        assert info == FUSED % "float"
        assert bool(got[1, y - 1:y + 2, xx - 1:xx + 2].isnan().all()), (cin, y, xx)
        allowed = torch.zeros(2, HW, HW, dtype=torch.bool, device="cuda")
        allowed[1, y - 1:y + 2, xx - 2:xx + 3] = True
        if xx % 16 == 15:
            allowed[1, y - 2:y + 1, xx + 16] = True
        same = (_bits(got).view(2, HW, HW, 128) == _bits(clean).view(2, HW, HW, 128)).all(dim=3)
        assert bool((same | allowed).all()), (cin, y, xx, torch.nonzero(~(same | allowed))[:8].tolist())
    # The staged path (x 4 bytes past alignment: k_nchw_to_nhwc_xcol + the tap-major kernel) pads K with zeros of its own,
    # never with a neighbour's channels: its reach is exactly the 3 x 3 neighbourhood, every channel of it NaN.
    sbuf, xs = _place(xc, shift=1)
    info, clean_s, _ = _run(m, sbuf, xs, 64)
    assert info == (XCOL + BF_RING) % "float" and bool(torch.isfinite(clean_s).all())
    for (y, xx) in ((100, 37), (100, 47)):
        xn = xc.clone()
        xn[1, 0, y, xx] = float("nan")
        nbuf, xd = _place(xn, shift=1)
        info, got, _ = _run(m, nbuf, xd, 64)
        assert info == (XCOL + BF_RING) % "float"
        hit = torch.zeros(2, HW, HW, dtype=torch.bool, device="cuda")
        hit[1, y - 1:y + 2, xx - 1:xx + 2] = True
        assert bool(got[hit].isnan().all()), (cin, y, xx, "staged path: the NaN was dropped")
        same = (_bits(got).view(2, HW, HW, 128) == _bits(clean_s).view(2, HW, HW, 128)).all(dim=3)
        assert torch.equal(~same, hit), (cin, y, xx, torch.nonzero(same == hit)[:8].tolist())
    m.close()


@pytest.mark.gpu
def test_first_layer_entry_rejects_bad_arguments(rest):
    """Every argument error is VA_ERR_INVALID before anything is launched: `out` is still NaN afterwards."""
    from video_analytics_amd import _ffi
    L = _ffi.lib()
    w, b = _weights(3, 500)
    mean, std = _norm(3)
    bfm, f32m, plain = _model(rest, "bf16", w, b, mean, std), _model(rest, "f32", w, b, mean, std), _model(rest, "bf16", w, b)
    x = torch.zeros(1, 3, HW, HW, device="cuda")
    xq = torch.zeros(1, 3, HW, HW, dtype=torch.uint8, device="cuda")
    out = torch.full((HW * HW * 64 + 8,), float("nan"), device="cuda")       # (large enough for either dtype at batch 1)
    staged = torch.full((HW * HW * 64 + 8,), float("nan"), device="cuda")
    info = ctypes.create_string_buffer(160)
    P = _ffi.ptr
    call = lambda m, xp, u8, B, sp, op: L.va_vgg16_first_layer(m, xp, u8, B, sp, op, info, len(info), _ffi.stream_ptr())
    bad = [
        (None, P(x), 0, 1, P(staged), P(out)), (bfm._h, None, 0, 1, P(staged), P(out)), (bfm._h, P(x), 0, 1, None, P(out)),
        (bfm._h, P(x), 0, 1, P(staged), None),
        (bfm._h, P(x), 0, 0, P(staged), P(out)), (f32m._h, P(x), 0, -1, P(staged), P(out)),
        (plain._h, P(xq), 1, 1, P(staged), P(out)),                      # u8 without mean / std
        (bfm._h, P(x), 0, 1, P(staged[1:]), P(out)), (bfm._h, P(x), 0, 1, P(staged), P(out[2:])),  # 4 / 8 bytes off
        (f32m._h, P(xq), 1, 1, P(staged), P(out[1:])),
        (bfm._h, P(x), 0, 335, P(staged), P(out)), (bfm._h, P(xq), 1, 4097, P(staged), P(out)),     # the bf16 batch limit
    ]
    for args in bad:
        assert call(*args) == _ffi.VA_ERR_INVALID, args
        assert info.value == b"" and L.va_last_error() != b""
    with pytest.raises(ValueError, match="split the batch"):
        _ffi.check(call(bfm._h, P(x), 0, 340, P(staged), P(out)))
    with pytest.raises(ValueError):
        bfm.first_layer(x, staged[:HW * HW * 64].view(1, HW * HW, 64), out[:HW * HW * 64].view(1, HW, HW, 64))  # f32 tensors, bf16 model
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and bool(staged.isnan().all())
    for m in (bfm, f32m, plain):
        m.close()
