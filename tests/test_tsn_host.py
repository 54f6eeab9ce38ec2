"""TSN training, host side: the scale-jitter and corner-crop draws, training-time segment sampling, and
float32 numpy restatements of the crop-resize gather and the consensus loss, each held to a float64 witness with a
tolerance derived here.  tests/test_tsn_gpu.py holds the kernels to these restatements bit for bit."""
import random
from fractions import Fraction

import numpy as np
import pytest
import torch

F32 = np.float32
EPS = 2.0 ** -24  # unit roundoff of float32: |fl(x) - x| <= EPS * |x|
OUT = 224
MEAN, STD = F32(0.485), F32(0.229)


# ---- S17: the restatement ----

def s17_taps(size, flip=False):
    """S17's positions of the 224 outputs along an axis of ``size`` source pixels, in its written order and in float32
    -> (i0 int, i1 int, a f32, u f32, p f32, s f32); ``flip`` mirrors the output index first (columns only)."""
    o = np.arange(OUT)
    if flip:
        o = OUT - 1 - o
    s = F32(size) / F32(224.0)
    p = (o.astype(F32) + F32(0.5)) * s
    u = p - F32(0.5)
    u = np.minimum(np.maximum(u, F32(0.0)), F32(size - 1))
    i0 = np.floor(u).astype(np.int64)
    a = u - i0.astype(F32)
    i1 = np.minimum(i0 + 1, size - 1)
    assert u.dtype == F32 and a.dtype == F32
    return i0, i1, a, u, p, s


def s17_resize(plane, row):
    """One source plane (float32 [h,w]) through table row {src, top, left, ch, cw, flip} -> float32 [224,224]: S12's
    bilinear form on S17's taps."""
    _, top, left, ch, cw, flip = (int(v) for v in row)
    plane = plane.astype(F32, copy=False)
    x0, x1, ax, _, _, _ = s17_taps(cw, bool(flip))
    y0, y1, ay, _, _, _ = s17_taps(ch)
    ra, rb = plane[top + y0], plane[top + y1]
    A, B, C, D = ra[:, left + x0], ra[:, left + x1], rb[:, left + x0], rb[:, left + x1]
    t = A + ax[None, :] * (B - A)
    b = C + ax[None, :] * (D - C)
    val = t + ay[:, None] * (b - t)
    assert val.dtype == F32
    return val


def s9_quantise(val, bound=20.0, invert=False):
    """S9 in its written order on float32 values -> the normalised float32 network input."""
    bound = F32(bound)
    t = (F32(255.0) * (val + bound)) / (F32(2.0) * bound)
    q = np.rint(np.minimum(np.maximum(t, F32(0.0)), F32(255.0)))
    if invert:
        q = F32(255.0) - q
    return (q / F32(255.0) - MEAN) / STD


def s17_flow_stack(flow, table, invert_x=False):
    """flow float32 [N,2,h,w], table int [n_out,6] -> float32 [n_out,224,224]: va_flow_to_stack_resize."""
    planes = flow.reshape((-1,) + flow.shape[2:])
    out = np.empty((len(table), OUT, OUT), dtype=F32)
    for o, row in enumerate(np.asarray(table).tolist()):
        inv = bool(invert_x) and bool(row[5]) and row[0] % 2 == 0
        out[o] = s9_quantise(s17_resize(planes[row[0]], row), invert=inv)
    return out


def s17_images_u8(x, table, layout="NCHW"):
    """x uint8 [n,c,h,w] (or [n,h,w,c]), table int [n_out,6] -> uint8 [n_out,c,224,224]: va_resize_images_u8."""
    if layout == "NHWC":
        x = x.transpose(0, 3, 1, 2)
    out = np.empty((len(table), x.shape[1], OUT, OUT), dtype=np.uint8)
    for o, row in enumerate(np.asarray(table).tolist()):
        for c in range(x.shape[1]):
            val = s17_resize(x[row[0], c].astype(F32), row)
            out[o, c] = np.rint(np.minimum(np.maximum(val, F32(0.0)), F32(255.0))).astype(np.uint8)
    return out


# ---- S17: the position bound and the value tolerance, derived ----

def position_bound(size, flip=False):
    """Bound on |u - u*| per output index, u* = (o' + 1/2) * size / 224 - 1/2 clamped to [0, size - 1] being the exact
    position.  Round to nearest puts a result within half a unit in the last place of its exact value, and
    ``np.spacing(|r|)`` is never less than that unit at the rounded result r.  Three operations round:
      s = fl(size / 224)          |s - s*| <= spacing(s) / 2, carried to the product by the exact factor (o' + 1/2),
      p = fl((o' + 1/2) * s)      |p - (o' + 1/2) s| <= spacing(p) / 2,
      u = fl(p - 1/2)             |u - (p - 1/2)| <= spacing(|u|) / 2;
    (o' + 1/2) is exact in float32, the clamp's limits 0 and size - 1 are exact and clamping never increases a distance,
    and u - floor(u) is exact (both lie in one binade below 2^23 or floor(u) = 0)."""
    _, _, _, _, p, s = s17_taps(size, flip)
    o = np.arange(OUT)
    if flip:
        o = OUT - 1 - o
    u_raw = p - F32(0.5)
    return ((o + 0.5) * float(np.spacing(s)) / 2.0 + np.spacing(np.abs(p)).astype(np.float64) / 2.0
            + np.spacing(np.abs(u_raw)).astype(np.float64) / 2.0)


def value_tolerance(region, ch, cw, flip):
    """Bound on |restatement - exact bilinear value| per output pixel, for data ``region`` (the crop):
    the bilinear interpolant is continuous and piecewise linear with slope at most D = the largest difference of
    neighbouring samples, so a position error (dx, dy) moves it by at most (dx + dy) * D; and its evaluation
    t = A + ax*(B - A), b likewise, val = t + ay*(b - t) rounds three times per line: |t^ - t| <= ax*|B - A|*(2 EPS + EPS^2)
    + EPS*|t^| <= EPS*(2.01 D + 1.01 F) = E1 with F = max |f|, the same for b, the exact combination of t^ and b^ is within E1
    of val and its own three roundings add at most (D + 2 E1)*2.01 EPS + (F + 2 E1)*1.01 EPS: EPS*(5 D + 3 F) covers
    the sum.  The float64 witness's own error (a few 2^-53 F) is far inside that margin."""
    r = region.astype(np.float64)
    D = 0.0
    if r.shape[-1] > 1:
        D = max(D, float(np.abs(np.diff(r, axis=-1)).max()))
    if r.shape[-2] > 1:
        D = max(D, float(np.abs(np.diff(r, axis=-2)).max()))
    Fm = float(np.abs(r).max())
    dx, dy = position_bound(cw, flip), position_bound(ch)
    return (dx[None, :] + dy[:, None]) * D + EPS * (5.0 * D + 3.0 * Fm)


def witness(plane, row):
    """float64 torch bilinear interpolation (align_corners=False, no antialiasing) of the cropped, mirrored region."""
    _, top, left, ch, cw, flip = (int(v) for v in row)
    reg = np.ascontiguousarray(plane[top:top + ch, left:left + cw].astype(np.float64))
    if flip:
        reg = reg[:, ::-1].copy()
    t = torch.from_numpy(reg)[None, None]
    return torch.nn.functional.interpolate(t, size=(OUT, OUT), mode="bilinear", align_corners=False)[0, 0].numpy()


def s17_cases(h, w):
    """(top, left, ch, cw) of every size pair at its centre offset, plus degenerate 1x1 and 2x3 crops."""
    from video_analytics_amd import augment
    _, pairs = augment.scale_jitter_sizes(h, w)
    cases = []
    for cw, ch in pairs:
        left, top = augment.fixed_offsets(h, w, ch, cw)[4]
        cases.append((top, left, ch, cw))
    return cases + [(h - 1, w - 1, 1, 1), (7, 5, 2, 3)]


# ---- S18 ----

def test_scale_jitter_sizes_known_answers():
    from video_analytics_amd import augment
    sizes, pairs = augment.scale_jitter_sizes(240, 320)
    assert sizes == [240, 210, 180, 158]
    assert pairs == [(240, 240), (210, 240), (240, 210), (210, 210), (180, 210), (210, 180), (180, 180), (158, 180),
                     (180, 158), (158, 158)]
    assert augment.scale_jitter_sizes(256, 340)[0] == [256, 224, 192, 168]
    assert augment.scale_jitter_sizes(340, 256)[0] == [256, 224, 192, 168]
    assert augment.scale_jitter_sizes(255, 400)[0][1] == 224   # 223 is within 3 of 224
    assert augment.scale_jitter_sizes(252, 400)[0][1] == 220   # 220 is not
    assert len(augment.scale_jitter_sizes(224, 224)[1]) == 10


def test_fixed_offsets_order():
    from video_analytics_amd import augment
    got = augment.fixed_offsets(240, 320, 180, 210)
    ws, hs = (320 - 210) // 4, (240 - 180) // 4
    assert (ws, hs) == (27, 15)
    assert got == [(0, 0), (108, 0), (0, 60), (108, 60), (54, 30), (0, 30), (108, 30), (54, 60), (54, 0), (27, 15), (81, 15),
                   (27, 45), (81, 45)]
    assert augment.fixed_offsets(240, 320, 180, 210, more=False) == got[:5]
    assert set(augment.fixed_offsets(224, 224, 224, 224)) == {(0, 0)}


@pytest.mark.parametrize("h,w", [(240, 320), (256, 340), (224, 224)])
@pytest.mark.parametrize("fix,more", [(True, True), (True, False), (False, True)])
def test_drawn_crops_lie_inside_the_frame_in_a_fixed_draw_order(h, w, fix, more):
    from video_analytics_amd import augment
    n = 200
    got = augment.draw_scale_jitter_crops(n, h, w, random.Random(5), fix=fix, more=more)
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 5)
    augment.check_jitter_crops(got, n, h, w, "test")
    top, left, ch, cw, flip = (got[:, i] for i in range(5))
    assert bool((top >= 0).all()) and bool((left >= 0).all()) and bool((top + ch <= h).all()) and bool((left + cw <= w).all())
    assert set(flip.tolist()) == {0, 1}
    # the draws, restated: choice of the pair, choice of the offset (or two randints), one random() for the flip
    rng = random.Random(5)
    _, pairs = augment.scale_jitter_sizes(h, w)
    ref = []
    for _ in range(n):
        cw_, ch_ = rng.choice(pairs)
        if fix:
            l_, t_ = rng.choice(augment.fixed_offsets(h, w, ch_, cw_, more))
        else:
            l_ = rng.randint(0, w - cw_)
            t_ = rng.randint(0, h - ch_)
        ref.append([t_, l_, ch_, cw_, int(rng.random() < 0.5)])
    assert got.tolist() == ref
    assert len(set((r[3], r[2]) for r in ref)) == len(set(pairs))  # every size pair is drawn
    # the global generator is the default
    random.seed(11)
    a = augment.draw_scale_jitter_crops(4, h, w, fix=fix, more=more)
    assert a.tolist() == augment.draw_scale_jitter_crops(4, h, w, random.Random(11), fix=fix, more=more).tolist()


def test_snippet_tables_expand_one_crop_per_snippet():
    from video_analytics_amd import augment
    crops = torch.tensor([[3, 5, 180, 210, 1], [0, 0, 240, 240, 0]], dtype=torch.int32)
    rgb, fl = augment.snippet_tables(crops, [4, 9], [7, 0], 2)
    assert rgb.tolist() == [[4, 3, 5, 180, 210, 1], [9, 0, 0, 240, 240, 0]]
    assert fl.tolist() == [[14 + c, 3, 5, 180, 210, 1] for c in range(4)] + [[c, 0, 0, 240, 240, 0] for c in range(4)]
    assert rgb.dtype == torch.int32 and fl.dtype == torch.int32
    augment.check_resize_table(rgb, 10, 240, 320, "test")
    augment.check_resize_table(fl, 18, 240, 320, "test")
    for bad in ([[10, 0, 0, 224, 224, 0]], [[-1, 0, 0, 224, 224, 0]], [[0, 17, 0, 224, 224, 0]], [[0, 0, 97, 224, 224, 0]],
                [[0, 0, 0, 0, 224, 0]], [[0, 0, 0, 224, 321, 0]], [[0, -1, 0, 224, 224, 0]], [[0, 0, 0, 224, 224, 2]]):
        with pytest.raises(ValueError):
            augment.check_resize_table(torch.tensor(bad, dtype=torch.int32), 10, 240, 320, "test")
    for bad in (torch.zeros(0, 6, dtype=torch.int32), torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 6), [[0] * 6]):
        with pytest.raises(ValueError):
            augment.check_resize_table(bad, 10, 240, 320, "test")
    with pytest.raises(ValueError):
        augment.snippet_tables(crops, [4], [7, 0], 2)
    with pytest.raises(ValueError):
        augment.check_jitter_crops(crops, 3, 240, 320, "test")


# ---- S19 ----

@pytest.mark.parametrize("k", [1, 3, 7])
def test_segment_starts_are_in_range_ordered_and_one_per_segment(k):
    from video_analytics_amd.video import segmentPlan, segmentStarts
    L = 10
    rng = random.Random(k)
    for T in range(L + 1, 402):
        P = T - 1
        st = segmentStarts(T, k, L, rng)
        assert len(st) == k and all(0 <= s <= P - L for s in st), (T, st)
        assert st == sorted(st), (T, st)
        avg = (P - L + 1) // k
        if avg > 0:
            assert all(i * avg <= s < (i + 1) * avg for i, s in enumerate(st)), (T, st)
        plan = segmentPlan(T, st, L)
        assert plan.pairs == sorted(set(plan.pairs)) and plan.pair_computations == len(plan.pairs) <= min(P, k * L)
        assert plan.sequences == [(p, p + 1) for p in plan.pairs]
        for s, j in zip(st, plan.index):
            assert plan.pairs[j:j + L] == list(range(s, s + L))
    with pytest.raises(ValueError):
        segmentStarts(L, k, L, rng)  # P = L - 1: no window
    with pytest.raises(ValueError):
        segmentStarts(40, 0, L, rng)
    with pytest.raises(ValueError):
        segmentPlan(21, [0, 11], L)   # the window from 11 leaves the 20 pairs
    with pytest.raises(ValueError):
        segmentPlan(21, [-1], L)


def test_segment_starts_draw_order():
    from video_analytics_amd.video import segmentStarts
    rng, ref = random.Random(3), random.Random(3)
    assert segmentStarts(100, 3, 10, rng) == [i * 30 + ref.randrange(30) for i in range(3)]   # P - L + 1 = 90
    assert segmentStarts(13, 3, 10, rng) == sorted(ref.randrange(3) for _ in range(3))        # avg = 0: 3 starts
    assert segmentStarts(11, 3, 10, rng) == [0, 0, 0]
    random.seed(8)
    a = segmentStarts(64, 3, 10)
    assert a == segmentStarts(64, 3, 10, random.Random(8))


# ---- S17 on the host ----

@pytest.mark.parametrize("size", sorted({240, 210, 180, 158, 256, 224, 192, 168, 320, 1, 2, 3, 241, 147}))
def test_positions_against_exact_rationals(size):
    worst = 0.0
    for flip in (False, True):
        i0, i1, a, u, _, _ = s17_taps(size, flip)
        bound = position_bound(size, flip)
        for x in range(OUT):
            o = OUT - 1 - x if flip else x
            exact = Fraction(2 * o + 1, 2) * Fraction(size, 224) - Fraction(1, 2)
            exact = min(max(exact, Fraction(0)), Fraction(size - 1))
            err = abs(Fraction(float(u[x])) - exact)
            worst = max(worst, float(err))
            assert err <= Fraction(float(bound[x])), (size, flip, x, float(err), float(bound[x]))
            assert Fraction(float(a[x])) == Fraction(float(u[x])) - int(i0[x])  # the weight is exact
            assert 0 <= i0[x] <= i1[x] <= size - 1 and i1[x] - i0[x] <= 1 and 0.0 <= a[x] < 1.0
    print("size %d: max |u - u*| = %.3g (bound %.3g = %.1f * 2^-24)" % (size, worst, bound.max(), bound.max() / EPS))
    if size == 224:
        assert worst == 0.0 and not s17_taps(224)[2].any() and not s17_taps(224, True)[2].any()


@pytest.mark.parametrize("h,w", [(240, 320), (241, 321)])
def test_restatement_against_the_float64_witness(h, w):
    rs = np.random.RandomState(h)
    plane = (rs.standard_normal((h, w)) * 12.0).astype(F32)
    fmax = float(np.abs(plane).max())
    worst = 0.0
    for (top, left, ch, cw) in s17_cases(h, w):
        for flip in (0, 1):
            row = (0, top, left, ch, cw, flip)
            got = s17_resize(plane, row).astype(np.float64)
            ref = witness(plane, row)
            tol = value_tolerance(plane[top:top + ch, left:left + cw], ch, cw, bool(flip))
            err = np.abs(got - ref)
            worst = max(worst, float(err.max()))
            print("%dx%d crop %dx%d at (%d,%d) flip %d: max |restatement - witness| = %.3g = %.1f * 2^-24 * max|f| "
                  "(tolerance %.3g .. %.3g)" % (w, h, cw, ch, left, top, flip, err.max(), err.max() / (EPS * fmax), tol.min(),
                                               tol.max()))
            assert (err <= tol).all(), (row, float(err.max()), float(tol.max()))
    print("worst over the cases: %.3g = %.1f * 2^-24 * max|f|" % (worst, worst / (EPS * fmax)))


@pytest.mark.parametrize("h,w", [(240, 320), (224, 224), (241, 321)])
def test_restatement_at_224_is_the_plain_crop(h, w):
    rs = np.random.RandomState(w)
    plane = (rs.standard_normal((h, w)) * 12.0).astype(F32)
    for top, left in ((0, 0), (h - 224, w - 224), ((h - 224) // 2, (w - 224) // 3)):
        win = plane[top:top + 224, left:left + 224]
        assert np.array_equal(s17_resize(plane, (0, top, left, 224, 224, 0)), win)
        assert np.array_equal(s17_resize(plane, (0, top, left, 224, 224, 1)), win[:, ::-1])
    fl = plane[None, None].repeat(2, axis=1)
    t0, l0 = min(3, h - 224), min(2, w - 224)
    tab = [[1, t0, l0, 224, 224, 1], [0, t0, l0, 224, 224, 1]]
    win = plane[t0:t0 + 224, l0:l0 + 224][:, ::-1]
    assert np.array_equal(s17_flow_stack(fl, tab)[0], s9_quantise(win))
    assert np.array_equal(s17_flow_stack(fl, tab, True)[0], s9_quantise(win))  # an odd plane (y flow) is never inverted
    assert np.array_equal(s17_flow_stack(fl, tab, True)[1], s9_quantise(win, invert=True))


@pytest.mark.parametrize("h,w", [(240, 320), (241, 321)])
def test_u8_restatement_rounds_as_the_witness_away_from_ties(h, w):
    """Where the witness is farther from a tie (k + 1/2) than the value tolerance, rint of the restatement's float32 value
    must be rint of the witness; elsewhere either neighbour may come out.  At most 2 % of a case's pixels may be that close."""
    rs = np.random.RandomState(w)
    img = rs.randint(0, 256, size=(1, 1, h, w)).astype(np.uint8)
    for (top, left, ch, cw) in s17_cases(h, w):
        for flip in (0, 1):
            row = (0, top, left, ch, cw, flip)
            got = s17_images_u8(img, [row])[0, 0].astype(np.int64)
            ref = witness(img[0, 0], row)
            tol = value_tolerance(img[0, 0, top:top + ch, left:left + cw], ch, cw, bool(flip))
            tie = np.abs(ref - np.floor(ref) - 0.5)
            near = tie <= tol
            want = np.rint(np.clip(ref, 0.0, 255.0)).astype(np.int64)
            verr = float(np.abs(s17_resize(img[0, 0].astype(F32), row).astype(np.float64) - ref).max())
            print("%dx%d u8 crop %dx%d flip %d: %.3f %% of the pixels within the tolerance (<= %.3g) of a tie, max value "
                  "error %.3g" % (w, h, cw, ch, flip, 100.0 * near.mean(), tol.max(), verr))
            assert np.array_equal(got[~near], want[~near]), row
            assert int(np.abs(got - want).max()) <= 1, row
            assert near.mean() <= 0.02, (row, float(near.mean()))
    # NHWC input: the same numbers
    nhwc = np.ascontiguousarray(rs.randint(0, 256, size=(2, h, w, 3)).astype(np.uint8))
    tab = [[1, 3, 5, 180, 210, 1], [0, 0, 0, h, w, 0]]
    assert np.array_equal(s17_images_u8(nhwc, tab, "NHWC"), s17_images_u8(nhwc.transpose(0, 3, 1, 2), tab))


# ---- S20 ----

def s20_consensus_loss(z, y):
    """The consensus loss in float32, in the kernel's order: z [n,k,c], labels [n] -> (loss, hits, dz [n,k,c], m [n,c])."""
    z = np.asarray(z, dtype=F32)
    n, k, c = z.shape
    m = z[:, 0].copy()
    for j in range(1, k):
        m = m + z[:, j]
    m = m / F32(k)
    inv_n = F32(1.0) / F32(n)
    loss, hits = F32(0.0), 0
    dz = np.empty_like(z)
    for v in range(n):
        l = m[v]
        mx, am = l[0], 0
        for j in range(1, c):
            if l[j] > mx:
                mx, am = l[j], j
        e = np.exp(l - mx)
        se = F32(0.0)
        for j in range(c):
            se = se + e[j]
        loss = loss + ((np.log(se) + mx) - l[int(y[v])])
        hits += int(am == int(y[v]))
        onehot = np.zeros(c, dtype=F32)
        onehot[int(y[v])] = 1.0
        g = (e * (F32(1.0) / se) - onehot) * inv_n
        dz[v] = (g / F32(k))[None, :]
    return F32(loss * inv_n), hits, dz, m


@pytest.mark.parametrize("n,k,c,scale", [(8, 3, 101, 3.0), (2, 1, 7, 1.0), (5, 7, 101, 30.0), (1, 25, 300, 10.0), (64, 1, 101, 5.0)])
def test_consensus_loss_against_float64_autograd(n, k, c, scale):
    """Against cross_entropy(z.mean(1), y) in float64.  Error budget, with Z = max |z| and R the spread of the means:
    a mean carries k roundings of magnitudes <= Z: k EPS Z; the exponent l - mx then carries 2 k EPS Z + EPS R, which is the
    exponential's relative error, plus 2 EPS for exp itself; the sum of c terms adds c EPS, the reciprocal, the two products
    and the division by k four more: every softmax entry (<= 1) is within (2 k Z + R + c + 8) EPS, and dz is that over n k.
    The loss per video: log of the sum (its relative error, c + 2 k Z + R + 2 roundings, becomes absolute), mx and the
    label's mean (k Z each), two additions; the mean over n videos adds n roundings of the loss itself."""
    rs = np.random.RandomState(n * 100 + k)
    z = (rs.standard_normal((n, k, c)) * scale).astype(F32)
    y = rs.randint(0, c, size=n)
    loss, hits, dz, m = s20_consensus_loss(z, y)
    zt = torch.from_numpy(z.astype(np.float64)).requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(zt.mean(1), torch.from_numpy(y).long())
    ref.backward()
    Z = float(np.abs(z).max())
    R = float(m.max(axis=1).max() - m.min(axis=1).min())
    tol_dz = (2 * k * Z + R + c + 8) * EPS / (n * k)
    tol_loss = (c + 4 * k * Z + 2 * R + n + 8) * EPS * max(1.0, float(ref.detach()))
    e_dz = float(np.abs(dz.astype(np.float64) - zt.grad.numpy()).max())
    e_loss = abs(float(loss) - float(ref.detach()))
    print("n=%d k=%d c=%d: |loss - witness| = %.3g (tolerance %.3g), max |dz - witness| = %.3g (tolerance %.3g)"
          % (n, k, c, e_loss, tol_loss, e_dz, tol_dz))
    assert e_loss <= tol_loss and e_dz <= tol_dz
    assert hits == int((zt.detach().mean(1).argmax(1).numpy() == y).sum())
    assert all(np.array_equal(dz[:, 0], dz[:, j]) for j in range(k))
    if k == 1:
        assert np.array_equal(m, z[:, 0])
