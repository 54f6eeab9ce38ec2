"""Every stage of the fusion SVM's fit on its own (``va_linear_svm_fit_phase``) against the long-double
stage reference tests/svm_stage_reference.py, in a workspace the test owns (``va_linear_svm_fit_layout``), prefilled with NaN.

Every operation is held from the inputs the device itself had: the margins M from the planted W; U bit for bit from the
device's M; f from the device's M; G and H P from the device's U; the CG update from the device's H P; the line search's
decisions from the device's Q.  The one tolerance is the reference's rule ``2 L 2^-53 S`` (L terms, S the sum of their
magnitudes); errors are printed in units of it.  Decisions (active set, stop rule, end of the CG, Armijo) are compared
everywhere: the seeds are such that no margin of the reference lies inside the error bound of what is decided
(tests/test_svm_stages_host.py asserts that, and the tests here assert it again on the device's own values).

Forty failed trials of the line search with a descent direction CAN be constructed: S = -sigma G with sigma 2^41 Armijo
roots leaves t = 2^-39 still four roots long.  Those rows are in every line-search case with at least nine class rows.

Figures printed on the MI355X, the worst over all cases, errors in units of the bound each is held to (so held to 1):
    eval         M 0.198    f 0.031    G 0.0615   rr 0.0352   gn 0.468 (of one ulp)   cgtol 0.232 (of four ulps)
    CG step      U 0.0738   HP 0.0181  S' 0.488   R' 0.477    rr' 0.05   P' 0.579
    line search  Q 0.141; the smallest distance of an Armijo decision from its threshold, 3.0e12 bounds (must exceed 1)
    inside a real fit, worst |(-G - H S) - R| / |G| after a CG x 100: golden problem 4 9.06e-15, problem 6 1.67e-14, held to
    1e-11 (the float64 restatement on a CPU: 3.7e-14; both below 1e-12, so nothing to explain); worst |R| / cgtol where the CG
    ended early 0.9998 and 0.997, held to 1; no class-step's stored f' exceeded f + 1e-4 t G.S (13 and 14 Newton steps).
No kernel was found wrong: every stage passed as first written.
"""
import ctypes

import numpy as np
import pytest
import torch

import svm_fit_oracle as so
import svm_stage_reference as sr
from video_analytics_amd import _ffi, fusion

pytestmark = pytest.mark.gpu

INIT, EVAL_FIRST, EVAL, CG, LINE_SEARCH = range(5)
F64_2D = ("W", "G", "S", "R", "P", "HP")
F64_1D = ("f", "gn", "g0", "steps", "rr", "cgtol", "cgs")
LD, U53 = sr.LD, sr.U53


class Dev(object):
    """One problem on the device and a workspace filled with `fill`; fields are read and written by name."""

    def __init__(self, x, y, n_classes, C=1.0, scaling=1.0, tol=sr.TOL, fill=float("nan")):
        self.L = _ffi.lib()
        self.n, self.dim = x.shape
        self.n_classes, self.rows, self.D = n_classes, (1 if n_classes == 2 else n_classes), self.dim + 1
        self.scalars = (float(C), float(scaling), float(tol))
        self.x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).cuda()
        self.y = torch.as_tensor(np.ascontiguousarray(y, dtype=np.int32)).cuda()
        off = (ctypes.c_size_t * len(sr.FIELDS))()
        self.need = self.L.va_linear_svm_fit_layout(self.n, self.dim, self.rows, off, len(sr.FIELDS))
        assert self.need > 0 and self.need == self.L.va_linear_svm_fit_workspace_bytes(self.n, self.dim, self.rows)
        self.off = dict(zip(sr.FIELDS, list(off)))
        self.work = torch.full((self.need // 8,), fill, dtype=torch.float64, device="cuda")
        chunks, blocks = -(-self.n // 256), -(-self.n // 64)
        self.shape = dict([(k, (self.rows, self.D)) for k in F64_2D] + [(k, (self.n, self.rows)) for k in ("M", "U", "Q")]
                          + [("part", (chunks, self.rows, self.D)), ("losspart", (blocks, self.rows))]
                          + [(k, (self.rows,)) for k in F64_1D + ("live", "notdone")])

    @classmethod
    def of(cls, case, **kw):
        return cls(case.x, case.y, case.classes, case.C, case.scaling, case.tol, **kw)

    def view(self, name):
        shape = self.shape[name]
        count = int(np.prod(shape))
        if name in ("live", "notdone"):
            return self.work.view(torch.int32)[self.off[name] // 4: self.off[name] // 4 + count].view(shape)
        return self.work[self.off[name] // 8: self.off[name] // 8 + count].view(shape)

    def get(self, name):
        return self.view(name).cpu().numpy().copy()

    def bits(self, name):
        a = self.get(name)
        return a.view(np.int64) if a.dtype == np.float64 else a

    def put(self, **fields):
        for name, a in fields.items():
            dtype = np.int32 if name in ("live", "notdone") else np.float64
            a = np.broadcast_to(np.asarray(a, dtype=dtype), self.shape[name]).copy()
            self.view(name).copy_(torch.as_tensor(a))

    def phase(self, phase, count=1):
        C, s, tol = self.scalars
        rc = self.L.va_linear_svm_fit_phase(_ffi.ctx(0), _ffi.ptr(self.x), _ffi.ptr(self.y), self.n, self.dim, self.n_classes, C, s, tol, phase,
                                            count, _ffi.ptr(self.work), self.need, _ffi.stream_ptr(self.x))
        assert rc == _ffi.VA_OK, self.L.va_last_error()

    def raw(self):
        return self.work.view(torch.int64).cpu().numpy().copy()

    def state(self, *names):
        return dict((k, self.get(k)) for k in names)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)


def worst(x):
    x = np.asarray(x, dtype=np.float64)
    return float(x.max()) if x.size else 0.0


def check_eval(d, case, plant, first, integer=False):
    """Plant, run one eval phase, hold everything it writes and everything it must leave alone -> worst errors by stage."""
    p = case.p
    on = np.asarray(plant["notdone"]) != 0
    live_in = np.where(on, 0, 5).astype(np.int32)  # a stopped row keeps its (odd) live value
    d.put(W=plant["W"], notdone=plant["notdone"], g0=plant["g0"], live=live_in)
    before = dict((k, d.bits(k)) for k in F64_2D + F64_1D)
    d.phase(EVAL_FIRST if first else EVAL)
    st = dict(plant, live=live_in)
    out0, mag0, dec0 = sr.eval(p, st, first)
    Yt = p.Y.T.astype(np.float64)
    M, U = d.get("M"), d.get("U")
    err = {}
    if integer:
        assert np.array_equal(M[:, on], out0["M"][:, on].astype(np.float64))
        assert ((1.0 - Yt * M == 0)[:, on]).sum() >= 10 and not (U[:, on][(1.0 - Yt * M == 0)[:, on]] != 0).any()
        err["M"] = 0.0
    else:
        bM = sr.bound(p.L_fwd, mag0["M"])
        err["M"] = worst(sr.nerr(M, out0["M"], bM)[:, on])
        assert not (dec0["act_margin"] <= bM)[:, on].any(), "the reference's active set is decided outside the bound"
        assert not (np.abs(1.0 - Yt * M) <= bM)[:, on].any(), "and so is the device's"
    assert same_bits(U[:, on], np.where(1.0 - Yt * M > 0.0, M - Yt, 0.0)[:, on]), "U from the device's M, bit for bit"
    assert np.array_equal((1.0 - Yt * M > 0.0)[:, on], dec0["act"][:, on])
    G = d.get("G")
    out1, mag1, _ = sr.eval(p, st, first, given=dict(M=M, U=U))
    err["f"] = worst(sr.nerr(d.get("f"), out1["f"], mag1["f_bound"])[on])
    err["G"] = worst(sr.nerr(G, out1["G"], sr.bound(p.L_xtu, mag1["G"]))[on])
    assert same_bits(d.get("R")[on], -G[on]) and same_bits(d.get("P")[on], -G[on]) and (d.bits("S")[on] == 0).all()
    gn, g0, rr = d.get("gn"), d.get("g0"), d.get("rr")
    rr_ref = (sr.ld(G) ** 2).sum(1)
    err["rr"] = worst(sr.nerr(rr, rr_ref, sr.bound(p.L_dot, rr_ref))[on])
    err["gn"] = worst(sr.nerr(gn, np.sqrt(sr.ld(rr)), 2 * U53 * sr.ld(gn))[on])  # one rounding of the square root, at most an ulp
    assert same_bits(g0[on], gn[on] if first else np.asarray(plant["g0"], dtype=np.float64)[on])
    with np.errstate(invalid="ignore", divide="ignore"):
        cgtol_ref = np.minimum(LD(0.1), np.sqrt(sr.ld(gn) / sr.ld(g0))) * sr.ld(gn)
    err["cgtol"] = worst(sr.nerr(d.get("cgtol"), cgtol_ref, 8 * U53 * cgtol_ref)[on])  # a division, a square root, a product
    go_on = ~(gn <= case.tol * g0)
    assert np.array_equal(go_on[on], ~dec0["stop"][on]), "the stop rule decides as the reference does"
    assert not (dec0["stop_margin"] <= sr.bound(p.L_dot, out0["gn"]))[on].any()
    assert np.array_equal(d.get("notdone"), np.where(on, go_on, 0)) and np.array_equal(d.get("live"), np.where(on, go_on, 5))
    for k in F64_2D + F64_1D:  # a stopped row keeps every bit; eval never writes HP
        rows = ~on if k != "HP" else np.ones_like(on)
        assert np.array_equal(d.bits(k)[rows], before[k][rows]), k
    assert max(err.values()) <= 1.0, err
    return err, dict(M=M, U=U, G=G, f=d.get("f"), gn=gn, cgtol=d.get("cgtol"), on=on)


def run_eval_case(case, integer=False):
    """EVAL_FIRST and EVAL, under two notdone patterns and two prefills; what a row gets depends on neither."""
    errs, seen = {}, []
    for pattern, fill in (("all", float("nan")), ("alternate", 0.0)):
        plant = sr.eval_plant(case, pattern)
        for first in (True, False):
            d = Dev.of(case, fill=fill)
            err, got = check_eval(d, case, plant, first, integer)
            for k, v in err.items():
                errs[k] = max(errs.get(k, 0.0), v)
            seen.append((first, got))
    for first in (True, False):
        (a, b) = [g for f, g in seen if f == first]
        both = a["on"] & b["on"]
        for k in ("G", "f", "gn", "cgtol"):
            assert same_bits(a[k][both], b[k][both]), k
        assert same_bits(a["M"][:, both], b["M"][:, both]) and same_bits(a["U"][:, both], b["U"][:, both])
    return errs


@pytest.mark.parametrize("case", sr.CASES, ids=sr.CASE_IDS)
def test_eval_at_an_arbitrary_iterate(case):
    case = sr.Case(*case)
    errs = run_eval_case(case)
    print("eval %s: worst error / bound: %s" % (sr.CASE_IDS[sr.CASES.index((case.n, case.dim, case.classes, case.scaling, case.C))],
                                                 ", ".join("%s %.3g" % kv for kv in sorted(errs.items()))))


def test_eval_with_integer_margins_exactly_at_the_hinge():
    """Integer x and W: every margin is exact, some equal y (h = 0), and those entries are inactive: the inequality is strict."""
    errs = run_eval_case(sr.Case(257, 63, 65, integer=True), integer=True)
    print("eval integer: worst error / bound: %s" % ", ".join("%s %.3g" % kv for kv in sorted(errs.items())))


def mini_newton(d):
    d.phase(EVAL_FIRST)
    d.phase(CG, 2)
    d.phase(LINE_SEARCH)
    d.phase(EVAL)


@pytest.mark.parametrize("shape,pattern", [((63, 16, 17), "alternate"), ((513, 64, 130), "tile"), ((257, 63, 65), "one")])
def test_dead_rows_and_dead_tiles(shape, pattern):
    """Stopped rows keep every bit through a whole Newton step; a tile of 64 stopped classes is never touched (its columns of
    M U Q, its rows of part and its entries of losspart keep the NaN prefill); NaN in a stopped row's vectors changes no
    running row's result by a bit."""
    case = sr.Case(*shape)
    notdone = sr.eval_plant(case, pattern)["notdone"]
    on = notdone != 0
    rng = np.random.RandomState(11)
    runs = []
    for poison in (False, True):
        d = Dev.of(case)
        vec = dict((k, rng.randn(case.rows, case.D)) for k in F64_2D)
        if poison:
            for k in F64_2D:
                vec[k][~on] = np.nan
        vec["W"][on] = case.W[on]
        d.put(notdone=notdone, live=0, **vec)
        d.put(**dict((k, np.where(on, 0.0, 3.0 + i)) for i, k in enumerate(F64_1D)))
        before = dict((k, d.bits(k)) for k in F64_2D + F64_1D)
        mini_newton(d)
        for k in F64_2D + F64_1D:
            assert np.array_equal(d.bits(k)[~on], before[k][~on]), k
        assert (d.get("notdone")[~on] == 0).all() and (d.get("live")[~on] == 0).all()
        assert (d.get("steps")[on] == 1).all() and (d.get("cgs")[on] >= 1).all() and np.isfinite(d.get("W")[on]).all()
        if pattern == "tile":
            dead = slice(64, 128)
            for k in ("M", "U", "Q"):
                assert np.isnan(d.get(k)[:, dead]).all(), k
                assert np.isfinite(d.get(k)[:, on]).all(), k
            assert np.isnan(d.get("part")[:, dead, :]).all() and np.isnan(d.get("losspart")[:, dead]).all()
            assert np.isfinite(d.get("part")[:, on, :]).all() and np.isfinite(d.get("losspart")[:, on]).all()
        runs.append(d)
    a, b = runs
    for k in F64_2D + F64_1D + ("live", "notdone"):
        assert same_bits(a.get(k)[on], b.get(k)[on]), k
    for k in ("M", "U", "Q"):
        assert same_bits(a.get(k)[:, on], b.get(k)[:, on]), k
    assert same_bits(a.get("part")[:, on, :], b.get("part")[:, on, :]) and same_bits(a.get("losspart")[:, on], b.get("losspart")[:, on])


@pytest.mark.parametrize("case", sr.CASES, ids=sr.CASE_IDS)
def test_one_cg_step_from_an_arbitrary_state(case):
    case = sr.Case(*case)
    p = case.p
    d = Dev.of(case)
    d.put(W=case.W, notdone=1, live=0, g0=1.0)
    d.phase(EVAL_FIRST)
    M = d.get("M")
    st = sr.cg_plant(case, M)
    live = st["live"] != 0
    plant = dict((k, st[k]) for k in ("P", "R", "S", "HP", "rr", "cgtol", "cgs", "live"))
    d.put(**plant)
    before = dict((k, d.bits(k)) for k in F64_2D + F64_1D)
    d.phase(CG, 1)
    out0, mag0, dec0 = sr.cg_step(p, st)
    stepped, goes = live & dec0["php_positive"], out0["live"] != 0
    err = {}
    U, HP, S1, R1, P1, rr1 = (d.get(k) for k in ("U", "HP", "S", "R", "P", "rr"))
    err["U"] = worst(sr.nerr(U, out0["U"], sr.bound(p.L_fwd, mag0["U"]))[:, live])
    assert not (U[:, live][~p.active(M)[0][:, live]] != 0).any(), "inactive entries are exactly 0"
    out1, mag1, _ = sr.cg_step(p, st, given=dict(U=np.where(live[None, :], U, 0.0)))
    err["HP"] = worst(sr.nerr(HP, out1["HP"], sr.bound(p.L_xtu, mag1["HP"]))[live])
    out2, mag2, dec2 = sr.cg_step(p, st, given=dict(U=np.where(live[None, :], U, 0.0), HP=np.where(live[:, None], HP, 0.0)))
    err["S"] = worst(sr.nerr(S1, out2["S"], mag2["S_bound"])[stepped])
    err["R"] = worst(sr.nerr(R1, out2["R"], mag2["R_bound"])[stepped])
    rn_ref = (sr.ld(R1) ** 2).sum(1)
    err["rr"] = worst(sr.nerr(rr1, rn_ref, sr.bound(p.L_dot, rn_ref))[goes])
    # the decisions, from the device's own R': outside the bound on both sides, and the reference's
    rnorm = np.sqrt(rn_ref)
    assert not (np.abs(rnorm - st["cgtol"]) <= sr.bound(p.L_dot, rnorm))[stepped].any()
    assert not (dec0["cg_end_margin"] <= sr.bound(p.L_dot, rnorm))[stepped].any()
    assert np.array_equal(d.get("live"), out0["live"]) and np.array_equal(d.get("live")[stepped], (rnorm > st["cgtol"])[stepped])
    assert goes.sum() >= stepped.sum() // 2 and (stepped & ~goes).sum() >= stepped.sum() // 2 - 1, "half go on, half end"
    assert same_bits(d.get("cgs"), st["cgs"] + stepped)
    given = dict(U=np.where(live[None, :], U, 0.0), HP=np.where(live[:, None], HP, 0.0), S=np.where(stepped[:, None], S1, 0.0),
                 R=np.where(stepped[:, None], R1, 0.0), rn=np.where(goes, rr1, rn_ref))
    out3, mag3, _ = sr.cg_step(p, st, given=given)
    err["P"] = worst(sr.nerr(P1, out3["P"], mag3["P_bound"])[goes])
    # what must keep its bits: P and rr of a row whose CG ended; S, R of a row with P = 0 (its H P is 0); everything of a row
    # that was not live; W, G and the scalars the CG does not own everywhere
    assert np.array_equal(d.bits("P")[~goes], before["P"][~goes]) and np.array_equal(d.bits("rr")[~goes], before["rr"][~goes])
    for k in ("S", "R"):
        assert np.array_equal(d.bits(k)[~stepped], before[k][~stepped]), k
    if case.rows > 1:
        assert live[1] and not stepped[1] and (HP[1] == 0).all() and d.get("live")[1] == 0
    assert np.array_equal(d.bits("HP")[~live], before["HP"][~live])
    for k in ("W", "G", "f", "gn", "g0", "steps", "cgtol"):
        assert np.array_equal(d.bits(k), before[k]), k
    print("cg %s: worst error / bound: %s" % (sr.CASE_IDS[sr.CASES.index((case.n, case.dim, case.classes, case.scaling, case.C))],
                                               ", ".join("%s %.3g" % kv for kv in sorted(err.items()))))
    assert max(err.values()) <= 1.0, err


@pytest.mark.parametrize("shape", [(63, 16, 17), (513, 64, 130)])
def test_three_cg_rounds_in_one_call_are_three_calls(shape):
    case = sr.Case(*shape)
    raws = []
    for counts in ((3,), (1, 1, 1)):
        d = Dev.of(case)
        d.put(W=case.W, notdone=1, live=0, g0=1.0)
        d.phase(EVAL_FIRST)
        st = sr.cg_plant(case, d.get("M"))
        st["cgtol"] = np.zeros(case.rows)  # every live row goes on
        d.put(**dict((k, st[k]) for k in ("P", "R", "S", "HP", "rr", "cgtol", "cgs", "live")))
        for c in counts:
            d.phase(CG, c)
        raws.append(d.raw())
        live = st["live"] != 0
        stepped = live & (np.abs(st["P"]).sum(1) > 0)
        assert np.array_equal(d.get("cgs"), st["cgs"] + 3 * stepped) and np.array_equal(d.get("live"), stepped.astype(np.int32))
    assert np.array_equal(raws[0], raws[1])


@pytest.mark.parametrize("case", sr.CASES, ids=sr.CASE_IDS)
def test_line_search_from_an_arbitrary_direction(case):
    case = sr.Case(*case)
    p = case.p
    d = Dev.of(case)
    d.put(W=case.W, notdone=1, live=0, g0=1.0)
    d.phase(EVAL_FIRST)
    G, M = d.get("G"), d.get("M")
    ls, kind = sr.ls_plant(case, case.W, G, M)
    on = ls["notdone"] != 0
    d.put(S=ls["S"], steps=ls["steps"], notdone=ls["notdone"])
    before = dict((k, d.bits(k)) for k in F64_2D + F64_1D)
    d.phase(LINE_SEARCH)
    out0, mag0, dec0 = sr.line_search(p, ls)
    Q = d.get("Q")
    err = dict(Q=worst(sr.nerr(Q, out0["Q"], sr.bound(p.L_fwd, mag0["Q"]))[:, on]))
    out1, _, dec1 = sr.line_search(p, ls, given=dict(Q=np.where(on[None, :], Q, 0.0)))
    for dec in (dec0, dec1):  # no decision inside its bound, by the reference's Q and by the device's
        assert not (dec["descent_margin"] <= dec["descent_bound"])[on].any() and not (dec["armijo_margin_over_bound"] <= 1)[on].any()
    t = dec1["t"].astype(np.float64)
    assert np.array_equal(t, dec0["t"].astype(np.float64))
    assert np.array_equal(t, np.where(kind <= 6, 0.5 ** np.minimum(kind, 6), 0.0)), "the planted step lengths: 1 .. 2^-6, refused, 40 failures"
    found = t > 0
    W1 = d.get("W")
    assert same_bits(W1[found], (case.W + t[:, None] * np.nan_to_num(ls["S"]))[found]), "W + t S, bit for bit"
    assert np.array_equal(d.bits("W")[~found], before["W"][~found])
    assert same_bits(d.get("steps"), ls["steps"] + found)
    if case.rows >= sr.LS_KINDS:
        assert sorted(set(kind.tolist())) == list(range(sr.LS_KINDS))
    for k in ("G", "S", "R", "P", "HP", "f", "gn", "g0", "rr", "cgtol", "cgs"):
        assert np.array_equal(d.bits(k), before[k]), k
    print("line search %s: Q error / bound %.3g, smallest Armijo margin / bound %.3g, t %s" % (
        sr.CASE_IDS[sr.CASES.index((case.n, case.dim, case.classes, case.scaling, case.C))], err["Q"],
        float(dec1["armijo_margin_over_bound"][on & (kind != 7)].min()) if (on & (kind != 7)).any() else float("inf"), sorted(set(t.tolist()))))
    assert err["Q"] <= 1.0, err


def golden_problem(i):
    g = so.load_golden()[i]
    classes, y = fusion.check_svm_fit_args(g["X"], g["labels"])
    return g["X"], y, len(classes)


@pytest.mark.parametrize("i", [0, 3], ids=["problem1", "problem4"])
def test_phases_are_the_fit(i):
    """va_linear_svm_fit(restart = 1, newton_iters = k) leaves the bytes INIT, EVAL_FIRST, (CG x 100, LINE_SEARCH, EVAL) x k leave."""
    x, y, n_classes = golden_problem(i)
    for k in (0, 1, 3):
        a, b = Dev(x, y, n_classes), Dev(x, y, n_classes)
        coef = torch.zeros((a.rows, a.dim), dtype=torch.float64, device="cuda")
        intercept = torch.zeros((a.rows,), dtype=torch.float64, device="cuda")
        stats = torch.zeros((a.rows, 4), dtype=torch.float64, device="cuda")
        C, s, tol = a.scalars
        assert a.L.va_linear_svm_fit(_ffi.ctx(0), _ffi.ptr(a.x), _ffi.ptr(a.y), a.n, a.dim, n_classes, C, s, tol, k, 1, _ffi.ptr(coef),
                                     _ffi.ptr(intercept), _ffi.ptr(stats), _ffi.ptr(a.work), a.need, _ffi.stream_ptr(a.x)) == _ffi.VA_OK
        b.phase(INIT)
        b.phase(EVAL_FIRST)
        for _ in range(k):
            b.phase(CG, 100)
            b.phase(LINE_SEARCH)
            b.phase(EVAL)
        ra, rb = a.raw(), b.raw()
        assert np.array_equal(ra, rb), (k, int((ra != rb).sum()))
        assert same_bits(stats.cpu().numpy()[:, 3], b.get("steps")) and same_bits(coef.cpu().numpy(), b.get("W")[:, :-1])
        assert b.get("steps").max() == k


def test_phase_entry_point_rejects_bad_arguments_before_any_launch():
    x, y, n_classes = golden_problem(0)
    d = Dev(x, y, n_classes)
    raw = d.raw()
    C, s, tol = d.scalars

    def call(phase=EVAL, count=1, **over):
        a = dict(x=_ffi.ptr(d.x), y=_ffi.ptr(d.y), n=d.n, dim=d.dim, n_classes=n_classes, C=C, s=s, tol=tol, work=_ffi.ptr(d.work), need=d.need)
        a.update(over)
        return d.L.va_linear_svm_fit_phase(_ffi.ctx(0), a["x"], a["y"], a["n"], a["dim"], a["n_classes"], a["C"], a["s"], a["tol"], phase, count,
                                           a["work"], a["need"], _ffi.stream_ptr(d.x))

    for kw, msg in ((dict(phase=-1), "unknown phase"), (dict(phase=5), "unknown phase"), (dict(phase=CG, count=0), "1 <= count"),
                    (dict(phase=CG, count=101), "1 <= count"), (dict(C=0.0), "C must"), (dict(tol=float("nan")), "tol must"),
                    (dict(s=-1.0), "intercept_scaling must"), (dict(n=1), "n >= 2"), (dict(dim=8193), "1 <= dim"), (dict(n_classes=1), "n_classes"),
                    (dict(x=None), "NULL pointer"), (dict(work=None), "NULL pointer")):
        assert call(**kw) == _ffi.VA_ERR_INVALID, kw
        assert msg in d.L.va_last_error().decode(), (kw, d.L.va_last_error())
    assert call(need=d.need - 1) == _ffi.VA_ERR_WORKSPACE and str(d.need) in d.L.va_last_error().decode()
    assert d.L.va_linear_svm_fit_phase(None, _ffi.ptr(d.x), _ffi.ptr(d.y), d.n, d.dim, n_classes, C, s, tol, EVAL, 1, _ffi.ptr(d.work), d.need,
                                       None) == _ffi.VA_ERR_INVALID and b"ctx is NULL" in d.L.va_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d.raw(), raw), "nothing ran"
    assert call(phase=INIT, count=-7) == _ffi.VA_OK  # count is the CG phase's alone
    assert (d.get("W") == 0).all() and (d.get("notdone") == 1).all()


@pytest.mark.parametrize("i", [3, 5], ids=["problem4", "problem6"])
def test_cg_invariant_inside_a_real_fit(i):
    """Stepped by phases to convergence.  After every CG x 100, before the line search: the residual the recurrence carries is
    the true residual, |(-G - H S) - R| <= 1e-11 |G| with H from the device's own M (the float64 restatement on a CPU keeps
    3.7e-14 |G|; a product that loses a row, a chunk or the homogeneous column gives more than 1e-6 |G|:
    tests/test_svm_stages_host.py); |R| <= cgtol wherever the CG took fewer than 100 steps.  After the line search and the
    eval: f' <= f + 1e-4 t G.S, with f and f' evaluated in long double at the device's iterates and the error bound of the
    float64 sum the line search decided on (the stored f is rounded, and near the optimum the decrease is below its ulp)."""
    x, y, n_classes = golden_problem(i)
    p = sr.Problem(x, y, n_classes, tol=sr.TOL)
    d = Dev(x, y, n_classes)
    d.phase(INIT)
    d.phase(EVAL_FIRST)
    worst_gap, worst_r, rounded_f_up, iters = 0.0, 0.0, 0, 0
    for iters in range(1, 41):
        st0 = d.state("W", "G", "M", "f", "cgs", "notdone", "steps")
        on = st0["notdone"] != 0
        if not on.any():
            break
        d.phase(CG, 100)
        st = d.state("G", "S", "R", "M", "cgtol", "cgs", "live")
        assert same_bits(st["G"], st0["G"]) and same_bits(st["M"], st0["M"])
        res, _ = sr.true_residual(p, st)
        gnorm = np.sqrt((sr.ld(st["G"]) ** 2).sum(1))
        gap = (np.sqrt(((res - sr.ld(st["R"])) ** 2).sum(1)) / gnorm)[on]
        worst_gap = max(worst_gap, worst(gap))
        assert (gap <= 1e-11).all(), gap.max()
        took = st["cgs"] - st0["cgs"]
        rnorm = np.sqrt((sr.ld(st["R"]) ** 2).sum(1))
        ended = on & (took < 100)
        assert (took[on] >= 1).all() and (took[~on] == 0).all() and (st["live"][ended] == 0).all()
        worst_r = max(worst_r, worst((rnorm / sr.ld(st["cgtol"]))[ended]))
        assert (rnorm <= sr.ld(st["cgtol"]) + sr.bound(p.L_dot, rnorm))[ended].all()
        d.phase(LINE_SEARCH)
        W1, Q = d.get("W"), d.get("Q")
        d.phase(EVAL)
        stepped = d.get("steps") - st0["steps"]
        assert set(stepped[on].tolist()) <= {0.0, 1.0} and (stepped[~on] == 0).all() and same_bits(W1[~on], st0["W"][~on])
        # t from the iterates: W' = W + t S with t a power of two
        k = np.abs(st["S"]).argmax(1)
        r = np.arange(p.rows)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.where(stepped > 0, 2.0 ** np.round(np.log2(np.abs((W1[r, k] - st0["W"][r, k]) / st["S"][r, k]))), 0.0)
        assert same_bits(W1[on], (st0["W"] + t[:, None] * st["S"])[on]) and (t[on] <= 1).all()
        gs = (sr.ld(st["G"]) * sr.ld(st["S"])).sum(1)
        lsst = dict(W=st0["W"], S=st["S"], M=st["M"])
        delta, bnd = sr.ls_delta(p, lsst, sr.ld(t), Q)
        thr = sr.ARMIJO * sr.ld(t) * (gs + sr.bound(p.L_dot, np.abs(sr.ld(st["G"]) * sr.ld(st["S"])).sum(1)))
        assert (gs[on] < 0).all() and (delta <= thr + bnd)[on].all()
        # and f itself, in long double at both iterates.  delta is the same difference taken at the device's margins M and
        # M + t Q, which are off the exact ones by the bounds of the two products and one rounding of W + t S.
        f0, f1 = (sr.eval(p, dict(W=w, notdone=st0["notdone"]), True)[0]["f"] for w in (st0["W"], W1))
        dm = sr.bound(p.L_fwd, p.forward(st0["W"])[1]) + sr.ld(t) * sr.bound(p.L_fwd, p.forward(np.nan_to_num(st["S"]))[1]) \
            + 2 * U53 * p.forward(W1)[1]
        h0 = np.maximum(0, 1 - p.Y.T * sr.ld(st["M"]))
        ht = np.maximum(0, 1 - p.Y.T * (sr.ld(st["M"]) + sr.ld(t) * sr.ld(np.nan_to_num(Q))))
        slack = 2 * p.C * ((h0 + ht + dm) * dm).sum(0)
        assert (f1 - f0 <= thr + bnd + slack)[on].all()
        rounded_f_up += int((d.get("f") > st0["f"] + (sr.ARMIJO * sr.ld(t) * gs).astype(np.float64))[on].sum())
    print("problem %d: %d Newton steps; worst |true residual - R| / |G| = %.3g (held to 1e-11; float64 restatement on a CPU 3.7e-14); "
          "worst |R| / cgtol at the end of a CG = %.4g (held to 1); class-steps whose stored, rounded f' exceeds f + 1e-4 t G.S: %d"
          % (i + 1, iters - 1, worst_gap, worst_r, rounded_f_up))
    assert not d.get("notdone").any() and iters <= 30
    gn, g0 = d.get("gn"), d.get("g0")
    assert (gn <= sr.TOL * g0).all()
