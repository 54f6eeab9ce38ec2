"""The stage tests of the fusion SVM's fit, the parts that need no GPU: the layout entry point, the
long-double stage reference (tests/svm_stage_reference.py) composed into a fit, the mutation checks that show the GPU
assertions of tests/test_svm_stages_gpu.py have teeth, and the census of the reference's decisions on the chosen seeds."""
import ctypes

import numpy as np
import pytest

import svm_fit_oracle as so
import svm_stage_reference as sr
from video_analytics_amd import _ffi, fusion


def layout(n, dim, rows, count=len(sr.FIELDS)):
    off = (ctypes.c_size_t * max(count, 1))()
    return _ffi.lib().va_linear_svm_fit_layout(n, dim, rows, off, count), list(off)


@pytest.mark.parametrize("n,dim,classes", sr.SHAPES)
def test_layout_entry_point(n, dim, classes):
    L = _ffi.lib()
    rows, D = (1 if classes == 2 else classes), dim + 1
    total, off = layout(n, dim, rows)
    assert total > 0 and total == L.va_linear_svm_fit_workspace_bytes(n, dim, rows)
    assert off[0] == 0 and all(a < b for a, b in zip(off, off[1:])) and all(o % 256 == 0 for o in off)
    chunks, blocks = -(-n // 256), -(-n // 64)
    sizes = [8 * rows * D] * 6 + [8 * n * rows] * 3 + [8 * chunks * rows * D, 8 * blocks * rows] + [8 * rows] * 7 + [4 * rows] * 2
    assert len(sizes) == len(sr.FIELDS) == 20
    for i, size in enumerate(sizes):  # every field fits before the next one starts, with less than one alignment step to spare
        end = off[i + 1] if i + 1 < len(off) else total
        assert 0 <= end - off[i] - size < 256, sr.FIELDS[i]


def test_layout_entry_point_refuses_bad_sizes_and_counts():
    L = _ffi.lib()
    for bad in ((1, 8, 3), (10, 0, 3), (10, 8193, 3), (10, 8, 0), (10, 8, 2), (10, 8, 4097)):
        assert layout(*bad)[0] == 0, bad
        assert b"need n >= 2" in L.va_last_error()
    for count in (0, 19, 21, -1):
        total, off = layout(10, 8, 3, count)
        assert total == 0 and b"exactly 20 fields" in L.va_last_error(), count
        assert all(o == 0 for o in off), "nothing is written"
    assert L.va_linear_svm_fit_layout(10, 8, 3, None, 20) == 0 and b"NULL" in L.va_last_error()


def test_reference_stages_composed_reach_the_oracles_optimum():
    g = so.load_golden()[0]
    classes, y = fusion.check_svm_fit_args(g["X"], g["labels"])
    p = sr.Problem(g["X"], y, len(classes), tol=1e-8)
    st = sr.initial_state(p)
    for it in range(30):
        if not st["notdone"].any():
            break
        st, dec = sr.newton_step(p, st)
    W = st["W"].astype(np.float64)
    Xa, Y = so.augmented(g["X"]), so.signs(g["labels"], classes)
    gn = np.linalg.norm(so.gradient(W, Xa, Y), axis=1)
    g0 = np.linalg.norm(so.gradient(np.zeros_like(W), Xa, Y), axis=1)
    print("Newton steps %s, |g| / |g0| %.3g" % (st["steps"].astype(int).tolist(), (gn / g0).max()))
    assert not st["notdone"].any() and it <= 25 and (gn <= 2e-8 * g0).all()
    assert np.allclose(st["f"].astype(np.float64), so.objective(W, Xa, Y), rtol=1e-12, atol=0)
    assert np.allclose(st["g0"].astype(np.float64), g0, rtol=1e-12, atol=0)


@pytest.fixture(scope="module")
def mid_cg_states():
    """Golden problems 5 (two chunks, the last of 44 rows) and 6 (the last chunk is one row) in the middle of their second
    Newton step's CG: a state with S, R and P all far from zero."""
    out = []
    for i in (4, 5):
        g = so.load_golden()[i]
        classes, y = fusion.check_svm_fit_args(g["X"], g["labels"])
        if i == 4:  # classes 11 and up merged into one: 12 class rows are enough, and quicker in long double
            p = sr.Problem(g["X"], np.minimum(y, 11), 12)
        else:
            p = sr.Problem(g["X"], y, len(classes))
        st, _ = sr.newton_step(p, sr.initial_state(p))
        for _ in range(4):
            st.update(sr.cg_step(p, st)[0])
        out.append((p, st))
    return out


@pytest.mark.parametrize("drop", ["last_row", "last_chunk", "homogeneous"])
def test_mutations_of_the_hessian_product_break_both_assertions(mid_cg_states, drop):
    """A Hessian product that loses the last row, the last chunk or the homogeneous column moves the true-residual gap above
    1e-6 |G| (the GPU test holds 1e-11) and the stage error above 1e6 bounds (the GPU test holds 1)."""
    for p, st in mid_cg_states:
        assert p.chunks == 2 and st["live"].any()
        res, _ = sr.true_residual(p, st)
        gnorm = np.sqrt((st["G"] ** 2).sum(1))
        clean = (np.sqrt(((res - st["R"]) ** 2).sum(1)) / gnorm).max()
        HP, mag = sr.hessian_product(p, st, st["P"])
        p.drop = drop
        try:
            res_m, _ = sr.true_residual(p, st)
            HP_m, _ = sr.hessian_product(p, st, st["P"])
        finally:
            p.drop = None
        gap = (np.sqrt(((res_m - st["R"]) ** 2).sum(1)) / gnorm).max()
        stage = sr.nerr(HP_m, HP, sr.bound(p.L_xtu, mag)).max()
        print("n %d rows %d %s: clean gap %.3g |G|, mutated gap %.3g |G|, mutated stage error %.3g bounds" % (p.n, p.rows, drop, clean, gap, stage))
        assert clean < 1e-15 and gap > 1e-6 and stage > 1e6


def census(case, integer=False):
    """Every decision of the reference on the planted states of one case -> {decision: number inside its error bound}."""
    p = case.p
    inside = {}
    plant = sr.eval_plant(case, "all")
    out, mag, dec = sr.eval(p, plant, False)
    if integer:  # the margins are exact integers on both sides: the decision is exact, and some are exactly at the threshold
        M = out["M"]
        assert (M == np.round(M)).all() and mag["M"].max() < 2.0 ** 50 and (dec["act_margin"] == 0).sum() >= 10
        assert not dec["act"][dec["act_margin"] == 0].any()
    else:
        inside["act"] = int((dec["act_margin"] <= sr.bound(p.L_fwd, mag["M"])).sum())
    # the stop rule is decided on gn, a square root of a sum of D squares
    inside["stop"] = int((dec["stop_margin"] <= sr.bound(p.L_dot, out["gn"])).sum())
    assert dec["stop"].any() or case.rows < 3
    st = sr.cg_plant(case, out["M"])
    o2, m2, d2 = sr.cg_step(p, st)
    live = st["live"] != 0
    inside["php"] = int((d2["php_margin"] <= sr.bound(p.L_dot, m2["php"]))[live & (np.abs(st["P"]).sum(1) > 0)].sum())
    rnorm = np.sqrt((o2["R"] ** 2).sum(1))
    inside["cg_end"] = int((d2["cg_end_margin"] <= sr.bound(p.L_dot, rnorm))[live & d2["php_positive"]].sum())
    ev, _, _ = sr.eval(p, dict(W=case.W, notdone=np.ones(case.rows, dtype=np.int32)), True)
    ls, kind = sr.ls_plant(case, case.W, ev["G"].astype(np.float64), ev["M"].astype(np.float64))
    o3, m3, d3 = sr.line_search(p, ls)
    inside["descent"] = int((d3["descent_margin"] <= d3["descent_bound"])[kind != 9].sum())
    inside["armijo"] = int((d3["armijo_margin_over_bound"] <= 1)[kind != 9].sum())
    want_t = np.where(kind <= 6, 0.5 ** np.minimum(kind, 6), 0.0)
    assert np.array_equal(d3["t"].astype(np.float64), want_t), (d3["t"], kind)
    return inside


@pytest.mark.parametrize("case", sr.CASES, ids=sr.CASE_IDS)
def test_reference_excludes_no_decision_on_the_chosen_seeds(case):
    inside = census(sr.Case(*case))
    print(inside)
    assert all(v == 0 for v in inside.values()), inside


def test_reference_decisions_of_the_integer_case_are_exact():
    inside = census(sr.Case(257, 63, 65, integer=True), integer=True)
    assert all(v == 0 for v in inside.values()), inside
