"""The numpy restatement of the HMM chain (tests/hmm_oracle.py) against witnesses that share nothing with
it, and the host side of video_analytics_amd.hmm.  No test here needs a GPU.

Most cases here hold the restatement itself -- against scipy, the enumeration of all paths and ``logsumexp`` -- and import
nothing of the library: they validate the reference the GPU tests lean on, and pass wherever tests/hmm_oracle.py exists.
The cases that take the ``hmm`` fixture (compose, the M-step, rounds and jobs, the checks of ``fit``, ``mean_over_frames``,
``save`` / ``load``) and every case of tests/test_hmm_gpu.py are the ones that fail without the library's ``hmm`` module.

The emission bound.  With u = 2^-53, one term ((x - mu)(x - mu)) iv carries four roundings in the restatement (the
difference, the square, the product, and iv = 1 / var) and at most seven in scipy's route through sqrt(1 / var), so each
term is off by at most 4u and 7u of itself; adding D terms costs each side at most (D - 1) u of the sum of their magnitudes;
c_g adds D logarithms (1 ulp each and D roundings of the running sum) to D log 2 pi, which is at most (2D + 2) u of the sum
of the magnitudes of its parts on either side, and that sum is at most 2.2 |c_g| for variances in [0.5, 2], where
|log var| <= 0.7 against log 2 pi = 1.84.  Together the two sides differ by at most
    (11 + 2 (D - 1) + 2.2 (4 D + 4)) u (|c_g| + 1/2 sum_d |term_d|)  <=  (11 D + 18) u S,   S = |c_g| + 1/2 sum_d |term_d|,
and the test asserts exactly that, with nothing measured in it.

The Viterbi witness enumerates all N^T paths in long double; a case counts only when the witness's best path beats the
second best by a positive gap, which is asserted on every drawn input, so none is left out.  The score then matches to the
rounding of the T + (T - 1) + 1 = 2T adds along the best path: 2T u max(|partial sums|), and a partial sum is at most one
|logB| entry per frame -- bounded by the frame's largest finite one -- plus T + 1 model terms, each at most the largest
finite |log-probability| of the model."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as ho  # noqa: E402

NEG_INF = float("-inf")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def hmm():
    pytest.importorskip("torch")
    import __graft_entry__
    from video_analytics_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        __graft_entry__.build()
    from video_analytics_amd import hmm as module
    return module


# ---- emissions ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 3, 64, 65, 512])
def test_emissions_against_scipy_logpdf(d):
    from scipy.stats import multivariate_normal
    rng = np.random.RandomState(d)
    g, t = 4, 6
    means, variances, x = rng.randn(g, d), rng.uniform(0.5, 2.0, (g, d)), rng.randn(t, d) * 2.0
    got = ho.emissions(x, means, variances)
    for k in range(g):
        want = multivariate_normal.logpdf(x, mean=means[k], cov=np.diag(variances[k]))  # Sheet04.py:250
        terms = ((x - means[k]) ** 2) / variances[k]
        c = -0.5 * (d * np.log(2 * np.pi) + np.log(variances[k]).sum())
        scale = abs(c) + 0.5 * np.abs(terms).sum(axis=1)
        assert (np.abs(got[:, k] - np.atleast_1d(want)) <= (11 * d + 18) * U * scale).all(), (d, k)


def test_emissions_take_float32_rows_exactly():
    rng = np.random.RandomState(1)
    x32 = rng.randn(5, 7).astype(np.float32)
    means, variances = rng.randn(3, 7), rng.uniform(0.5, 2.0, (3, 7))
    assert np.array_equal(ho.emissions(x32, means, variances), ho.emissions(x32.astype(np.float64), means, variances))


# ---- Viterbi ------------------------------------------------------------------------------------------------------------------

def draw_model(rng, n, kind, g):
    emit = rng.randint(0, g, n)
    full = np.log(rng.uniform(0.05, 1.0, (n, n)))
    i = np.arange(n)
    if kind == "dense":
        la = full
    elif kind == "ltr":
        la = np.where((i[:, None] == i[None, :]) | (i[:, None] + 1 == i[None, :]), full, NEG_INF)
    else:  # dense with holes
        la = np.where(rng.uniform(size=(n, n)) < 0.6, full, NEG_INF)
    lpi, lf = np.log(rng.uniform(0.05, 1.0, n)), np.log(rng.uniform(0.05, 1.0, n))
    if kind == "holes":
        lpi[rng.randint(n)] = NEG_INF
        lf[rng.randint(n)] = NEG_INF
    if kind == "ltr":
        lpi[1:], lf[:-1] = NEG_INF, NEG_INF
    return emit, lpi, la, lf


def composed_model(rng):
    with np.errstate(divide="ignore"):
        units = [(0,) + ho.left_to_right(2, 0.6, 0.4), (2,) + ho.left_to_right(1, 0.7, 0.3)]
    emit, lpi, la, lf, _ = ho.compose(units)
    return emit, lpi, la, lf


VITERBI_CASES = [(n, t, kind) for n in (1, 2, 3) for t in (1, 2, 3, 5, 7) for kind in ("dense", "ltr", "holes")] + [(3, t, "composed") for t in (3, 4, 7)]


@pytest.mark.parametrize("n,t,kind", VITERBI_CASES)
def test_viterbi_against_the_enumeration_of_all_paths(n, t, kind):
    rng = np.random.RandomState(100 * n + 10 * t + len(kind))
    g = 4
    emit, lpi, la, lf = composed_model(rng) if kind == "composed" else draw_model(rng, n, kind, g)
    logb = rng.randn(t, g) * 2.0
    if kind == "holes":
        logb[rng.randint(t), rng.randint(g)] = NEG_INF
    want, wpath, gap = ho.brute_force(logb, emit, lpi, la, lf)
    score, path, status = ho.viterbi(logb, emit, lpi, la, lf)
    fast = ho.viterbi_fast(logb, emit, lpi, la, lf)
    assert fast[2] == status and np.array_equal(fast[1], path) and (fast[0] == score or status == 2)
    if wpath is None:
        assert status == 1 and score == NEG_INF and (path == -1).all()
        return
    assert gap > 0 or len(emit) ** t == 1, "the drawn case is a tie: draw another"  # the condition on the inputs; never skipped
    assert status == 0 and np.array_equal(path, wpath)
    finite = np.where(np.isfinite(logb), np.abs(logb), 0.0)
    params = np.concatenate([lpi, la.ravel(), lf])
    partial = finite.max(axis=1).sum() + (t + 1) * np.abs(params[np.isfinite(params)]).max()
    assert abs(np.longdouble(score) - want) <= 2 * t * U * partial


def test_viterbi_forced_ties_go_to_the_lowest_index():
    inf = NEG_INF
    # two predecessors of state 2 tie at frame 1 (0 + -1 and -1 + 0, exact in integers): the lower one, state 0, wins
    score, path, st = ho.viterbi(np.zeros((2, 3)), np.arange(3), np.array([0.0, -1.0, inf]),
                                 np.array([[inf, inf, -1.0], [inf, inf, 0.0], [inf, inf, inf]]), np.array([inf, inf, 0.0]))
    assert (score, list(path), st) == (-1.0, [0, 2], 0)
    # both final states tie, and every predecessor on the way: the lowest everywhere
    score, path, st = ho.viterbi(np.zeros((3, 2)), np.arange(2), np.zeros(2), np.full((2, 2), -1.0), np.full(2, -2.0))
    assert (score, list(path), st) == (-4.0, [0, 0, 0], 0)
    # states 1 and 2 tie for the final maximum above state 0: state 1
    score, path, st = ho.viterbi(np.zeros((1, 3)), np.arange(3), np.array([-3.0, -1.0, -1.0]), np.full((3, 3), inf), np.zeros(3))
    assert (score, list(path), st) == (-1.0, [1], 0)


def test_viterbi_status_of_nan_and_of_no_path():
    rng = np.random.RandomState(3)
    emit, lpi, la, lf = draw_model(rng, 3, "ltr", 4)
    logb = rng.randn(6, 4)
    assert ho.viterbi(logb[:2], emit, lpi, la, lf)[2] == 1  # two frames cannot cross three states
    bad = logb.copy()
    bad[3, emit[1]] = np.nan
    score, path, st = ho.viterbi(bad, emit, lpi, la, lf)
    assert st == 2 and np.isnan(score) and (path == -1).all()


# ---- forward-backward ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,t,kind", [(n, t, kind) for n in (1, 2, 3) for t in (1, 2, 4, 7) for kind in ("dense", "ltr", "holes")])
def test_forward_backward_against_the_enumeration(n, t, kind):
    rng = np.random.RandomState(7 * n + 31 * t + len(kind))
    g = 4
    emit, lpi, la, lf = draw_model(rng, n, kind, g)
    logb = rng.randn(t, g) * 2.0
    best, wpath, _ = ho.brute_force(logb, emit, lpi, la, lf)
    gm, xi, ll, st = ho.forward_backward(logb, emit, lpi, la, lf)
    if wpath is None:
        assert st == 1 and ll == NEG_INF and not gm.any() and not xi.any()
        return
    G, X, L = ho.brute_force_posteriors(logb, emit, lpi, la, lf)
    # gamma and xi lie in [0, 1]; every entry is a ratio of sums of at most N^T products of 2T factors
    tol = 64 * t * n * U
    assert st == 0 and np.abs(gm - G).max() <= tol and np.abs(xi - X).max() <= tol * t
    assert abs(ll - L) <= 64 * t * U * (np.abs(logb).sum() + 10.0 * t)
    assert np.allclose(gm.sum(axis=1), 1.0, atol=tol, rtol=0)


def log_domain_forward_backward(logb, emit, log_pi, log_a, log_final):
    """The textbook log-domain recursions with scipy's logsumexp: (gamma, xi_sum, loglik)."""
    from scipy.special import logsumexp
    T, n = logb.shape[0], len(emit)
    lb = logb[:, emit]
    la, lbeta = np.empty((T, n)), np.empty((T, n))
    la[0] = log_pi + lb[0]
    for t in range(1, T):
        la[t] = logsumexp(la[t - 1][:, None] + log_a, axis=0) + lb[t]
    lbeta[T - 1] = log_final
    for t in range(T - 2, -1, -1):
        lbeta[t] = logsumexp(log_a + (lb[t + 1] + lbeta[t + 1])[None, :], axis=1)
    ll = logsumexp(la[T - 1] + log_final)
    xi = np.zeros((n, n))
    for t in range(T - 1):
        xi += np.exp(la[t][:, None] + log_a + (lb[t + 1] + lbeta[t + 1])[None, :] - ll)
    return np.exp(la + lbeta - ll), xi, ll


def test_forward_backward_against_the_log_domain_at_200_frames():
    rng = np.random.RandomState(9)
    t, g = 200, 6
    for kind, n in (("dense", 5), ("ltr", 8), ("holes", 6)):
        emit, lpi, la, lf = draw_model(rng, n, kind, g)
        logb = rng.randn(t, g) * 3.0 - 40.0  # far below what an unscaled product of 200 factors could hold
        gm, xi, ll, st = ho.forward_backward(logb, emit, lpi, la, lf)
        with np.errstate(divide="ignore", invalid="ignore"):
            G, X, L = log_domain_forward_backward(logb, emit, lpi, la, lf)
        if not np.isfinite(L):
            assert st == 1
            continue
        # the log-domain side exponentiates sums near |loglik| ~ 10^4: its own rounding is |loglik| u, relative, per entry
        tol = 16 * abs(L) * U
        assert st == 0 and np.abs(gm - G).max() <= tol and np.abs(xi - X).max() <= tol * t and abs(ll - L) <= tol


def test_forward_backward_status():
    rng = np.random.RandomState(10)
    emit, lpi, la, lf = draw_model(rng, 3, "dense", 4)
    logb = rng.randn(5, 4)
    dead = logb.copy()
    dead[2, :] = NEG_INF
    gm, xi, ll, st = ho.forward_backward(dead, emit, lpi, la, lf)
    assert st == 1 and ll == NEG_INF and not gm.any() and not xi.any()
    nan = logb.copy()
    nan[1, emit[0]] = np.nan
    assert ho.forward_backward(nan, emit, lpi, la, lf)[3] == 2


# ---- compose ------------------------------------------------------------------------------------------------------------------

def test_compose_against_matrices_written_by_hand(hmm):
    inf = NEG_INF
    s, x, e = np.log(0.9), np.log(0.1), np.log(0.1)
    hs = hmm.HmmSet(np.zeros((5, 1)), np.ones((5, 1)))
    hs.add_unit(hmm.HmmSet.left_to_right("a", 0, 2))
    hs.add_unit(hmm.HmmSet.left_to_right("b", 2, 1))
    hs.add_unit(hmm.HmmSet.left_to_right("c", 3, 2))
    two = np.array([[s, x, inf], [inf, s, e + 0.0], [inf, inf, s]])
    three = np.array([[s, e + 0.0, inf, inf, inf], [inf, s, x, inf, inf], [inf, inf, s, e + 0.0, inf], [inf, inf, inf, s, x],
                      [inf, inf, inf, inf, s]])
    for names, dense, emit, pi, fin in ((["a", "b"], two, [0, 1, 2], [0.0, inf, inf], [inf, inf, e]),
                                        (["b", "c", "a"], three, [2, 3, 4, 0, 1], [0.0, inf, inf, inf, inf], [inf, inf, inf, inf, e])):
        m = hs.compose(names)
        want = hmm.Model.from_dense(dense, pi, fin, emit)
        for f in ("emit", "pred_ptr", "pred_idx", "pred_logp", "log_pi", "log_final"):
            assert np.array_equal(getattr(m, f), getattr(want, f)), (names, f)
        units = [(hs.units[hs.unit_index(nm)].first,) + ho.left_to_right(hs.units[hs.unit_index(nm)].n_states) for nm in names]
        o = ho.compose(units)
        assert np.array_equal(o[0], emit) and np.array_equal(o[2], dense) and np.array_equal(o[1], pi) and np.array_equal(o[3], fin)
        assert np.array_equal(m.unit_of_state, o[4])
    # a general topology: two ways in, two ways out
    hs.add_unit(hmm.HmmSet.unit_from_dense("d", 0, [[0.5, 0.25], [0.0, 0.5]], [0.5, 0.5], [0.25, 0.5]))
    m = hs.compose(["d", "d"])
    l5, l25 = np.log(0.5), np.log(0.25)
    dense = np.array([[l5, l25, l25 + l5, l25 + l5], [inf, l5, l5 + l5, l5 + l5], [inf, inf, l5, l25], [inf, inf, inf, l5]])
    want = hmm.Model.from_dense(dense, [l5, l5, inf, inf], [inf, inf, l25, l5], [0, 1, 0, 1])
    for f in ("emit", "pred_ptr", "pred_idx", "pred_logp", "log_pi", "log_final"):
        assert np.array_equal(getattr(m, f), getattr(want, f)), f
    sp, si, se = hmm.successor_lists(m)
    assert list(sp) == [0, 4, 7, 9, 10] and list(si) == [0, 1, 2, 3, 1, 2, 3, 2, 3, 3]
    assert all(m.pred_idx[e] == i for i in range(4) for e in se[sp[i]:sp[i + 1]])
    with pytest.raises(ValueError, match="no unit named"):
        hs.compose(["a", "z"])
    with pytest.raises(ValueError, match="at most 1024"):
        hs.compose(["a"] * 513)


# ---- the M-step and fit ---------------------------------------------------------------------------------------------------------

def planted_sequences(seed, n_seq=6, d=2, spread=6.0):
    rng = np.random.RandomState(seed)
    centres = {0: np.array([[0.0, 0.0], [spread, spread], [2 * spread, 0.0]]), 1: np.array([[0.0, 2 * spread], [-spread, spread]])}
    seqs, unit_of = [], []
    for i in range(n_seq):
        u = i % 2
        runs = [int(rng.randint(5, 9)) for _ in centres[u]]
        seqs.append(np.concatenate([c + rng.randn(r, d) for c, r in zip(centres[u], runs)]))
        unit_of.append(u)
    return seqs, unit_of, centres


def test_baum_welch_never_lowers_the_likelihood_and_recovers_planted_means():
    seqs, unit_of, centres = planted_sequences(21)
    means, variances, units, lls = ho.fit(seqs, unit_of, [3, 2], 6, "baum-welch", var_floor=0.0)
    # EM's guarantee holds for the exact M-step, which var_floor = 0 is; the slack is the rounding of a sum of ~100 terms
    for a, b in zip(lls[:-1], lls[1:]):
        assert b >= a - 1e-9 * abs(a), lls
    assert lls[-1] > lls[0]
    want = np.concatenate([centres[0], centres[1]])
    assert np.abs(means - want).max() < 1.0  # within the noise of ~20 unit-variance frames per state (sigma / sqrt(20) = 0.22)
    for pi, a, ex in units:
        rows = np.exp(a).sum(axis=1) + np.exp(ex)
        assert np.allclose(rows, 1.0, atol=1e-12) and np.isclose(np.exp(pi).sum(), 1.0)


def test_viterbi_training_against_a_literal_loop():
    seqs, unit_of, _ = planted_sequences(22, n_seq=4)
    means, variances, units, lls = ho.fit(seqs, unit_of, [3, 2], 1, "viterbi")
    # one iteration by hand: uniform split -> Gaussians -> decode -> means of the decoded frames
    firsts = [0, 3]
    x = np.concatenate(seqs)
    seg = np.concatenate([[0], np.cumsum([len(q) for q in seqs])])
    lab = np.concatenate([firsts[unit_of[i]] + (np.arange(len(q)) * [3, 2][unit_of[i]]) // len(q) for i, q in enumerate(seqs)])
    m0 = np.array([x[lab == g].mean(axis=0) for g in range(5)])
    v0 = np.array([(x[lab == g] ** 2).mean(axis=0) - m0[g] ** 2 + 1e-6 for g in range(5)])
    logb = ho.emissions(x, m0, v0)
    lab1, total = np.empty(len(x), dtype=int), 0.0
    for i in range(len(seqs)):
        emit = firsts[unit_of[i]] + np.arange([3, 2][unit_of[i]])
        score, path, st = ho.viterbi(logb[seg[i]:seg[i + 1]], emit, *ho.left_to_right(len(emit)))
        assert st == 0
        lab1[seg[i]:seg[i + 1]] = emit[path]
        total += score
    m1 = np.array([x[lab1 == g].mean(axis=0) for g in range(5)])
    assert np.allclose(means, m1, rtol=0, atol=1e-12) and np.isclose(lls[0], total, rtol=1e-14)


def test_a_starved_state_keeps_its_parameters(hmm):
    stats = np.array([[10.0, 20.0, 50.0], [1e-4, 5.0, 9.0], [0.0, 0.0, 0.0], [np.nan, 1.0, 1.0]])
    means, variances = np.full((4, 1), 7.0), np.full((4, 1), 3.0)
    for fn in (hmm.mstep_gaussians, ho.mstep_gaussians):
        m, v = fn(stats, means, variances, 0.5, 1e-3)
        assert m[0, 0] == 2.0 and v[0, 0] == 5.0 - 4.0 + 0.5
        assert (m[1:] == 7.0).all() and (v[1:] == 3.0).all()
    # transitions: a row without statistics is kept, the others sum to one with their exit, absent edges stay absent
    u = hmm.HmmSet.left_to_right("a", 0, 3)
    xi = np.array([[6.0, 2.0, 9.0], [0.0, 0.0, 0.0], [0.0, 0.0, 3.0]])
    new = hmm.mstep_unit(u, xi, np.array([4.0, 1.0, 0.0]), np.array([5.0, 0.0, 1.0]))
    o = ho.mstep_unit(u.log_pi, u.log_a, u.exit_logp, xi, np.array([4.0, 1.0, 0.0]), np.array([5.0, 0.0, 1.0]))
    for got, want in zip((new.log_pi, new.log_a, new.exit_logp), o):
        assert np.array_equal(got, want)
    assert np.array_equal(np.exp(new.log_a[0]), [0.75, 0.25, 0.0]) and np.array_equal(new.log_a[1], u.log_a[1])
    assert np.array_equal(np.exp(new.log_a[2]), [0.0, 0.0, 0.75]) and np.exp(new.exit_logp[2]) == 0.25 and new.log_pi[0] == 0.0


# ---- the rest of the host side ----------------------------------------------------------------------------------------------------

def test_mean_over_frames(hmm):
    for fn in (hmm.mean_over_frames, ho.mean_over_frames):
        assert fn([1, 1, 2, 3], [1, 2, 2, 3]) == 0.75
    assert hmm.mean_over_frames([np.array([1, 1]), np.array([2, 3, 4, 5])], [np.array([1, 0]), np.array([2, 3, 4, 0])]) == 4.0 / 6.0
    with pytest.raises(ValueError, match="equal"):
        hmm.mean_over_frames([1, 2], [1])
    assert hmm.boundaries([4, 4, 2, 2, 2, 4]) == [(0, 2, 4), (2, 5, 2), (5, 6, 4)]
    assert list(hmm.best_grammar(np.array([[1.0, 1.0], [np.nan, -5.0], [NEG_INF, NEG_INF]]))) == [0, 1, 0]
    assert list(hmm.uniform_alignment(7, 3)) == [0, 0, 0, 1, 1, 2, 2]


def test_rounds_and_jobs(hmm):
    need = np.array([40, 10, 50, 60, 5])
    assert hmm.plan_rounds(need, [1, 1, 1, 1, 1], 100, "viterbi", need, need) == [(0, 3), (3, 5)]
    assert hmm.plan_rounds(need, [1, 0, 1, 0, 1], 100, "viterbi", need, need) == [(0, 5)]
    with pytest.raises(ValueError, match="job 3 alone"):
        hmm.plan_rounds(need, [1, 1, 1, 1, 1], 59, "viterbi", need, need)
    assert hmm.check_jobs(None, 2, 2).tolist() == [[0, 0, 1], [0, 1, 1], [1, 0, 1], [1, 1, 1]]
    for bad, msg in (([(2, 0, 1)], "sequence"), ([(0, 2, 1)], "model"), ([(0, 0, 3)], "want_path"), ([[0.5, 0, 1]], "integers")):
        with pytest.raises(ValueError, match=msg):
            hmm.check_jobs(bad, 2, 2)


def test_fit_argument_checks(hmm):
    ok = dict(n_seqs=2, unit_of_sequence=["a", "b"], n_states=3, init_alignments=None, lengths=[4, 5], iters=2, method="baum-welch",
              var_floor=1e-6, min_occupancy=1e-3, self_prob=0.9, next_prob=0.1)
    assert hmm.check_fit_args(**ok) == (["a", "b"], [3, 3])
    assert hmm.check_fit_args(**dict(ok, n_states={"a": 2, "b": 4}))[1] == [2, 4]
    for over, msg in ((dict(unit_of_sequence=["a"]), "unit_of_sequence"), (dict(n_states=0), "n_states"), (dict(n_states={"a": 2}), "lacks"),
                      (dict(iters=-1), "iters"), (dict(method="em"), "method"), (dict(var_floor=-1.0), "var_floor"),
                      (dict(min_occupancy=float("nan")), "min_occupancy"), (dict(self_prob=0.0), "self_prob"), (dict(next_prob=1.5), "next_prob"),
                      (dict(init_alignments=[[0, 1, 2, 2]]), "init_alignments"), (dict(init_alignments=[[0, 1, 2, 3], [0] * 5]), "init_alignments")):
        with pytest.raises(ValueError, match=msg):
            hmm.check_fit_args(**dict(ok, **over))


def test_save_and_load_round_trip_the_bits(hmm, tmp_path):
    rng = np.random.RandomState(30)
    hs = hmm.HmmSet(rng.randn(5, 3), rng.uniform(0.5, 2.0, (5, 3)))
    hs.add_unit(hmm.HmmSet.left_to_right("pour", 0, 3, 0.8, 0.2))
    hs.add_unit(hmm.HmmSet.unit_from_dense("stir", 3, [[0.5, 0.25], [0.0, 0.5]], [0.5, 0.5], [0.25, 0.5]))
    hs.save(str(tmp_path / "set.npz"))
    back = hmm.HmmSet.load(str(tmp_path / "set.npz"))
    assert back.names == hs.names and np.array_equal(back.means, hs.means) and np.array_equal(back.variances, hs.variances)
    for a, b in zip(hs.units, back.units):
        assert a.first == b.first and all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("log_pi", "log_a", "exit_logp"))
    seg = hmm.HmmSegmenter()
    with pytest.raises(ValueError, match="not fitted"):
        seg.save(str(tmp_path / "m.npz"))
    seg.hmmset, seg.logliks, seg.grammars = hs, [-3.5, -2.25], [["pour", "stir"], ["stir"]]
    seg.save(str(tmp_path / "m.npz"))
    m = hmm.HmmSegmenter.load(str(tmp_path / "m.npz"))
    assert m.grammars == seg.grammars and m.logliks == seg.logliks and np.array_equal(m.hmmset.means, hs.means)
    assert np.array_equal(m.hmmset.compose(["pour", "stir"]).pred_logp, hs.compose(["pour", "stir"]).pred_logp)
