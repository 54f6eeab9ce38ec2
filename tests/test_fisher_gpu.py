"""Fisher vectors on the device (csrc/fisher.hip) against the numpy reference of tests/fisher_oracle.py:
every entry point on its own, then ``gmm_fit`` and ``TrajectoryClassifier`` end to end.

Tolerances.  Both sides are float64; they differ in summation order and in the expanded form of the quadratic.  Every
compared quantity is scaled -- sums by the sum of the absolute values of the terms they accumulate, derived parameters by the
reference's own magnitude -- and ``hold`` asserts 16 x the largest scaled deviation recorded on an MI355X over the cases of
this file (``RECORDED``, the figure beside each name), and never more than 1e-9: anything larger in a float64 pipeline is a
bug, not rounding.  The float32 outputs (``pca_transform``, the Fisher vectors) are compared with the reference rounded to
float32, with 1 ulp allowed for the rounding of a float64 that differs in its last bits; what exceeds the ulp is scaled and
held like the rest."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 1e-9
# the largest scaled deviation from the reference over the cases of this file, recorded on an MI355X
RECORDED = {
    "moments": 1.26e-15,        # count, column sums, X^T X / sum |terms|
    "transform": 0.0,           # pca_transform beyond 1 ulp of float32 / sum |terms|
    "pca": 1.09e-13,            # mean, components, explained variance of pca_fit / the reference's largest magnitude
    "gamma": 1.40e-17,          # posteriors / the largest sum |terms| of the log-densities
    "stats": 3.61e-15,          # S0, S1, S2 / (sum gamma |x|^p) x the largest sum |terms| of the log-densities
    "loglik": 6.51e-18,         # sum logsumexp / sum |logsumexp|
    "mstep": 1.45e-16,          # weights, means, variances / the reference's largest magnitude
    "em": 3.38e-14,             # parameters and lower bounds of gmm_fit / the reference's largest magnitude
    "fisher": 0.0,              # Fisher vectors beyond 1 ulp of float32 (unit vectors: scale 1)
}
SEEN = {}


def hold(name, got, want, scale):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isfinite(got).all(), name
    diff = np.abs(got - want)
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), diff.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, diff / scale, np.where(diff > 0, np.inf, 0.0))
    dev = float(rel.max()) if rel.size else 0.0
    SEEN[name] = max(SEEN.get(name, 0.0), dev)
    print("DEV %s %.3e (largest so far %.3e)" % (name, dev, SEEN[name]))
    assert dev <= min(16.0 * RECORDED[name], CAP), (name, dev)


def hold32(name, got32, want64, scale):
    """float32 output against the float64 reference rounded to float32: 1 ulp is free, the rest is held like a float64"""
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32
    w32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    ulp = np.spacing(np.abs(w32)).astype(np.float64)
    excess = np.maximum(np.abs(got32.astype(np.float64) - w32.astype(np.float64)) - ulp, 0.0)
    hold(name, excess, np.zeros_like(excess), scale)


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def cpu(t):
    return t.cpu().numpy()


def device_stats(x, seg, w, mu, var, mode="soft", **kw):
    from video_analytics_amd import fisher
    st, ll = fisher.gmm_stats(dev(x), seg, w, mu, var, mode, **kw)
    return cpu(st), cpu(ll)


def hold_stats(x, seg, w, mu, var, got, mode="soft"):
    st, ll = got
    want, want_ll, scale = fo.stats(x, seg, w, mu, var, mode)
    amp = 1.0 if mode == "hard" else float(fo.log_prob_scale(x, w, mu, var).max())  # gamma's own error: that of its exponent
    hold("stats", st, want, scale * amp)
    hold("loglik", ll, want_ll, fo.loglik_scale(x, seg, w, mu, var) * float(fo.log_prob_scale(x, w, mu, var).max()))
    return want


# ---- PCA -------------------------------------------------------------------------------------------------------------------

def rows(n, d, seed):
    rng = np.random.RandomState(seed)
    return (rng.randn(n, d) * (0.5 + rng.rand(d)) + rng.randn(d)).astype(np.float32)


def hold_moments(got, x):
    for g, w, s in zip(got, fo.moments(x), fo.moments_scale(x)):
        if np.ndim(g) == 2:
            assert not np.tril(g, -1).any()  # below the diagonal: zeros
            w, s = np.triu(w), np.triu(s)
        hold("moments", g, w, s)


@pytest.mark.parametrize("n,d", [(1, 3), (15, 1), (16, 30), (17, 64), (63, 3), (64, 64), (65, 30), (1000, 64), (1000, 426), (3000, 30), (700, 129)])
def test_pca_moments(n, d):
    """one chunk (n <= 256), four with a ragged last one (n = 1000), twelve (n = 3000); one to seven tiles of 64 columns,
    with the ones column in a tile of its own (d = 64) and in the last ragged tile"""
    from video_analytics_amd import fisher
    x = rows(n, d, 10 * n + d)
    hold_moments(fisher.pca_moments(dev(x)), x)


def test_pca_moments_accumulate_over_a_list():
    from video_analytics_amd import fisher
    parts = [rows(n, 30, 40 + n) for n in (300, 1, 700)]
    x = np.concatenate(parts)
    got = fisher.pca_moments([dev(p) for p in parts] + [torch.empty((0, 30), dtype=torch.float32, device="cuda")])
    hold_moments(got, x)
    one = fisher.pca_moments(dev(x))
    for a, b, s in zip(got, one, fo.moments_scale(x)):
        hold("moments", a, b, np.triu(s) if np.ndim(s) == 2 else s)
    a, b = fisher.pca_fit([dev(p) for p in parts], 5), fisher.pca_fit(dev(x), 5)
    assert a.n_samples == b.n_samples == 1001
    for name in ("mean", "components", "explained_variance"):
        hold("pca", getattr(a, name), getattr(b, name), np.abs(getattr(b, name)).max())


def separated_rows(n, d, m, seed):
    """float32 rows whose sample covariance has the leading eigenvalues (8 x 0.95^j)^2, j = 0 .. m, by construction (orthonormal
    centred scores), and 1e-3 noise in the other directions"""
    rng = np.random.RandomState(seed)
    u = rng.randn(n, m + 1)
    u, _ = np.linalg.qr(u - u.mean(0))
    v, _ = np.linalg.qr(rng.randn(d, d))
    s = 8.0 * 0.95 ** np.arange(m + 1) * np.sqrt(n - 1.0)
    return ((u * s) @ v[:, :m + 1].T + 1e-3 * rng.randn(n, d) + rng.randn(d)).astype(np.float32)


@pytest.mark.parametrize("n,d,m", [(1000, 426, 64), (300, 30, 5)])
def test_pca_fit_and_transform(n, d, m, tmp_path):
    from video_analytics_amd import fisher
    x = separated_rows(n, d, m, 3)
    mean, comp, ev = fo.pca_fit(x, m)
    lead = np.linalg.eigvalsh(np.cov(x.astype(np.float64).T))[::-1][:m + 1]
    assert (lead[:-1] / lead[1:]).min() > 1.08  # separated eigenvalues: the eigenvectors are determined
    model = fisher.pca_fit(dev(x), m)
    assert model.n_samples == n and model.components.shape == (m, d)
    hold("pca", model.mean, mean, np.abs(mean).max())
    hold("pca", model.components, comp, np.abs(comp).max())
    hold("pca", model.explained_variance, ev, np.abs(ev).max())
    assert (np.abs(model.components).max(1) == model.components.max(1)).all()  # the sign convention
    for rows_ in (x, x[:1], x[:17], x[:65]):
        got = cpu(model.transform(dev(rows_)))
        hold32("transform", got, fo.pca_transform(rows_, model.mean, model.components),
               fo.pca_transform_scale(rows_, model.mean, model.components))
    model.save(str(tmp_path / "pca.npz"))
    back = fisher.PCAModel.load(str(tmp_path / "pca.npz"))
    assert np.array_equal(back.components, model.components) and np.array_equal(back.mean, model.mean) and back.n_samples == n
    assert torch.equal(back.transform(dev(x)), model.transform(dev(x)))
    with pytest.raises(ValueError, match="n_components"):
        fisher.pca_fit(dev(x[:4]), 4)
    with pytest.raises(ValueError, match="columns"):
        model.transform(dev(x[:, :d - 1]))


# ---- mixture statistics ------------------------------------------------------------------------------------------------------

RAGGED = np.concatenate([[0], np.cumsum((0, 1, 63, 65, 700, 0, 171))]).astype(np.int64)  # 7 segments, 1000 rows
STATS_CASES = (
    [(n, 3, 5, dict(chunk_rows=16), None) for n in (1, 15, 16, 17, 63, 64, 65)]
    + [(65, d, 16, dict(chunk_rows=16), None) for d in (1, 3, 30, 64)]
    + [(1000, 30, k, {}, None) for k in (1, 5, 16, 17, 64, 65, 200, 256)]
    + [(1000, 3, 5, kw, None) for kw in (dict(chunk_rows=1024), dict(chunk_rows=250), dict(chunk_rows=96), dict(chunk_rows=96, batch_rows=192),
                                         dict(chunk_rows=16, batch_rows=16))]
    + [(1000, 30, 17, kw, RAGGED) for kw in ({}, dict(chunk_rows=64), dict(chunk_rows=64, batch_rows=128), dict(chunk_rows=100, batch_rows=300))]
    + [(1000, 1, 5, dict(chunk_rows=64), RAGGED), (1000, 426, 1, dict(chunk_rows=256), RAGGED), (1000, 64, 256, dict(chunk_rows=128), RAGGED)]
)


def case_id(c):
    n, d, k, kw, seg = c
    return "n%d-d%d-k%d%s%s" % (n, d, k, "".join("-%s%d" % (a[:5], b) for a, b in sorted(kw.items())), "-ragged" if seg is not None else "")


@pytest.mark.parametrize("case", STATS_CASES, ids=[case_id(c) for c in STATS_CASES])
def test_gmm_stats_soft(case):
    from video_analytics_amd import fisher
    n, d, k, kw, seg = case
    seg = np.array([0, n]) if seg is None else seg
    x, w, mu, var = fo.mixture_rows(n, d, k, seed=n + 7 * d + 13 * k)
    hold_stats(x, seg, w, mu, var, device_stats(x, seg, w, mu, var, **kw))
    got = fisher.GMMModel(w, mu, var).posteriors(dev(x))
    hold("gamma", got, fo.posteriors(x, w, mu, var)[0], float(fo.log_prob_scale(x, w, mu, var).max()))
    assert np.abs(got.sum(1) - 1.0).max() < 1e-12


def test_gmm_stats_at_the_real_shape():
    x, w, mu, var = fo.mixture_rows(3000, 64, 256, seed=1)
    seg = np.array([0, 1100, 1100, 3000])
    hold_stats(x, seg, w, mu, var, device_stats(x, seg, w, mu, var))


@pytest.mark.parametrize("case", [c for c in STATS_CASES if c[0] >= 65], ids=[case_id(c) for c in STATS_CASES if c[0] >= 65])
def test_gmm_stats_hard_assignments_equal_the_reference(case):
    from video_analytics_amd import fisher
    n, d, k, kw, seg = case
    seg = np.array([0, n]) if seg is None else seg
    x, w, mu, var = fo.mixture_rows(n, d, k, seed=n + 7 * d + 13 * k)
    best, gap = fo.hard_assignments(x, w, mu, var)
    assert gap.min() > 1e-6  # no rounding can flip a row
    got = fisher.GMMModel(w, mu, var).posteriors(dev(x), mode="hard")
    assert np.array_equal(got, fo.one_hot(best, k))
    st, ll = device_stats(x, seg, w, mu, var, "hard", **kw)
    want = hold_stats(x, seg, w, mu, var, (st, ll), "hard")
    assert np.array_equal(st[:, :, 0], want[:, :, 0])  # counts: whole numbers, exact in any order


@pytest.mark.parametrize("k,dup", [(5, (1, 3)), (17, (0, 16)), (64, (20, 21)), (256, (100, 255))])
def test_hard_ties_go_to_the_lowest_component(k, dup):
    """two components with the same parameters: every row they win goes to the lower index, whether both sit in one lane's
    registers (16 apart), in neighbouring lanes, or anywhere"""
    from video_analytics_amd import fisher
    x, w, mu, var = fo.mixture_rows(500, 8, k, seed=k)
    lo, hi = dup
    mu[hi], var[hi] = mu[lo], var[lo]
    w[hi] = w[lo]
    w /= w.sum()
    got = fisher.GMMModel(w, mu, var).posteriors(dev(x), mode="hard")
    best = fo.hard_assignments(x, w, mu, var)[0]
    assert (best == lo).any() and not (best == hi).any()
    assert np.array_equal(got, fo.one_hot(best, k))
    # planted exact ties everywhere: all components equal, every row goes to component 0
    same = fisher.GMMModel(np.full(k, 1.0 / k), np.repeat(mu[:1], k, 0), np.repeat(var[:1], k, 0)).posteriors(dev(x), mode="hard")
    assert (same[:, 0] == 1).all() and same.sum() == len(x)


def test_chunk_lengths_agree_and_calls_repeat_to_the_bit():
    x, w, mu, var = fo.mixture_rows(1000, 30, 17, seed=4)
    scale = fo.stats(x, RAGGED, w, mu, var)[2] * float(fo.log_prob_scale(x, w, mu, var).max())
    base, base_ll = device_stats(x, RAGGED, w, mu, var)
    again, again_ll = device_stats(x, RAGGED, w, mu, var)
    assert np.array_equal(base, again) and np.array_equal(base_ll, again_ll)
    for kw in (dict(chunk_rows=64), dict(chunk_rows=100, batch_rows=300), dict(chunk_rows=16, batch_rows=32)):
        st, ll = device_stats(x, RAGGED, w, mu, var, **kw)
        st2, ll2 = device_stats(x, RAGGED, w, mu, var, **kw)
        assert np.array_equal(st, st2) and np.array_equal(ll, ll2)
        hold("stats", st, base, scale)
        hold("loglik", ll, base_ll, fo.loglik_scale(x, RAGGED, w, mu, var) * float(fo.log_prob_scale(x, w, mu, var).max()))
    # batches change where responsibilities are held, never the sums: same chunk length, same bits
    a = device_stats(x, RAGGED, w, mu, var, chunk_rows=64, batch_rows=64)
    b = device_stats(x, RAGGED, w, mu, var, chunk_rows=64, batch_rows=640)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_stats_argument_checks():
    from video_analytics_amd import fisher
    x, w, mu, var = fo.mixture_rows(40, 3, 2, seed=1)
    xd = dev(x)
    for kw, msg in ((dict(segments=[0, 39]), "segments must ascend"), (dict(segments=[1, 40]), "segments must ascend"),
                    (dict(segments=[0, 30, 20, 40]), "segments must ascend"), (dict(mode="fuzzy"), "mode"), (dict(chunk_rows=8), "chunk_rows"),
                    (dict(chunk_rows=64, batch_rows=32), "batch_rows"), (dict(means=mu[:1]), "means"), (dict(x=xd.double()), "float32"),
                    (dict(x=xd.cpu()), "CUDA")):
        args = dict(x=xd, segments=[0, 40], weights=w, means=mu, variances=var)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            fisher.gmm_stats(**args)
    with pytest.raises(ValueError, match="k out of range"):
        fisher.gmm_stats(dev(fo.mixture_rows(300, 2, 257, 1)[0]), [0, 300], *fo.mixture_rows(300, 2, 257, 1)[1:])
    with pytest.raises(ValueError, match="n_components = 50 exceeds"):
        fisher.gmm_fit(xd, 50)
    with pytest.raises(ValueError, match="init"):
        fisher.gmm_fit(xd, 2, init=(w, mu))
    with pytest.raises(ValueError, match="power"):
        fisher.fisher_vectors(xd, [0, 40], fisher.GMMModel(w, mu, var), power=2.0)
    with pytest.raises(ValueError, match="GMMModel"):
        fisher.fisher_vectors(xd, [0, 40], (w, mu, var))


# ---- M-step, EM ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d,k", [(65, 1, 1), (1000, 30, 17), (1000, 64, 256), (1000, 426, 1)])
def test_mstep_alone(n, d, k):
    from video_analytics_amd import fisher
    x, w, mu, var = fo.mixture_rows(n, d, k, seed=5)
    st = fo.stats(x, RAGGED if n == 1000 else [0, n], w, mu, var)[0]
    total = st[0].copy()
    for s in range(1, len(st)):
        total = total + st[s]  # the segments in ascending order
    for reg in (1e-6, 0.0):
        got = [cpu(t) for t in fisher.gmm_mstep(dev(st), reg)]
        for g, want in zip(got, fo.mstep(total, reg)):
            hold("mstep", g, want, np.abs(want).max())
        assert abs(got[0].sum() - 1.0) < 1e-14


def em_data():
    x, w0, mu0, var0 = fo.mixture_rows(1000, 7, 5, seed=3, spread=1.5)
    return x, w0, mu0, var0


@pytest.mark.parametrize("iters", (1, 5, 20))
def test_gmm_fit_from_given_parameters(iters):
    from video_analytics_amd import fisher
    x, w0, mu0, var0 = em_data()
    w, mu, var, history, _ = fo.em(x, w0, mu0, var0, iters, tol=0.0)
    m = fisher.gmm_fit(dev(x), 5, init=(w0, mu0, var0), max_iter=iters, tol=0.0, chunk_rows=128)
    assert m.n_iter == iters and not m.converged and len(m.history) == iters and m.lower_bound == m.history[-1]
    for got, want in ((m.weights, w), (m.means, mu), (m.variances, var), (m.history, history)):
        hold("em", got, want, np.abs(want).max())


def test_gmm_fit_from_a_seed_repeats_and_round_trips(tmp_path):
    from video_analytics_amd import fisher
    x = em_data()[0]
    kw = dict(seed=3, kmeans_iters=4, max_iter=5, tol=0.0)
    w0, mu0, var0 = fo.init(x, 5, seed=3, kmeans_iters=4)
    w, mu, var, history, _ = fo.em(x, w0, mu0, var0, 5, tol=0.0)
    a, b = fisher.gmm_fit(dev(x), 5, **kw), fisher.gmm_fit(dev(x), 5, **kw)
    for got, want in ((a.weights, w), (a.means, mu), (a.variances, var), (a.history, history)):
        hold("em", got, want, np.abs(want).max())
    assert np.array_equal(a.weights, b.weights) and np.array_equal(a.means, b.means) and np.array_equal(a.variances, b.variances)
    assert a.history == b.history  # EM parameters after 5 iterations: identical bits
    a.save(str(tmp_path / "gmm.npz"))
    back = fisher.GMMModel.load(str(tmp_path / "gmm.npz"))
    assert np.array_equal(back.means, a.means) and back.history == a.history and back.n_iter == 5 and back.converged == a.converged


def test_gmm_fit_recovers_a_planted_mixture():
    from video_analytics_amd import fisher
    rng = np.random.RandomState(101)
    planted = np.array([[0.0, 0.0, 0.0], [8.0, 0.0, 0.0], [0.0, 8.0, 8.0]])  # unit variances: at least 8 sigma apart
    z = rng.randint(0, 3, 2000)
    x = (planted[z] + rng.randn(2000, 3)).astype(np.float32)
    m = fisher.gmm_fit(dev(x), 3, seed=0)
    assert m.converged and m.n_iter < 100 and np.isfinite(m.history).all()
    order = [int(np.argmin(((m.means - p) ** 2).sum(1))) for p in planted]
    assert sorted(order) == [0, 1, 2]
    stderr = 1.0 / np.sqrt(np.bincount(z, minlength=3))
    assert (np.abs(m.means[order] - planted) <= 3.0 * stderr[:, None]).all()
    assert np.abs(m.weights[order] - np.bincount(z, minlength=3) / 2000.0).max() < 1e-3
    bad = x.copy()
    bad[5, 1] = np.nan
    with pytest.raises(RuntimeError, match="iteration 1"):
        fisher.gmm_fit(dev(bad), 3, seed=0)


# ---- Fisher vectors ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("power", (0.0, 0.5))
@pytest.mark.parametrize("d,k", [(1, 1), (3, 5), (30, 17), (64, 256)])
def test_fisher_encode_alone(d, k, power):
    """from the reference's statistics: the same formula on the same numbers, 1 ulp of float32"""
    from video_analytics_amd import fisher
    x, w, mu, var = fo.mixture_rows(1000, d, k, seed=6)
    st = fo.stats(x, RAGGED, w, mu, var)[0]
    counts = np.diff(RAGGED)
    got = cpu(fisher.fisher_encode(dev(st), counts, w, mu, var, power))
    want = np.stack([fo.fisher_from_stats(st[s], int(counts[s]), w, mu, var, power) for s in range(len(st))])
    assert got.shape == (7, k + 2 * k * d)
    hold32("fisher", got, want, 1.0)
    assert not got[0].any() and not got[5].any()  # T = 0
    if d > 1:
        assert np.abs(np.linalg.norm(got[[1, 2, 3, 4, 6]].astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_fisher_encode_stores_a_tiny_vector_as_it_is():
    from video_analytics_amd import fisher
    x, w, mu, var = fo.mixture_rows(100, 4, 3, seed=9)
    st = fo.stats(x, [0, 100], w, mu, var)[0]
    st[0, :, 0] = 100 * w * (1 + 1e-9)
    st[0, :, 1:5] = mu * st[0, :, :1]
    st[0, :, 5:] = (var + mu * mu) * st[0, :, :1]
    want = fo.fisher_from_stats(st[0], 100, w, mu, var)
    assert 0 < np.linalg.norm(want) < fo.EPSILON
    got = cpu(fisher.fisher_encode(dev(st), [100], w, mu, var))
    hold32("fisher", got[0], want, 1.0)
    one = fo.mstep(fo.stats_from_gamma(x, np.ones((100, 1)), [0, 100])[0], 0.0)  # a one-component fit of the same rows
    fv = cpu(fisher.fisher_vectors(dev(x), [0, 100], fisher.GMMModel(*one)))
    assert fv.shape == (1, 9) and np.abs(fv).max() < 1e-12  # all three blocks zero to rounding, and not normalised


@pytest.mark.parametrize("power", (0.0, 0.5))
@pytest.mark.parametrize("d,k,kw", [(3, 5, {}), (30, 17, dict(chunk_rows=64, batch_rows=128)), (64, 256, dict(chunk_rows=128))])
def test_fisher_vectors(d, k, kw, power):
    from video_analytics_amd import fisher
    x, w, mu, var = fo.mixture_rows(1000, d, k, seed=8)
    gmm = fisher.GMMModel(w, mu, var)
    got = fisher.fisher_vectors(dev(x), RAGGED, gmm, power, **kw)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (7, k + 2 * k * d)
    assert torch.equal(got, fisher.fisher_vectors(dev(x), RAGGED, gmm, power, **kw))  # identical bits
    want = fo.fisher_vectors(x, RAGGED, w, mu, var, power)
    hold32("fisher", cpu(got), want, 1.0)
    empty = fisher.fisher_vectors(torch.empty((0, d), dtype=torch.float32, device="cuda"), [0, 0, 0], gmm)
    assert tuple(empty.shape) == (2, k + 2 * k * d) and not empty.any()


# ---- the classifier ------------------------------------------------------------------------------------------------------------

def videos(n_videos, seed):
    """per-video descriptors [n_i, 30] of two planted classes whose rows come from different mixtures; video 1 is empty"""
    rng = np.random.RandomState(seed)
    base = np.random.RandomState(77)
    basis = base.randn(6, 30)
    centres = {0: base.randn(3, 6) * 4.0, 1: base.randn(3, 6) * 4.0}
    out, labels = [], []
    for v in range(n_videos):
        c = v % 2
        n = 0 if (v == 1 and seed == 0) else int(rng.randint(150, 250))
        z = rng.randint(0, 3, n)
        out.append(((centres[c][z] + rng.randn(n, 6)) @ basis + 0.05 * rng.randn(n, 30)).astype(np.float32))
        labels.append(10 + c)
    return out, np.array(labels)


def test_trajectory_classifier_end_to_end(tmp_path):
    from video_analytics_amd import fisher, trajectories
    train, y = videos(12, seed=0)
    held, y_held = videos(8, seed=1)
    clf = trajectories.TrajectoryClassifier().fit([dev(v) for v in train], y, n_components=6, n_gmm=4, power=0.5, max_iter=30)
    assert clf.gmm.means.shape == (4, 6) and clf.pca.components.shape == (6, 30) and clf.classes.tolist() == [10, 11]
    pred = clf.predict([dev(v) for v in held])
    assert pred.tolist() == y_held.tolist()  # held-out predictions all correct
    enc = clf.encode([dev(v) for v in train])
    assert tuple(enc.shape) == (12, 4 + 2 * 4 * 6) and not enc[1].any()  # the empty video: a zero vector
    seg = np.concatenate([[0], np.cumsum([len(v) for v in train])])
    reduced = fo.pca_transform(np.concatenate(train), clf.pca.mean, clf.pca.components).astype(np.float32)
    want = fo.fisher_vectors(reduced, seg, clf.gmm.weights, clf.gmm.means, clf.gmm.variances, 0.5)
    hold32("fisher", cpu(enc), want, 1.0)
    assert torch.equal(enc, fisher.fisher_vectors(dev(reduced), seg, clf.gmm, 0.5))
    clf.save(str(tmp_path / "model.npz"))
    back = trajectories.TrajectoryClassifier.load(str(tmp_path / "model.npz"))
    assert back.predict([dev(v) for v in held]).tolist() == pred.tolist()
    assert torch.equal(back.encode([dev(v) for v in held]), clf.encode([dev(v) for v in held]))
    with pytest.raises(ValueError, match="exceeds the 8192 columns"):
        trajectories.TrajectoryClassifier().fit([dev(v) for v in train], y)  # Sheet02's 64 x 256: 33,024 columns
    with pytest.raises(ValueError, match="12 videos but 3 labels"):
        trajectories.TrajectoryClassifier().fit([dev(v) for v in train], y[:3], 6, 4)


def test_encode_through_the_real_front_end():
    """dense_trajectories on the planted scene of tests/dtraj_scenes.py -> PCA, a small mixture, one Fisher vector"""
    import dtraj_scenes as scenes
    from video_analytics_amd import fisher, trajectories
    gray, flow, _ = scenes.planted()
    out = trajectories.dense_trajectories(dev(gray), dev(flow), length=6, nt=3, patch=16)
    desc = out["desc"]
    assert out["count"] >= 50 and desc.shape[1] == 2 * 6 + 33 * 12
    clf = trajectories.TrajectoryClassifier()
    clf.pca = fisher.pca_fit(desc, 8)
    clf.gmm = fisher.gmm_fit(clf.pca.transform(desc), 3, max_iter=10)
    fv = clf.encode([desc])
    assert tuple(fv.shape) == (1, 3 + 2 * 3 * 8) and bool(torch.isfinite(fv).all())
    assert abs(float(fv.double().norm()) - 1.0) < 1e-6
