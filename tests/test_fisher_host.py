"""Fisher vectors, the host side: the numpy reference of tests/fisher_oracle.py against scikit-learn and
against a literal restatement, the analytic properties of the Fisher vector, and the host-only entry points of the library.
No GPU is needed; tests/test_fisher_gpu.py holds the kernels to the same reference."""
import ctypes
import importlib
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_oracle as fo  # noqa: E402
from video_analytics_amd import fisher as _feature  # noqa: E402,F401  the feature under test: without it no test here passes


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    from video_analytics_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        __graft_entry__.build()
    return _ffi.lib()


@pytest.mark.parametrize("iters", (1, 5, 20))
def test_reference_em_agrees_with_sklearn(iters):
    """GaussianMixture(diag) from the same initial parameters, tol = 0: measured 8e-14 on the parameters and 2e-15 on the
    lower bound at this shape; asserted at 1e-11 because BLAS summation order differs between machines."""
    from sklearn.mixture import GaussianMixture
    x, w0, mu0, var0 = fo.mixture_rows(1000, 7, 5, seed=3, spread=1.5)
    x = x.astype(np.float64)
    gm = GaussianMixture(5, covariance_type="diag", weights_init=w0, means_init=mu0, precisions_init=1.0 / var0, max_iter=iters, tol=0.0,
                         reg_covar=1e-6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm.fit(x)
    w, mu, var, history, converged = fo.em(x, w0, mu0, var0, iters, tol=0.0, reg_covar=1e-6)
    dev = [np.abs(w - gm.weights_).max(), np.abs(mu - gm.means_).max(), np.abs(var - gm.covariances_).max(), abs(history[-1] - gm.lower_bound_)]
    print("iters %d: weights %.3g means %.3g covariances %.3g lower bound %.3g" % (iters, *dev))
    assert len(history) == iters and not converged
    assert max(dev) <= 1e-11, dev


def test_reference_pca_agrees_with_sklearn():
    """PCA(svd_solver='full') on data whose leading eigenvalues are well separated (asserted first: a near-tie makes the
    eigenvectors arbitrary).  Measured 8e-16 on the components and 1.4e-14 on explained_variance_; asserted at 1e-11."""
    from sklearn.decomposition import PCA
    rng = np.random.RandomState(0)
    d, m = 12, 5
    q, _ = np.linalg.qr(rng.randn(d, d))
    scales = np.array([9.0, 6.0, 4.0, 2.5, 1.5] + [0.3] * (d - 5))
    x = ((rng.randn(600, d) * scales) @ q.T + rng.randn(d)).astype(np.float32)
    ref = PCA(n_components=m, svd_solver="full").fit(x.astype(np.float64))
    lead = np.linalg.eigvalsh(np.cov(x.astype(np.float64).T))[::-1][:m + 1]
    assert (lead[:-1] / lead[1:]).min() > 1.3, lead
    mean, comp, ev = fo.pca_fit(x, m)
    dev = [np.abs(mean - ref.mean_).max(), np.abs(comp - ref.components_).max(), np.abs(ev - ref.explained_variance_).max()]
    print("mean %.3g components %.3g explained variance %.3g" % tuple(dev))
    assert max(dev) <= 1e-11, dev
    z = fo.pca_transform(x, mean, comp)
    assert np.abs(z - ref.transform(x.astype(np.float64))).max() <= 1e-11


def literal_fisher_vector(x, w, mu, var, power=0.0):
    """The Fisher vector of one video as the modelled project states it, component by component, with gamma the posterior."""
    x = np.asarray(x, dtype=np.float64)
    T, K = len(x), len(w)
    sigma = np.sqrt(var)
    gamma = fo.posteriors(x, w, mu, var)[0]
    alpha = [np.sum(gamma[:, k] - w[k]) / np.sqrt(w[k]) for k in range(K)]
    g_mu, g_sigma = [], []
    for k in range(K):
        u = (x - mu[k]) / sigma[k]
        g_mu.append(np.sum(gamma[:, k][:, None] * u, axis=0) / np.sqrt(w[k]))
        g_sigma.append(np.sum(gamma[:, k][:, None] * (u * u - 1.0) / np.sqrt(2.0), axis=0) / np.sqrt(w[k]))
    v = np.concatenate([np.array(alpha), np.ravel(np.array(g_mu)), np.ravel(np.array(g_sigma))]) / T
    if power > 0:
        v = np.sign(v) * np.abs(v) ** power
    norm = np.linalg.norm(v)
    return v if norm < fo.EPSILON else v / norm


@pytest.mark.parametrize("power", (0.0, 0.5))
def test_reference_fisher_vector_equals_the_literal_restatement(power):
    """Both float64; the statistics form cancels S2 - 2 mu S1 + mu^2 S0 where the literal form squares (x - mu) / sigma, an
    amplification of about max x^2 / var < 1e3 of 200 roundings of 1.1e-16: 1e-11 on a unit vector."""
    x, w, mu, var = fo.mixture_rows(200, 6, 4, seed=5)
    got = fo.fisher_vectors(x, [0, 200], w, mu, var, power)[0]
    want = literal_fisher_vector(x, w, mu, var, power)
    assert got.shape == (4 + 2 * 4 * 6,)
    assert np.abs(got - want).max() <= 1e-11


def test_fisher_vector_of_a_one_component_fit_is_zero():
    x = fo.mixture_rows(300, 5, 3, seed=7)[0]
    w, mu, var = fo.mstep(fo.stats_from_gamma(x, np.ones((300, 1)), [0, 300])[0], reg_covar=0.0)
    fv = fo.fisher_vectors(x, [0, 300], w, mu, var)[0]
    assert fv.shape == (1 + 2 * 5,) and np.abs(fv).max() < 1e-12  # below EPSILON: stored as it is, not blown up to norm 1


def test_fisher_vector_norm_power_and_empty_segment():
    x, w, mu, var = fo.mixture_rows(150, 4, 3, seed=9)
    seg = [0, 0, 100, 100, 150]
    fv = fo.fisher_vectors(x, seg, w, mu, var)
    assert fv.shape == (4, 3 + 2 * 3 * 4)
    assert not fv[0].any() and not fv[2].any()  # T = 0
    assert np.allclose(np.linalg.norm(fv[[1, 3]], axis=1), 1.0, rtol=0, atol=1e-14)
    st = fo.stats(x, seg, w, mu, var)[0]
    raw = fo.fisher_from_stats(st[1], 100, w, mu, var, 0.0)
    half = fo.fisher_from_stats(st[1], 100, w, mu, var, 0.5)
    root = np.sign(raw) * np.sqrt(np.abs(raw))  # raw is v / |v|: the signed root of v, normalised, is root / |root|
    assert np.abs(half - root / np.linalg.norm(root)).max() <= 1e-14
    # the EPSILON branch: a vector whose norm is below 1e-6 is returned as it is
    tiny = st[1].copy()
    tiny[:, 0] = 100 * w * (1 + 1e-9)
    tiny[:, 1:5] = mu * tiny[:, :1]
    tiny[:, 5:] = (var + mu * mu) * tiny[:, :1]
    v = fo.fisher_from_stats(tiny, 100, w, mu, var, 0.0)
    assert 0 < np.linalg.norm(v) < fo.EPSILON


def test_hard_assignments_take_the_lowest_component_on_ties():
    x, w, mu, var = fo.mixture_rows(50, 3, 4, seed=11)
    mu[2], var[2], w[2] = mu[0], var[0], w[0]
    best, gap = fo.hard_assignments(x, w, mu, var)
    assert 2 not in best and (gap[best == 0] == 0).all() and (best == 0).any()


# ---- the library's host-only entry points ----------------------------------------------------------------------------------

def test_gmm_workspace_bytes_names_the_field_out_of_range(lib):
    from video_analytics_amd import _ffi

    def need(n=1000, d=64, k=256, ns=1, **over):
        p = _ffi.GmmParams()
        lib.va_gmm_default_params(ctypes.byref(p))
        for key, v in over.items():
            setattr(p, key, v)
        return lib.va_gmm_workspace_bytes(n, d, k, ns, ctypes.byref(p))

    bad = [(dict(n=0), "n out of range"), (dict(d=0), "d out of range"), (dict(d=513), "d out of range"), (dict(k=0), "k out of range"),
           (dict(k=257), "k out of range"), (dict(ns=0), "n_segments out of range"), (dict(ns=65537), "n_segments out of range"),
           (dict(chunk_rows=15), "chunk_rows out of range"), (dict(chunk_rows=65537, batch_rows=65537), "chunk_rows out of range"),
           (dict(chunk_rows=64, batch_rows=63), "batch_rows out of range"), (dict(batch_rows=65537), "batch_rows out of range"),
           (dict(struct_bytes=4), "struct_bytes")]
    for kw, msg in bad:
        assert need(**kw) == 0, kw
        assert msg in lib.va_last_error().decode(), (kw, lib.va_last_error())
    for kw in (dict(n=1), dict(d=1), dict(d=512), dict(k=1), dict(k=256), dict(ns=65536, k=1, d=1), dict(chunk_rows=16), dict(chunk_rows=65536),
               dict(chunk_rows=64, batch_rows=64), dict(batch_rows=65536), dict(d=64, k=256), dict(d=426, k=1)):
        assert need(**kw) > 0, kw
    assert lib.va_gmm_workspace_bytes(1000, 64, 256, 1, None) == need()  # NULL: the defaults
    with pytest.raises(ValueError, match="chunk_rows"):
        _ffi.default_gmm_params(chunk_rows=8)
    with pytest.raises(ValueError, match="unknown GMM parameter"):
        _ffi.default_gmm_params(chunks=8)
    p = _ffi.default_gmm_params()
    assert (p.chunk_rows, p.batch_rows, p.struct_bytes) == (1024, 65536, ctypes.sizeof(_ffi.GmmParams))


def test_gmm_workspace_does_not_grow_with_the_rows(lib):
    a = lib.va_gmm_workspace_bytes(10 ** 6, 64, 256, 1, None)
    b = lib.va_gmm_workspace_bytes(2 ** 31 - 1, 64, 256, 1, None)
    assert a == b and 0 < a < (1 << 30), (a, b)
    assert lib.va_gmm_workspace_bytes(70000, 64, 256, 1, None) == a  # one batch of responsibilities, whatever n


def test_pca_workspace_bytes_and_chunks(lib):
    for n, d in ((0, 8), (8, 0), (8, 2049)):
        assert lib.va_pca_workspace_bytes(n, d) == 0 and lib.va_pca_chunk_rows(n, d) == 0
        assert b"1 <= d <= 2048" in lib.va_last_error()
    for n, d in ((1, 1), (1000, 426), (10 ** 6, 426), (2 ** 31 - 1, 426), (2 ** 31 - 1, 2048), (5000, 2048)):
        rows, need = lib.va_pca_chunk_rows(n, d), lib.va_pca_workspace_bytes(n, d)
        chunks = -(-n // rows)
        assert rows >= 256 and rows % 4 == 0 and 1 <= chunks <= 64 and need == chunks * (d + 1) ** 2 * 8 and need <= (1 << 30), (n, d)
    assert lib.va_pca_chunk_rows(1000, 426) == 256 and lib.va_pca_chunk_rows(3000, 64) == 256


def test_fisher_never_imports_sklearn(monkeypatch):
    monkeypatch.setitem(sys.modules, "sklearn", None)  # any ``import sklearn`` now raises ImportError
    for name in ("video_analytics_amd.fisher", "video_analytics_amd.trajectories"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    fisher = importlib.import_module("video_analytics_amd.fisher")
    traj = importlib.import_module("video_analytics_amd.trajectories")
    assert hasattr(fisher, "gmm_fit") and hasattr(traj, "TrajectoryClassifier")
    src = open(fisher.__file__).read() + open(traj.__file__).read() + open(os.path.join(os.path.dirname(fisher.__file__), "_features.py")).read()
    assert "import sklearn" not in src and "from sklearn" not in src


def test_host_side_argument_checks_name_the_argument():
    import torch
    from video_analytics_amd import fisher, trajectories
    with pytest.raises(ValueError, match="x must be a CUDA tensor"):
        fisher.gmm_fit(torch.zeros(10, 3), 2)
    with pytest.raises(ValueError, match="descs must be a CUDA tensor"):
        fisher.pca_fit(torch.zeros(10, 3), 2)
    for kw, name in ((dict(n_components=0), "n_components"), (dict(n_components=257), "n_components"), (dict(tol=-1.0), "tol"),
                     (dict(tol=float("nan")), "tol"), (dict(max_iter=0), "max_iter"), (dict(reg_covar=-1e-6), "reg_covar"),
                     (dict(seed=-1), "seed"), (dict(kmeans_iters=-1), "kmeans_iters"), (dict(max_iter=2.5), "max_iter")):
        args = dict(n_components=4, tol=1e-3, max_iter=10, reg_covar=1e-6, seed=0, kmeans_iters=3)
        args.update(kw)
        with pytest.raises(ValueError, match="gmm_fit: %s" % name):
            fisher.check_gmm_fit_args(**args)
    with pytest.raises(ValueError, match="n_components = 5 exceeds"):
        fisher.pca_from_moments(5.0, np.zeros(8), np.eye(8), 5)
    with pytest.raises(ValueError, match="n_components = 9 exceeds"):
        fisher.pca_from_moments(50.0, np.zeros(8), np.eye(8), 9)
    with pytest.raises(ValueError, match="descs_per_video"):
        trajectories.TrajectoryClassifier().fit([], [])
    with pytest.raises(ValueError, match="not fitted"):
        trajectories.TrajectoryClassifier().encode([torch.zeros(1, 1)])
    # the host half of pca_fit equals the reference's on exact moments
    x = fo.mixture_rows(200, 6, 3, seed=2)[0]
    n, s, xtx = fo.moments(x)
    model = fisher.pca_from_moments(n, s, np.triu(xtx), 3)
    mean, comp, ev = fo.pca_from_moments(n, s, xtx, 3)
    assert model.n_samples == 200 and np.abs(model.mean - mean).max() == 0
    assert np.abs(model.components - comp).max() <= 1e-12 and np.abs(model.explained_variance - ev).max() <= 1e-12
