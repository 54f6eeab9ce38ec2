"""The numpy reference of the Fisher-vector feature: plain float64, the direct ``(x - mu)^2 / var`` form of
the log-density, no chunking, numpy's own summation.  The tests hold ``video_analytics_amd.fisher`` to it and hold it, in
turn, to scikit-learn and to a literal per-component restatement (tests/test_fisher_host.py)."""
import numpy as np

EPSILON = 1e-6
LOG_2PI = float(np.log(2.0 * np.pi))


# ---- PCA -----------------------------------------------------------------------------------------------------------------

def moments(x):
    """-> (row count, column sums [d], X^T X [d,d]) of float32 rows, in float64"""
    x = np.asarray(x, dtype=np.float64)
    return float(x.shape[0]), x.sum(0), x.T @ x


def moments_scale(x):
    """the sums of the absolute values of the terms of ``moments``"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    return float(a.shape[0]), a.sum(0), a.T @ a


def pca_from_moments(count, colsum, xtx, n_components):
    """covariance with ddof = 1, eigh, descending eigenvalues, each component's largest-magnitude entry positive
    -> (mean [d], components [m,d], explained_variance [m])"""
    n = int(round(count))
    mean = colsum / n
    cov = (xtx - n * np.outer(mean, mean)) / (n - 1)
    cov = np.triu(cov) + np.triu(cov, 1).T
    vals, vecs = np.linalg.eigh(cov)
    vals, vecs = vals[::-1][:n_components], np.ascontiguousarray(vecs[:, ::-1][:, :n_components].T)
    big = np.argmax(np.abs(vecs), axis=1)
    vecs = vecs * np.sign(vecs[np.arange(len(vecs)), big])[:, None]
    return mean, vecs, vals


def pca_fit(x, n_components):
    return pca_from_moments(*moments(x), n_components=n_components)


def pca_transform(x, mean, components):
    return (np.asarray(x, dtype=np.float64) - mean) @ components.T


def pca_transform_scale(x, mean, components):
    return np.abs(np.asarray(x, dtype=np.float64) - mean) @ np.abs(components).T


# ---- the mixture ---------------------------------------------------------------------------------------------------------

def log_prob(x, w, mu, var):
    """log p_k of every row [n,k], direct form"""
    x = np.asarray(x, dtype=np.float64)
    quad = np.stack([(((x - mu[j]) ** 2) / var[j]).sum(1) for j in range(len(w))], axis=1)
    return np.log(w)[None] - 0.5 * quad - 0.5 * np.log(var).sum(1)[None] - 0.5 * x.shape[1] * LOG_2PI


def log_prob_scale(x, w, mu, var):
    """the sum of the absolute values of the terms the expanded form of ``log_prob`` accumulates:
    x^2 / (2 var), x mu / var, mu^2 / (2 var), log var / 2, log w, d/2 log 2 pi"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    return ((a ** 2) @ (0.5 / var).T + a @ (np.abs(mu) / var).T + (0.5 * mu ** 2 / var).sum(1)[None] + 0.5 * np.abs(np.log(var)).sum(1)[None]
            + np.abs(np.log(w))[None] + 0.5 * a.shape[1] * LOG_2PI)


def logsumexp(lp):
    m = lp.max(1)
    return m + np.log(np.exp(lp - m[:, None]).sum(1))


def posteriors(x, w, mu, var):
    """-> (gamma [n,k], logsumexp [n])"""
    lp = log_prob(x, w, mu, var)
    lse = logsumexp(lp)
    return np.exp(lp - lse[:, None]), lse


def hard_assignments(x, w, mu, var):
    """-> (arg-max of log p per row, lowest k on ties; the gap between the best and the second-best log p, inf for k = 1)"""
    lp = log_prob(x, w, mu, var)
    best = np.argmax(lp, axis=1)
    if lp.shape[1] == 1:
        return best, np.full(len(lp), np.inf)
    srt = np.sort(lp, axis=1)
    return best, srt[:, -1] - srt[:, -2]


def one_hot(best, k):
    g = np.zeros((len(best), k))
    g[np.arange(len(best)), best] = 1.0
    return g


def stats_from_gamma(x, gamma, segments):
    """-> stats [n_segments, k, 1 + 2d] = [S0 | S1 | S2]"""
    x = np.asarray(x, dtype=np.float64)
    k, d = gamma.shape[1], x.shape[1]
    out = np.zeros((len(segments) - 1, k, 1 + 2 * d))
    for s in range(len(segments) - 1):
        a, b = int(segments[s]), int(segments[s + 1])
        g, xs = gamma[a:b], x[a:b]
        out[s, :, 0] = g.sum(0)
        out[s, :, 1:1 + d] = g.T @ xs
        out[s, :, 1 + d:] = g.T @ (xs * xs)
    return out


def stats(x, segments, w, mu, var, mode="soft"):
    """-> (stats, loglik [n_segments], stats_scale): the last is stats with |x| in place of x (gamma >= 0), the sum of the
    absolute values of the terms each statistic accumulates"""
    gamma, lse = posteriors(x, w, mu, var)
    if mode == "hard":
        gamma = one_hot(hard_assignments(x, w, mu, var)[0], len(w))
    ll = np.array([lse[int(segments[s]):int(segments[s + 1])].sum() for s in range(len(segments) - 1)])
    return stats_from_gamma(x, gamma, segments), ll, stats_from_gamma(np.abs(np.asarray(x, dtype=np.float64)), gamma, segments)


def loglik_scale(x, segments, w, mu, var):
    lse = np.abs(posteriors(x, w, mu, var)[1])
    return np.array([lse[int(segments[s]):int(segments[s + 1])].sum() for s in range(len(segments) - 1)])


def mstep(st, reg_covar=1e-6):
    """sklearn's diagonal M-step from stats [k, 1 + 2d] -> (weights, means, variances)"""
    d = (st.shape[1] - 1) // 2
    nk = st[:, 0] + 10.0 * np.finfo(np.float64).eps
    s1, s2 = st[:, 1:1 + d], st[:, 1 + d:]
    mu = s1 / nk[:, None]
    var = s2 / nk[:, None] - 2.0 * (mu * s1 / nk[:, None]) + mu * mu + reg_covar
    return nk / nk.sum(), mu, var


def em(x, w, mu, var, max_iter, tol=0.0, reg_covar=1e-6):
    """EM from the given parameters, sklearn's loop: E-step, M-step, stop when the mean log-likelihood moves by less than tol
    -> (weights, means, variances, history, converged)"""
    n = len(x)
    seg = [0, n]
    history, prev, converged = [], -np.inf, False
    for _ in range(max_iter):
        st, ll, _ = stats(x, seg, w, mu, var)
        w, mu, var = mstep(st[0], reg_covar)
        lb = ll[0] / n
        history.append(lb)
        if abs(lb - prev) < tol:
            converged = True
            break
        prev = lb
    return w, mu, var, history, converged


def init(x, k, seed=0, kmeans_iters=10, reg_covar=1e-6):
    """the initial parameters of ``gmm_fit``: rows ``RandomState(seed).permutation(N)[:k]`` as means, ``kmeans_iters`` Lloyd
    steps (an empty cluster keeps its mean), one more hard pass and the M-step on its one-hot statistics"""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    mu = x[np.random.RandomState(seed).permutation(n)[:k]].copy()
    w, var = np.full(k, 1.0 / k), np.ones((k, d))
    for _ in range(kmeans_iters):
        st = stats(x, [0, n], w, mu, var, "hard")[0][0]
        full = st[:, 0] > 0
        mu[full] = st[full, 1:1 + d] / st[full, :1]
    return mstep(stats(x, [0, n], w, mu, var, "hard")[0][0], reg_covar)


# ---- Fisher vectors ------------------------------------------------------------------------------------------------------

def fisher_from_stats(st, count, w, mu, var, power=0.0):
    """one segment's Fisher vector (float64) from its stats [k, 1 + 2d] and row count"""
    k, d = mu.shape
    if count == 0:
        return np.zeros(k + 2 * k * d)
    s0, s1, s2 = st[:, :1], st[:, 1:1 + d], st[:, 1 + d:]
    wk = w[:, None]
    g_a = (s0 - count * wk) / np.sqrt(wk)
    g_m = (s1 - mu * s0) / (np.sqrt(var) * np.sqrt(wk))
    g_s = (((s2 - 2.0 * mu * s1) + mu * mu * s0) / var - s0) / np.sqrt(2.0 * wk)
    v = np.concatenate([g_a.ravel(), g_m.ravel(), g_s.ravel()]) / count
    if power > 0:
        v = np.sign(v) * np.abs(v) ** power
    norm = np.sqrt((v * v).sum())
    return v if norm < EPSILON else v / norm


def fisher_vectors(x, segments, w, mu, var, power=0.0):
    st = stats(x, segments, w, mu, var)[0]
    return np.stack([fisher_from_stats(st[s], int(segments[s + 1]) - int(segments[s]), w, mu, var, power) for s in range(len(st))])


# ---- test data -----------------------------------------------------------------------------------------------------------

def mixture_rows(n, d, k, seed, spread=3.0):
    """float32 rows [n,d] drawn from k well separated diagonal Gaussians, and reasonable parameters for them
    -> (x, weights, means, variances)"""
    rng = np.random.RandomState(seed)
    mu = rng.randn(k, d) * spread
    var = 0.5 + rng.rand(k, d)
    w = 0.5 + rng.rand(k)
    w /= w.sum()
    z = rng.randint(0, k, size=n)
    x = (mu[z] + rng.randn(n, d) * np.sqrt(var[z])).astype(np.float32)
    return x, w, mu, var
