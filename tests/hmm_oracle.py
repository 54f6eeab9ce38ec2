"""DESIGN.md S97-S103 in numpy float64, written for reading: the emission loop over the columns, the composition of units
into one dense model, Viterbi and the scaled forward-backward pass over a dense log-transition matrix, the soft and hard
Gaussian statistics, the M-step and ``fit``.  It shares no code with video_analytics_amd.hmm: models
are dense matrices here (``log_a[i, j]``: from i to j, -inf where there is no edge) and CSR there.

``brute_force`` and ``brute_force_posteriors`` are the witnesses of the tests: every one of the N^T paths in
``np.longdouble``."""
import itertools
import math

import numpy as np

NEG_INF = float("-inf")


def emission_constants(variances, dtype=np.float64):
    """iv = 1 / var and c_g = -0.5 (D log 2 pi + sum_d log var_gd), the logarithms added in ascending d.  ``dtype``: float64, the
    specification, or np.longdouble, the witness of ``fit`` (here and in every function below that takes it)."""
    variances = np.asarray(variances, dtype=dtype)
    g, d = variances.shape
    s = np.zeros(g, dtype=dtype)
    for c in range(d):
        s = s + np.log(variances[:, c])
    log_2pi = math.log(2.0 * math.pi) if dtype is np.float64 else np.log(8 * np.arctan(np.longdouble(1)))
    return 1 / variances, -0.5 * (d * log_2pi + s)


def emissions(x, means, variances, dtype=np.float64):
    """S98: logB[t, g] = c_g - 0.5 q, q the sum over d in ascending order of ((x_d - mu_gd)(x_d - mu_gd)) iv_gd."""
    x = np.asarray(x).astype(dtype)  # float32 widens exactly
    means = np.asarray(means, dtype=dtype)
    iv, c = emission_constants(variances, dtype)
    q = np.zeros((x.shape[0], means.shape[0]), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(x.shape[1]):
            df = x[:, d, None] - means[None, :, d]
            q = q + (df * df) * iv[None, :, d]
        return c[None, :] - 0.5 * q


def left_to_right(n, self_prob=0.9, next_prob=0.1, dtype=np.float64):
    """Sheet04's unit: (log_pi [n], log_a [n,n], exit [n])."""
    with np.errstate(divide="ignore"):
        a = np.full((n, n), NEG_INF, dtype=dtype)
        for i in range(n):
            a[i, i] = np.log(dtype(self_prob))
            if i + 1 < n:
                a[i, i + 1] = np.log(dtype(next_prob))
        pi, ex = np.full(n, NEG_INF, dtype=dtype), np.full(n, NEG_INF, dtype=dtype)
        pi[0], ex[n - 1] = 0.0, np.log(dtype(next_prob))
    return pi, a, ex


def compose(units):
    """S97: ``units`` is a list of (first Gaussian, log_pi, log_a, exit) -> (emit, log_pi, log_a dense, log_final, unit_of_state)."""
    n = sum(len(u[1]) for u in units)
    emit, owner = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    log_pi, log_final, log_a = np.full(n, NEG_INF), np.full(n, NEG_INF), np.full((n, n), NEG_INF)
    base = 0
    for k, (first, pi, a, ex) in enumerate(units):
        m = len(pi)
        emit[base:base + m] = first + np.arange(m)
        owner[base:base + m] = k
        log_a[base:base + m, base:base + m] = a
        if k == 0:
            log_pi[:m] = pi
        if k == len(units) - 1:
            log_final[base:] = ex
        if k + 1 < len(units):
            nxt_pi = units[k + 1][1]
            for s in range(m):
                for s2 in range(len(nxt_pi)):
                    if ex[s] > NEG_INF and nxt_pi[s2] > NEG_INF:
                        log_a[base + s, base + m + s2] = ex[s] + nxt_pi[s2]
        base += m
    return emit, log_pi, log_a, log_final, owner


def viterbi(logb, emit, log_pi, log_a, log_final):
    """S99 -> (score, path int32 [T], status).  ``logb``: the sequence's rows [T, G], whose dtype the recursion runs in."""
    T, n = logb.shape[0], len(emit)
    delta = np.empty((T, n), dtype=logb.dtype)
    back = np.full((T, n), -1, dtype=np.int64)
    nan = False
    with np.errstate(invalid="ignore"):
        for j in range(n):
            delta[0, j] = log_pi[j] + logb[0, emit[j]]
        for t in range(1, T):
            for j in range(n):
                best, arg = NEG_INF, -1
                for i in range(n):
                    if log_a[i, j] == NEG_INF:
                        continue  # no edge
                    cand = delta[t - 1, i] + log_a[i, j]
                    if cand > best:
                        best, arg = cand, i
                delta[t, j] = best + logb[t, emit[j]]
                back[t, j] = arg
        final = delta[T - 1] + log_final
        nan = bool(np.isnan(delta).any() or np.isnan(final).any())
    if nan:
        return float("nan"), np.full(T, -1, dtype=np.int32), 2
    score, last = NEG_INF, -1
    for j in range(n):
        if final[j] > score:
            score, last = final[j], j
    if last < 0:
        return NEG_INF, np.full(T, -1, dtype=np.int32), 1
    path = np.empty(T, dtype=np.int32)
    path[T - 1] = last
    for t in range(T - 1, 0, -1):
        path[t - 1] = back[t, path[t]]
    return logb.dtype.type(score), path, 0


def viterbi_fast(logb, emit, log_pi, log_a, log_final):
    """The same recursion with the inner loops as array operations, for the long and wide cases of the GPU tests.  np.argmax
    returns the first maximum, which is the strict ``>`` rule in ascending order; a column of -inf alone gives predecessor 0
    where ``viterbi`` gives -1, which no path of finite score passes through."""
    T, n = logb.shape[0], len(emit)
    back = np.zeros((T, n), dtype=np.int64)
    nan = False
    with np.errstate(invalid="ignore"):
        delta = log_pi + logb[0, emit]
        nan |= bool(np.isnan(delta).any())
        for t in range(1, T):
            cand = delta[:, None] + log_a  # [from, to]
            cand_cmp = np.where(np.isnan(cand), NEG_INF, cand)  # a NaN candidate never wins by >
            arg = np.argmax(cand_cmp, axis=0)
            delta = cand_cmp[arg, np.arange(n)] + logb[t, emit]
            back[t] = arg
            nan |= bool(np.isnan(delta).any())
        final = delta + log_final
        nan |= bool(np.isnan(final).any())
    if nan:
        return float("nan"), np.full(T, -1, dtype=np.int32), 2
    last = int(np.argmax(final))
    if final[last] == NEG_INF:
        return NEG_INF, np.full(T, -1, dtype=np.int32), 1
    path = np.empty(T, dtype=np.int32)
    path[T - 1] = last
    for t in range(T - 1, 0, -1):
        path[t - 1] = back[t, path[t]]
    return float(final[last]), path, 0


def brute_force(logb, emit, log_pi, log_a, log_final):
    """Every path in np.longdouble -> (best score, best path, gap to the second-best path's score); (-inf, None, nan) when no
    path has a finite score."""
    T, n = logb.shape[0], len(emit)
    ld = np.longdouble
    scored = []
    for p in itertools.product(range(n), repeat=T):
        s = ld(log_pi[p[0]]) + ld(logb[0, emit[p[0]]])
        for t in range(1, T):
            s = s + ld(log_a[p[t - 1], p[t]]) + ld(logb[t, emit[p[t]]])
        s = s + ld(log_final[p[-1]])
        scored.append((s, p))
    scored.sort(key=lambda sp: (-sp[0], sp[1]))
    if scored[0][0] == -np.inf:
        return ld(-np.inf), None, float("nan")
    gap = scored[0][0] - scored[1][0] if len(scored) > 1 else ld(np.inf)
    return scored[0][0], np.array(scored[0][1], dtype=np.int32), gap


def forward_backward(logb, emit, log_pi, log_a, log_final):
    """S100 -> (gamma [T,N], xi_sum [N,N], loglik, status), in the dtype of ``logb``."""
    T, n, dt = logb.shape[0], len(emit), logb.dtype
    zero = (np.zeros((T, n), dtype=dt), np.zeros((n, n), dtype=dt))
    lb = logb[:, emit]
    if np.isnan(lb).any() or (lb == np.inf).any():
        return zero + (float("nan"), 2)
    m = lb.max(axis=1)
    if (m == NEG_INF).any():
        return zero + (NEG_INF, 1)
    with np.errstate(divide="ignore", under="ignore"):
        b = np.exp(lb - m[:, None])
        pi, a, f = np.exp(log_pi), np.exp(log_a), np.exp(log_final)
        alpha, c = np.zeros((T, n), dtype=dt), np.zeros(T, dtype=dt)
        for t in range(T):
            u = b[t] * (pi if t == 0 else alpha[t - 1] @ a)
            c[t] = u.sum()
            if not (c[t] > 0 and np.isfinite(c[t])):
                return zero + ((NEG_INF, 1) if c[t] == 0 else (float("nan"), 2))
            alpha[t] = u / c[t]
        c_end = (alpha[T - 1] * f).sum()
        if not (c_end > 0 and np.isfinite(c_end)):
            return zero + ((NEG_INF, 1) if c_end == 0 else (float("nan"), 2))
        beta = np.zeros((T, n), dtype=dt)
        beta[T - 1] = f / c_end
        xi = np.zeros((n, n), dtype=dt)
        for t in range(T - 2, -1, -1):
            w = (b[t + 1] * beta[t + 1]) / c[t + 1]
            beta[t] = a @ w
            xi = xi + (alpha[t][:, None] * a) * w[None, :]
        loglik = dt.type(0)
        for t in range(T):
            loglik = loglik + (np.log(c[t]) + m[t])
        loglik = loglik + np.log(c_end)
    return alpha * beta, xi, dt.type(loglik), 0


def brute_force_posteriors(logb, emit, log_pi, log_a, log_final):
    """Every path in np.longdouble -> (gamma [T,N], xi_sum [N,N], loglik), all longdouble; the likelihood must be positive."""
    T, n = logb.shape[0], len(emit)
    ld = np.longdouble
    gamma, xi, z = np.zeros((T, n), dtype=ld), np.zeros((n, n), dtype=ld), ld(0)
    for p in itertools.product(range(n), repeat=T):
        s = ld(log_pi[p[0]]) + ld(logb[0, emit[p[0]]])
        for t in range(1, T):
            s = s + ld(log_a[p[t - 1], p[t]]) + ld(logb[t, emit[p[t]]])
        s = s + ld(log_final[p[-1]])
        if s == -np.inf:
            continue
        w = np.exp(s)
        z = z + w
        for t in range(T):
            gamma[t, p[t]] += w
        for t in range(1, T):
            xi[p[t - 1], p[t]] += w
    assert z > 0
    return gamma / z, xi / z, np.log(z)


def forward_backward_longdouble(logb, emit, log_pi, src, tgt, log_p, log_final):
    """The witness where the enumeration cannot go: S100 in np.longdouble over an edge list (src -> tgt with log_p), so that
    a model of 1024 states costs its edges and not its square.  -> (gamma [T,N], xi_sum [E], loglik, sum of |loglik's terms|),
    all longdouble; the likelihood must be positive."""
    ld = np.longdouble
    T, n = logb.shape[0], len(emit)
    lb = logb[:, emit].astype(ld)
    m = lb.max(axis=1)
    b = np.exp(lb - m[:, None])
    with np.errstate(divide="ignore"):
        pi, a, f = np.exp(np.asarray(log_pi, dtype=ld)), np.exp(np.asarray(log_p, dtype=ld)), np.exp(np.asarray(log_final, dtype=ld))
    alpha, c = np.zeros((T, n), dtype=ld), np.zeros(T, dtype=ld)
    for t in range(T):
        if t == 0:
            u = pi * b[0]
        else:
            acc = np.zeros(n, dtype=ld)
            np.add.at(acc, tgt, alpha[t - 1][src] * a)
            u = b[t] * acc
        c[t] = u.sum()
        assert c[t] > 0
        alpha[t] = u / c[t]
    c_end = (alpha[T - 1] * f).sum()
    assert c_end > 0
    beta = np.zeros((T, n), dtype=ld)
    beta[T - 1] = f / c_end
    xi = np.zeros(len(src), dtype=ld)
    for t in range(T - 2, -1, -1):
        w = (b[t + 1] * beta[t + 1]) / c[t + 1]
        acc = np.zeros(n, dtype=ld)
        np.add.at(acc, src, a * w[tgt])
        beta[t] = acc
        xi = xi + alpha[t][src] * a * w[tgt]
    terms = np.concatenate([np.log(c), m, [np.log(c_end)]])
    return alpha * beta, xi, terms.sum(), np.abs(terms).sum()


def gauss_stats_soft(x, gammas, emits, firsts, n_gaussians):
    """[sum w | sum w x | sum w x^2] per Gaussian from the posteriors of the jobs: job k covers the rows from firsts[k] on and
    its state j feeds Gaussian emits[k][j]."""
    x = np.asarray(x).astype(gammas[0].dtype)  # float64, or the witness's longdouble
    d = x.shape[1]
    out = np.zeros((n_gaussians, 1 + 2 * d), dtype=x.dtype)
    for gm, emit, f0 in zip(gammas, emits, firsts):
        rows = x[f0:f0 + gm.shape[0]]
        for j, g in enumerate(emit):
            w = gm[:, j]
            out[g, 0] += w.sum()
            out[g, 1:1 + d] += (w[:, None] * rows).sum(axis=0)
            out[g, 1 + d:] += (w[:, None] * (rows * rows)).sum(axis=0)
    return out


def gauss_stats_hard(x, align, n_gaussians, dtype=np.float64):
    x = np.asarray(x).astype(dtype)
    d = x.shape[1]
    out = np.zeros((n_gaussians, 1 + 2 * d), dtype=dtype)
    for t, g in enumerate(align):
        if g >= 0:
            out[g, 0] += 1.0
            out[g, 1:1 + d] += x[t]
            out[g, 1 + d:] += x[t] * x[t]
    return out


def mstep_gaussians(stats, means, variances, var_floor, min_occupancy):
    means, variances = means.copy(), variances.copy()
    d = means.shape[1]
    for g in range(len(means)):
        s0 = stats[g, 0]
        if np.isfinite(s0) and s0 >= min_occupancy and s0 > 0:
            means[g] = stats[g, 1:1 + d] / s0
            variances[g] = stats[g, 1 + d:] / s0 - means[g] * means[g] + var_floor
    return means, variances


def mstep_unit(log_pi, log_a, exit_logp, xi_sum, start_sum, exit_sum):
    """Rows renormalised over the unit's own out-edges and its exit; a row without statistics is kept; absent edges stay
    absent.  -> (log_pi, log_a, exit_logp)."""
    n = len(log_pi)
    log_pi, log_a, exit_logp = log_pi.copy(), log_a.copy(), exit_logp.copy()
    with np.errstate(divide="ignore"):
        for i in range(n):
            have = log_a[i] > NEG_INF
            total = np.sum([xi_sum[i, j] for j in range(n) if have[j]] + ([exit_sum[i]] if exit_logp[i] > NEG_INF else []))
            if total > 0 and np.isfinite(total):
                log_a[i, have] = np.log(xi_sum[i, have] / total)
                if exit_logp[i] > NEG_INF:
                    exit_logp[i] = np.log(exit_sum[i] / total)
        have = log_pi > NEG_INF
        total = start_sum[have].sum()
        if total > 0 and np.isfinite(total):
            log_pi[have] = np.log(start_sum[have] / total)
    return log_pi, log_a, exit_logp


def fit(seqs, unit_of, counts, iters, method="baum-welch", var_floor=1e-6, min_occupancy=1e-3, self_prob=0.9, next_prob=0.1,
        init_alignments=None, dtype=np.float64):
    """S102 on a list of [T_i, D] arrays; ``unit_of[i]`` indexes ``counts`` (states per unit).  -> (means, variances, units as
    (log_pi, log_a, exit) per unit, logliks).  With ``dtype=np.longdouble`` every operation runs in long double: the witness."""
    x = np.concatenate(seqs).astype(dtype)
    d = x.shape[1]
    seg = np.concatenate([[0], np.cumsum([len(q) for q in seqs])])
    firsts = np.concatenate([[0], np.cumsum(counts)])
    g = int(firsts[-1])
    align = np.empty(len(x), dtype=np.int64)
    for i, q in enumerate(seqs):
        n = counts[unit_of[i]]
        local = (np.arange(len(q)) * n) // len(q) if init_alignments is None else np.asarray(init_alignments[i])
        align[seg[i]:seg[i + 1]] = firsts[unit_of[i]] + local
    means, variances = mstep_gaussians(gauss_stats_hard(x, align, g, dtype), np.zeros((g, d), dtype=dtype), np.ones((g, d), dtype=dtype),
                                       dtype(var_floor), min_occupancy)
    units = [left_to_right(n, self_prob, next_prob, dtype) for n in counts]
    logliks = []
    for _ in range(iters):
        logb = emissions(x, means, variances, dtype)
        xi_sum = [np.zeros((n, n), dtype=dtype) for n in counts]
        start_sum, exit_sum = [np.zeros(n, dtype=dtype) for n in counts], [np.zeros(n, dtype=dtype) for n in counts]
        total, gammas, emits = dtype(0), [], []
        align = np.full(len(x), -1, dtype=np.int64)
        for i in range(len(seqs)):
            u = unit_of[i]
            pi, a, ex = units[u]
            emit = firsts[u] + np.arange(counts[u])
            if method == "baum-welch":
                gm, xi, ll, st = forward_backward(logb[seg[i]:seg[i + 1]], emit, pi, a, ex)
                gammas.append(gm)
                emits.append(emit)
                xi_sum[u], start_sum[u], exit_sum[u] = xi_sum[u] + xi, start_sum[u] + gm[0], exit_sum[u] + gm[-1]
                total = total + ll
            else:
                score, path, st = viterbi(logb[seg[i]:seg[i + 1]], emit, pi, a, ex)
                total = total + score
                if st == 0:
                    align[seg[i]:seg[i + 1]] = emit[path]
                    for t in range(1, len(path)):
                        xi_sum[u][path[t - 1], path[t]] += 1.0
                    start_sum[u][path[0]] += 1.0
                    exit_sum[u][path[-1]] += 1.0
        logliks.append(total)
        stats = gauss_stats_soft(x, gammas, emits, seg[:-1], g) if method == "baum-welch" else gauss_stats_hard(x, align, g, dtype)
        means, variances = mstep_gaussians(stats, means, variances, dtype(var_floor), min_occupancy)
        units = [mstep_unit(*units[u], xi_sum[u], start_sum[u], exit_sum[u]) for u in range(len(counts))]
    return means, variances, units, logliks


def mean_over_frames(pred, true):
    pred, true = np.asarray(pred).ravel(), np.asarray(true).ravel()
    return float((pred == true).sum()) / len(pred)
