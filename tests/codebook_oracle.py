"""numpy float64 restatement of the bag-of-words specification (video_analytics_amd/csrc/codebook.hip):
assignment, update, k-means++ seeding, histograms and the Lloyd loop of ``codebook.kmeans_fit``.  Nothing here calls the
library.

1. Assignment.  ``label_i`` = the lowest ``j`` that attains ``min_j s_ij``, ``s_ij = 1/2 |c_j|^2 - x_i . c_j`` with ``|c_j|^2``
   summed over the columns in ascending order.  ``d2_i = sum_c (x_ic - c_{label,c})^2``, columns ascending, one rounding per
   operation: given the label it is reproduced bit for bit (``direct_d2``).
2. Update.  ``counts``, the cluster means (an empty cluster keeps its centre), ``shift2 = sum_j |new_j - old_j|^2``.
3. Seeding.  Plain k-means++ from ``u [K]``: centre 0 is row ``floor(u_0 n)``; for ``j >= 1``, ``m_i = min(m_i, |x_i -
   c_{j-1}|^2)`` in the direct form; the sums of ``m`` over blocks of 256 rows (rows past ``n`` count 0) by the tree
   ``block_sums``; ``pre_b`` = the sum of the blocks before ``b`` in ascending order, ``total`` the sum of all; the running
   sum of row ``i`` of block ``b`` is ``pre_b`` plus the block's rows up to ``i`` in ascending order; the chosen row is the
   lowest ``i`` whose running sum exceeds ``u_j total``, the last row with ``m_i > 0`` if there is none, ``floor(u_j n)``
   when ``total`` is not positive.  Rows and ``m`` are reproduced exactly.
4. Histograms.  Integer counts per segment, then divided once by the float64 norm taken over the words in ascending order.
"""
import numpy as np

BLOCK = 256


def half_norms(centres):
    c = np.asarray(centres, dtype=np.float64)
    acc = np.zeros(len(c))
    for a in range(c.shape[1]):
        acc = acc + c[:, a] * c[:, a]
    return 0.5 * acc


def scores(x, centres):
    """s [n, K] (the products in numpy's own order: compare through ``gaps``)"""
    return half_norms(centres)[None, :] - np.asarray(x, dtype=np.float64) @ np.asarray(centres, dtype=np.float64).T


def score_scale(x, centres):
    """scale_i = max_j sum_c |x_ic c_jc| + 1/2 max_j |c_j|^2"""
    return (np.abs(np.asarray(x, dtype=np.float64)) @ np.abs(np.asarray(centres, dtype=np.float64)).T).max(axis=1) + half_norms(centres).max()


def direct_d2(x, centres, labels):
    x, c = np.asarray(x, dtype=np.float64), np.asarray(centres, dtype=np.float64)[np.asarray(labels)]
    acc = np.zeros(len(x))
    for a in range(x.shape[1]):
        t = x[:, a] - c[:, a]
        acc = acc + t * t
    return acc


def assign(x, centres):
    """-> (labels int32 [n], d2 [n], s [n, K])"""
    s = scores(x, centres)
    labels = np.argmin(s, axis=1).astype(np.int32)  # the first of the lowest
    return labels, direct_d2(x, centres, labels), s


def gaps(s, scale):
    """(second-best - best) / scale per row; +inf with a single centre"""
    if s.shape[1] < 2:
        return np.full(len(s), np.inf)
    two = np.partition(s, 1, axis=1)[:, :2]
    return (two[:, 1] - two[:, 0]) / scale


def update(x, labels, centres):
    """-> (counts int64 [K], sums [K, d], new centres [K, d], shift2, abs_sums [K, d])"""
    x, old = np.asarray(x, dtype=np.float64), np.asarray(centres, dtype=np.float64)
    k = len(old)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    sums, abs_sums = np.zeros_like(old), np.zeros_like(old)
    np.add.at(sums, labels, x)
    np.add.at(abs_sums, labels, np.abs(x))
    new = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], old)
    shift2 = float(((new - old) ** 2).sum(axis=1).sum())
    return counts, sums, new, shift2, abs_sums


def block_sums(m):
    """The sums of m over blocks of 256 rows: per 64 rows an xor butterfly (offsets 32, 16, ..., 1), then ((w0 + w1) + w2) + w3"""
    nb = (len(m) + BLOCK - 1) // BLOCK
    a = np.zeros(nb * BLOCK)
    a[:len(m)] = m
    a = a.reshape(nb, 4, 64)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[:, :, lanes ^ off]
    w = a[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def floor_row(u, n):
    return min(int(np.floor(u * float(n))), n - 1)


def choose(m, u):
    """The row of one seeding step from m [n] and u in [0, 1)"""
    n = len(m)
    bs = block_sums(m)
    inc = np.cumsum(bs)  # sequential
    total = inc[-1]
    if not total > 0.0:
        return floor_row(u, n)
    t = u * total
    nb = len(bs)
    run = np.concatenate([[0.0], inc[:-1]])
    a = np.zeros(nb * BLOCK)
    a[:n] = m
    a = a.reshape(nb, BLOCK)
    first = np.full(nb, -1, dtype=np.int64)
    for r in range(BLOCK):
        run = run + a[:, r]
        row = np.arange(nb) * BLOCK + r
        hit = (first < 0) & (run > t) & (row < n)
        first[hit] = row[hit]
    if (first >= 0).any():
        return int(first[first >= 0].min())
    return int(np.nonzero(m > 0.0)[0].max())


def seed(x, k, u):
    """-> (rows int32 [k], centres [k, d], m [n] as after the last step; +inf when k = 1)"""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    rows = [floor_row(u[0], n)]
    m = np.full(n, np.inf)
    for j in range(1, k):
        m = np.minimum(m, direct_d2(x, x[rows[-1]][None, :].astype(np.float64), np.zeros(n, dtype=np.int64)))
        rows.append(choose(m, u[j]))
    rows = np.asarray(rows, dtype=np.int32)
    return rows, x[rows].astype(np.float64), m


def seed_witness(x, k, u):
    """The same rows by per-row Python loops (small inputs only)"""
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    rows = [min(int(np.floor(u[0] * float(n))), n - 1)]
    m = [np.inf] * n
    for j in range(1, k):
        c = x[rows[-1]]
        for i in range(n):
            acc = np.float64(0.0)
            for a in range(d):
                t = np.float64(x[i, a]) - np.float64(c[a])
                acc = acc + t * t
            m[i] = min(m[i], acc)
        nb = (n + BLOCK - 1) // BLOCK
        bs = []
        for b in range(nb):
            v = [np.float64(m[i]) if i < n else np.float64(0.0) for i in range(b * BLOCK, (b + 1) * BLOCK)]
            w = []
            for q in range(4):
                lanes = v[64 * q:64 * q + 64]
                for off in (32, 16, 8, 4, 2, 1):
                    lanes = [lanes[l] + lanes[l ^ off] for l in range(64)]
                w.append(lanes[0])
            bs.append(((w[0] + w[1]) + w[2]) + w[3])
        pre, run = [], np.float64(0.0)
        for b in range(nb):
            pre.append(run)
            run = run + bs[b]
        total = run
        if not total > 0.0:
            rows.append(min(int(np.floor(u[j] * float(n))), n - 1))
            continue
        t = u[j] * total
        pick, last = None, None
        for b in range(nb):
            run = pre[b]
            for i in range(b * BLOCK, min((b + 1) * BLOCK, n)):
                run = run + m[i]
                if pick is None and run > t:
                    pick = i
                if m[i] > 0.0:
                    last = i
        rows.append(pick if pick is not None else last)
    return np.asarray(rows, dtype=np.int32), np.asarray(m, dtype=np.float64)


def assign_witness(x, centres):
    """Labels and d2 by a per-row loop over the (x - c)^2 distances: the lowest index of the smallest distance"""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(centres, dtype=np.float64)
    labels, d2 = [], []
    for i in range(len(x)):
        dist = [float(((x[i] - c[j]) ** 2).sum()) for j in range(len(c))]
        j = int(np.argmin(dist))
        labels.append(j)
        d2.append(dist[j])
    return np.asarray(labels, dtype=np.int32), np.asarray(d2)


def histograms(labels, segments, k, norm="l2"):
    """-> (float64 [S, k] before the rounding to float32, integer counts [S, k])"""
    s = len(segments) - 1
    counts = np.zeros((s, k), dtype=np.int64)
    for v in range(s):
        counts[v] = np.bincount(labels[segments[v]:segments[v + 1]], minlength=k)
    c = counts.astype(np.float64)
    if norm == "none":
        return c, counts
    if norm == "l2":
        scale = np.sqrt(np.cumsum(c * c, axis=1)[:, -1])  # ascending, sequential
    elif norm == "l1":
        scale = np.cumsum(c, axis=1)[:, -1]
    else:
        raise ValueError(norm)
    out = np.where(scale[:, None] > 0, c / np.where(scale > 0, scale, 1.0)[:, None], 0.0)
    return out, counts


def tolerance(x, tol):
    """sklearn's: tol x the mean over the columns of np.var"""
    return float(tol) * float(np.mean(np.var(np.asarray(x, dtype=np.float64), axis=0)))


def lloyd(x, centres, steps):
    """``steps`` plain Lloyd steps (no stopping rule).  -> (centres, smallest count seen, smallest scaled gap seen)"""
    c = np.asarray(centres, dtype=np.float64)
    scale_floor, least = np.inf, np.inf
    for _ in range(steps):
        labels, _d2, s = assign(x, c)
        scale_floor = min(scale_floor, float(gaps(s, score_scale(x, c)).min()))
        counts, _sums, c, _shift2, _abs = update(x, labels, c)
        least = min(least, int(counts.min()))
    return c, least, scale_floor


def fit(x, init, max_iter=300, tol=1e-4):
    """``codebook.kmeans_fit`` from a given init.  -> dict(centres, inertia, n_iter, converged, counts, min_gap)"""
    c = np.asarray(init, dtype=np.float64)
    tol_scaled = tolerance(x, tol)
    prev, n_iter, converged, min_gap = None, 0, False, np.inf
    for it in range(1, max_iter + 1):
        labels, _d2, s = assign(x, c)
        min_gap = min(min_gap, float(gaps(s, score_scale(x, c)).min()))
        n_iter = it
        if prev is not None and np.array_equal(labels, prev):
            converged = True
            break
        _counts, _sums, c, shift2, _abs = update(x, labels, c)
        prev = labels
        if shift2 <= tol_scaled:
            converged = True
            break
    labels, d2, s = assign(x, c)
    min_gap = min(min_gap, float(gaps(s, score_scale(x, c)).min()))
    return dict(centres=c, inertia=float(d2.sum()), n_iter=n_iter, converged=converged,
                counts=np.bincount(labels, minlength=len(c)).astype(np.int64), min_gap=min_gap, labels=labels, d2=d2)
