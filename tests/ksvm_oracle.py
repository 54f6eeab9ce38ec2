"""The kernel SVM restated in numpy float64 (the checker of tests/test_ksvm_host.py and tests/test_ksvm_gpu.py): the Gram
matrices in the device's written order, the dual problem, its bound, and the device's solver step for step (DESIGN.md
S104-S109).

For class row r with y_i = +-1, kernel K, Kt = K + s^2 (s = intercept_scaling) the dual of ``svm_fit_oracle``'s f_r is

    min over alpha >= 0 of   q(alpha) = 1/2 alpha^T ((y y^T) o Kt + I / (2C)) alpha - e^T alpha,

``dual_coef[r] = beta = y alpha``, ``intercept[r] = s^2 sum(beta)``.  q is 1/(2C)-strongly convex, so with the projected
gradient pg (g where alpha > 0, min(g, 0) where alpha = 0)

    |alpha - alpha*|_2 <= 2C |pg(alpha)|_2      for every feasible alpha,

the only tolerance the solver tests use."""
import numpy as np

from svm_fit_oracle import signs

CG_STEPS, LS_TRIALS, ARMIJO = 100, 40, 1e-4  # ksvm.hip's kKsvmCgSteps, kKsvmLsTrials, kKsvmArmijo


# ---- Gram matrices ---------------------------------------------------------------------------------------------------------

def chi2_distance(x, y=None, columns=None):
    """D[i][j] = sum_k (x_ik - y_jk)^2 / (x_ik + y_jk), k ascending over ``columns = (c0, c1)``, every operation IEEE float64
    and a term with x_ik + y_jk = 0 counted as 0: the device's bits."""
    x = np.asarray(x).astype(np.float64)
    y = x if y is None else np.asarray(y).astype(np.float64)
    c0, c1 = (0, x.shape[1]) if columns is None else columns
    acc = np.zeros((x.shape[0], y.shape[0]))
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(c0, c1):
            a, b = x[:, k][:, None], y[:, k][None, :]
            d, s = a - b, a + b
            acc = acc + np.where(s == 0.0, 0.0, (d * d) / s)
    return acc


def chi2_distance_witness(x, y=None, columns=None):
    """The same sum in long double."""
    x = np.asarray(x).astype(np.longdouble)
    y = x if y is None else np.asarray(y).astype(np.longdouble)
    c0, c1 = (0, x.shape[1]) if columns is None else columns
    a, b = x[:, None, c0:c1], y[None, :, c0:c1]
    s = a + b
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(s == 0, 0, (a - b) * (a - b) / np.where(s == 0, 1, s)).sum(-1)


def linear_gram(x, y=None):
    x = np.asarray(x).astype(np.float64)
    y = x if y is None else np.asarray(y).astype(np.float64)
    return x @ y.T


def linear_gram_witness(x, y=None):
    x = np.asarray(x).astype(np.longdouble)
    y = x if y is None else np.asarray(y).astype(np.longdouble)
    return (x[:, None, :] * y[None, :, :]).sum(-1)


def upper_mean(D):
    """The mean of the strict upper triangle, float64."""
    D = np.asarray(D, dtype=np.float64)
    iu = np.triu_indices(D.shape[0], 1)
    return float(D[iu].sum() / len(iu[0]))


def upper_mean_witness(D):
    D = np.asarray(D).astype(np.longdouble)
    iu = np.triu_indices(D.shape[0], 1)
    return D[iu].sum() / np.longdouble(len(iu[0]))


def combine_argument(dists, weights):
    """sum_c w_c D_c in channel order, multiply then add: the argument of the device's exp, bit for bit."""
    acc = np.float64(weights[0]) * np.asarray(dists[0], dtype=np.float64)
    for w, D in zip(weights[1:], dists[1:]):
        acc = acc + np.float64(w) * np.asarray(D, dtype=np.float64)
    return acc


def combine(dists, weights):
    return np.exp(-combine_argument(dists, weights))


def chi2_kernel(x, y=None, gamma=None, channels=None, scales=None):
    """-> (K, scales) as ``ksvm.chi2_kernel``."""
    x = np.asarray(x, dtype=np.float64)
    channels = [(0, x.shape[1])] if channels is None else list(channels)
    dists = [chi2_distance(x, y, ch) for ch in channels]
    if scales is None:
        scales = [float(gamma)] * len(channels) if gamma is not None else [1.0 / upper_mean(D) for D in dists]
    return combine(dists, scales), np.asarray(scales, dtype=np.float64)


# ---- the dual problem ------------------------------------------------------------------------------------------------------

def hessian(K, C, intercept_scaling=1.0):
    """H = K + s^2 + I / (2C): what every class row shares in beta."""
    K = np.asarray(K, dtype=np.float64)
    return K + float(intercept_scaling) ** 2 + np.eye(K.shape[0]) / (2.0 * C)


def projected_gradient(beta, K, Y, C, intercept_scaling=1.0):
    """-> (pg [rows, n], alpha [rows, n]) of dual coefficients beta [rows, n]; Y = signs(labels, classes)."""
    beta = np.atleast_2d(np.asarray(beta, dtype=np.float64))
    alpha = Y * beta
    g = Y * (beta @ hessian(K, C, intercept_scaling)) - 1.0
    return np.where(alpha > 0.0, g, np.minimum(g, 0.0)), alpha


def pg_norms(beta, K, Y, C, intercept_scaling=1.0):
    return np.linalg.norm(projected_gradient(beta, K, Y, C, intercept_scaling)[0], axis=1)


def nnls_witness(K, Y, C, intercept_scaling=1.0):
    """The independent solution: scipy's NNLS on the Cholesky factor of (y y^T) o Kt + I / (2C).  -> beta [rows, n]."""
    from scipy.linalg import solve_triangular
    from scipy.optimize import nnls
    H = hessian(K, C, intercept_scaling)
    out = np.zeros(Y.shape)
    for r, y in enumerate(Y):
        L = np.linalg.cholesky((y[:, None] * y[None, :]) * H)
        alpha, _ = nnls(L.T, solve_triangular(L, np.ones(len(y)), lower=True), maxiter=100 * len(y))
        out[r] = y * alpha
    return out


def primal_weights(beta, X, intercept_scaling=1.0):
    """W = beta [X, s]: the primal solver's [rows, d + 1]."""
    X = np.asarray(X, dtype=np.float64)
    Xa = np.concatenate([X, np.full((X.shape[0], 1), float(intercept_scaling))], axis=1)
    return np.atleast_2d(beta) @ Xa


# ---- the device's solver, step for step -------------------------------------------------------------------------------------
#
# A Newton-CG on the primal written in beta (f = Kt beta; P(beta) = 1/2 beta^T Kt beta + C sum max(0, 1 - y f)^2), whose Newton
# system on the violators V = {1 - y f > 0} is H_VV x_V = y_V with x = 0 elsewhere: the dual's optimality system on the face V.
# Every outer step judges the FEASIBLE candidate bc (beta on V where y beta > 0, exactly 0 elsewhere) by the dual's projected
# gradient, and starts the CG from it.

def masked_product(H, V, mask=None):
    """out[r] = H V[r], zeroed where mask[r] is false."""
    out = V @ H
    return out if mask is None else np.where(mask, out, 0.0)


def face(H, B, Y, C, HB=None):
    """EVAL, first half -> dict(HB, sv, BC, ref): violators, the feasible candidate, |beta - 2C y max(0, 1 - y f)| / (2C).
    ``HB``: the product H B where the caller has it (a stage test passes the device's)."""
    HB = masked_product(H, B) if HB is None else HB
    m = 1.0 - Y * (HB - B / (2.0 * C))
    sv = m > 0.0
    BC = np.where(sv & (Y * B > 0.0), B, 0.0)
    diff = B - np.where(sv, 2.0 * C * Y * m, 0.0)
    return {"HB": HB, "sv": sv, "BC": BC, "ref": np.sqrt((diff * diff).sum(1)) / (2.0 * C)}


def grad(H, fc, Y, tol, tight=None):
    """EVAL, second half -> dict(Z, pgn, stop, R, rr, cgtol, live, nsv, q): the projected gradient of BC and the CG's start."""
    n = H.shape[0]
    BC, sv = fc["BC"], fc["sv"]
    Z = masked_product(H, BC)
    g = Y * Z - 1.0
    pg = np.where(Y * BC > 0.0, g, np.minimum(g, 0.0))
    pgn = np.sqrt((pg * pg).sum(1))
    R = np.where(sv, Y - Z, 0.0)
    rr = (R * R).sum(1)
    eta = np.minimum(0.1, np.sqrt(fc["ref"] / np.sqrt(n)))
    if tight is not None:
        eta = np.where(tight, 0.0, eta)
    cgtol = np.maximum(eta * fc["ref"], 0.25 * tol * np.sqrt(n))
    stop = pgn <= tol * np.sqrt(n)
    return {"Z": Z, "pgn": pgn, "stop": stop, "R": R, "rr": rr, "cgtol": cgtol, "live": ~stop & (np.sqrt(rr) > cgtol),
            "nsv": (BC != 0.0).sum(1), "q": (BC * (0.5 * Z - Y)).sum(1)}


def cg_step(H, free, X, R, P, rr, cgtol, live):
    """One CG round of every live row, in place -> the CG steps taken (0 or 1 per row)."""
    HP = masked_product(H, P, free)
    took = np.zeros(len(X), dtype=np.int64)
    for r in np.nonzero(live)[0]:
        php = P[r] @ HP[r]
        if not php > 0.0:
            live[r] = False
            continue
        alpha = rr[r] / php
        X[r] = X[r] + alpha * P[r]
        R[r] = R[r] - alpha * HP[r]
        rn = R[r] @ R[r]
        took[r] = 1
        if np.sqrt(rn) <= cgtol[r]:
            live[r] = False
            continue
        P[r] = R[r] + (rn / rr[r]) * P[r]
        rr[r] = rn
    return took


def line_search(H, b, HB, S, y, C, Q=None):
    """The Armijo search of one row along beta + t S on P, with no product beyond Q = H S -> (new beta, t or 0.0)."""
    Q = H @ S if Q is None else Q
    KS = Q - S / (2.0 * C)
    f = HB - b / (2.0 * C)
    h0 = np.maximum(0.0, 1.0 - y * f)
    slope = KS @ (b - 2.0 * C * y * h0)
    bKS, sKS = b @ KS, S @ KS
    if not slope < 0.0:
        return b, 0.0
    t = 1.0
    for _ in range(LS_TRIALS):
        ht = np.maximum(0.0, 1.0 - y * (f + t * KS))
        delta = t * bKS + 0.5 * t * t * sKS + C * ((ht - h0) * (ht + h0)).sum()
        if delta <= ARMIJO * t * slope:
            return b + t * S, t
        t = 0.5 * t
    return b, 0.0


def dual_fit(K, labels, C=1.0, tol=1e-8, max_iter=100, intercept_scaling=1.0):
    """The device's solver -> (dual_coef [rows, n], intercept [rows], classes, info)."""
    classes = np.unique(labels)
    Y = signs(labels, classes)
    rows, n = Y.shape
    H = hessian(K, C, intercept_scaling)
    B, out = np.zeros((rows, n)), np.zeros((rows, n))
    notdone, tight = np.ones(rows, dtype=bool), np.zeros(rows, dtype=bool)
    steps, cgs = np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int64)
    pgn = np.zeros(rows)
    for it in range(max_iter + 1):
        fc = face(H, B, Y, C)
        gr = grad(H, fc, Y, tol, tight)
        out = np.where(notdone[:, None], fc["BC"], out)
        pgn = np.where(notdone, gr["pgn"], pgn)
        notdone &= ~gr["stop"]
        if not notdone.any() or it == max_iter:
            break
        X, R, P, rr = fc["BC"].copy(), gr["R"].copy(), gr["R"].copy(), gr["rr"].copy()
        live = gr["live"] & notdone
        for _ in range(CG_STEPS):
            if not live.any():
                break
            cgs += cg_step(H, fc["sv"], X, R, P, rr, gr["cgtol"], live)
        for r in np.nonzero(notdone)[0]:
            B[r], t = line_search(H, B[r], fc["HB"][r], X[r] - B[r], Y[r], C)
            steps[r] += t > 0.0
            tight[r] = not t > 0.0
    s2 = float(intercept_scaling) ** 2
    info = {"n_iter": int(steps.max()), "rel_pg": pgn / np.sqrt(n), "converged": not notdone.any(), "steps": steps, "cg_steps": cgs,
            "n_sv": (out != 0.0).sum(1), "stopped": ~notdone}
    return out, s2 * out.sum(1), classes, info


# ---- the test problems -------------------------------------------------------------------------------------------------------

def blobs(n, d, c, sep, seed=0):
    """X = centres[label] * sep + N(0, 1), labels = arange(n) % c."""
    rng = np.random.RandomState(seed)
    labels = np.arange(n) % c
    centres = rng.randn(c, d)
    return centres[labels] * sep + rng.randn(n, d), labels


def histograms(n, d, seed=0, zero_share=0.3):
    """Non-negative rows for the chi-square kernels: an all-zero column, about 30 % scattered zeros, two identical rows."""
    rng = np.random.RandomState(seed)
    x = rng.rand(n, d) * (rng.rand(n, d) >= zero_share)
    if d > 1:
        x[:, d // 2] = 0.0
    if n > 1:
        x[n - 1] = x[0]
    return x


SOLVER_PROBLEMS = {  # name: (n, d, c, C, sep)
    "three_classes": (130, 17, 3, 10.0, 4.0),
    "sixty_five_classes": (130, 17, 65, 1.0, 4.0),
    "two_classes": (65, 3, 2, 100.0, 6.0),
}


def solver_problem(name):
    """The problems the solver tests fit -> (X or histograms, labels, C, intercept_scaling, kernel)."""
    if name in SOLVER_PROBLEMS:
        n, d, c, C, sep = SOLVER_PROBLEMS[name]
        return blobs(n, d, c, sep) + (C, 1.0, "linear")
    if name == "tiny_C":  # every point a support vector: |f| stays far below 1
        X, lab = blobs(130, 17, 3, 4.0, seed=1)
        return 0.02 * X, lab, 0.01, 1.0, "linear"
    if name == "duplicated_rows":  # singular K
        X, lab = blobs(64, 5, 3, 2.0, seed=2)
        return np.concatenate([X, X[:16]]), np.concatenate([lab, lab[:16]]), 10.0, 1.0, "linear"
    if name == "no_intercept":
        return blobs(130, 17, 3, 4.0, seed=3) + (10.0, 0.0, "linear")
    if name == "wide":  # d = 300 > n = 65
        return blobs(65, 300, 4, 1.0, seed=4) + (1.0, 2.5, "linear")
    assert name == "chi2"
    h, lab = histograms(130, 67, seed=5), np.arange(130) % 5
    h[lab == 1, :10] += 1.0
    h[lab == 2, 10:20] += 1.0
    return h, lab, 10.0, 1.0, "chi2"


PROBLEMS = tuple(SOLVER_PROBLEMS) + ("tiny_C", "duplicated_rows", "no_intercept", "wide", "chi2")
