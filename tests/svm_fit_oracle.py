"""The fusion SVM's fit restated in numpy float64 (the checker of tests/test_svm_fit_host.py and tests/test_svm_fit_gpu.py):
liblinear's L2R_L2LOSS_SVC as ``LinearSVC()`` poses it, one-vs-rest.  For class row r

    f_r(w) = 1/2 |w|^2 + C sum_i max(0, 1 - y_i w.[x_i, s])^2,    w in R^(d+1),  s = intercept_scaling,

``coef[r] = w[:d]``, ``intercept[r] = s w[d]`` (the bias is regularised).  f_r is 1-strongly convex, so
``|w - w*| <= |grad f_r(w)|`` for the minimiser w*: two approximate solutions are never further apart than the sum of
their gradient norms -- the only tolerance the tests use."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svm_fit_small.npz")
N_PROBLEMS = 6


def load_golden():
    """-> list of dicts: X [n,d], labels [n], X_test [200,d] (float64), coef, intercept, classes (sklearn's)."""
    z = np.load(GOLDEN)
    out = []
    for p in range(1, N_PROBLEMS + 1):
        out.append({"X": z["p%d_X" % p].astype(np.float64), "labels": z["p%d_labels" % p], "X_test": z["p%d_X_test" % p].astype(np.float64),
                    "coef": z["p%d_coef" % p], "intercept": z["p%d_intercept" % p], "classes": z["p%d_classes" % p]})
    return out


def signs(labels, classes):
    """The label -> +-1 map: [rows, n] with +1 where ``labels[i] == classes[r]``; two classes give ONE row, for classes[1]."""
    labels, classes = np.asarray(labels), np.asarray(classes)
    pos = classes[1:] if len(classes) == 2 else classes
    return np.where(labels[None, :] == pos[:, None], 1.0, -1.0)


def augmented(X, intercept_scaling=1.0):
    X = np.asarray(X, dtype=np.float64)
    return np.concatenate([X, np.full((X.shape[0], 1), float(intercept_scaling))], axis=1)


def pack(coef, intercept, intercept_scaling=1.0):
    """[coef, intercept / s] -> the solver's w [rows, d+1] (s = 0: the bias coordinate is 0)."""
    coef = np.atleast_2d(np.asarray(coef, dtype=np.float64))
    b = np.atleast_1d(np.asarray(intercept, dtype=np.float64))
    last = b / intercept_scaling if intercept_scaling > 0 else np.zeros_like(b)
    return np.concatenate([coef, last[:, None]], axis=1)


def objective(W, Xa, Y, C=1.0):
    """f_r for every row: W [rows, d+1], Xa [n, d+1], Y [rows, n] -> [rows]."""
    h = np.maximum(0.0, 1.0 - Y * (W @ Xa.T))
    return 0.5 * (W * W).sum(1) + C * (h * h).sum(1)


def gradient(W, Xa, Y, C=1.0):
    """grad f_r for every row -> [rows, d+1]: w + 2C sum_{active} (m_i - y_i) x_i."""
    m = W @ Xa.T
    u = np.where(1.0 - Y * m > 0.0, m - Y, 0.0)
    return W + 2.0 * C * (u @ Xa)


def model_gradient_norms(coef, intercept, X, labels, classes, C=1.0, intercept_scaling=1.0):
    """-> (|grad f_r| [rows], |grad f_r(0)| [rows]) of a model given as sklearn gives it."""
    Xa, Y = augmented(X, intercept_scaling), signs(labels, classes)
    W = pack(coef, intercept, intercept_scaling)
    return np.linalg.norm(gradient(W, Xa, Y, C), axis=1), np.linalg.norm(gradient(np.zeros_like(W), Xa, Y, C), axis=1)


def newton_cg(X, labels, C=1.0, tol=1e-10, max_iter=100, intercept_scaling=1.0):
    """A plain Newton-CG, one class row after the other -> (coef, intercept, classes, Newton steps per row, CG steps)."""
    classes = np.unique(labels)
    Xa, Y = augmented(X, intercept_scaling), signs(labels, classes)
    rows, D = Y.shape[0], Xa.shape[1]
    W = np.zeros((rows, D))
    steps, cg_total = np.zeros(rows, dtype=int), 0
    for r in range(rows):
        y, w = Y[r], np.zeros(D)

        def f(v):
            h = np.maximum(0.0, 1.0 - y * (Xa @ v))
            return 0.5 * v @ v + C * h @ h

        g0 = None
        for _ in range(max_iter):
            m = Xa @ w
            act = 1.0 - y * m > 0.0
            g = w + 2.0 * C * (Xa[act].T @ (m[act] - y[act]))
            gn = np.linalg.norm(g)
            g0 = gn if g0 is None else g0
            if gn <= tol * g0:
                break
            Xact = Xa[act]
            s, res = np.zeros(D), -g
            p, rr = res.copy(), res @ res
            cgtol = min(0.1, np.sqrt(gn / g0)) * gn
            for _ in range(10 * D):
                hp = p + 2.0 * C * (Xact.T @ (Xact @ p))
                alpha = rr / (p @ hp)
                s, res = s + alpha * p, res - alpha * hp
                cg_total += 1
                rn = res @ res
                if np.sqrt(rn) <= cgtol:
                    break
                p, rr = res + (rn / rr) * p, rn
            t, f0, gs = 1.0, f(w), g @ s
            while f(w + t * s) > f0 + 1e-4 * t * gs and t > 1e-12:
                t *= 0.5
            w = w + t * s
            steps[r] += 1
        W[r] = w
    return W[:, :-1].copy(), intercept_scaling * W[:, -1], classes, steps, cg_total


def predict(X, coef, intercept, classes):
    s = np.asarray(X, dtype=np.float64) @ np.atleast_2d(coef).T + np.atleast_1d(intercept)
    classes = np.asarray(classes)
    return classes[(s[:, 0] > 0).astype(int)] if s.shape[1] == 1 else classes[s.argmax(1)]
