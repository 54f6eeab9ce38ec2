"""Writes tests/golden/svm_fit_small.npz: six small fusion-SVM problems with the solution of
``LinearSVC(tol=1e-12, max_iter=5_000_000, dual=False)`` (needs sklearn; run from the repository root:
``python tests/golden/make_svm_fit_golden.py``).

The data are seeded post-ReLU descriptors, ``max(0, 0.3 mu_class + N(0,1))``, rounded to float16 (stored as such to keep the
file small; the tests and the fit below use exactly those values as float64).  Every problem has one all-zero column, one
repeated row, every class present and 200 held-out rows.  Two conditions are asserted on what is stored:
the gradient norm of sklearn's solution is <= 1e-5 in every row, and the smallest top-2 score margin on the held-out rows
(|score| for the binary problem) is >= 1e-3.  If a seed breaks either, change the seed, not the bound."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import svm_fit_oracle as so  # noqa: E402

# (n, d, class labels, seed)
PROBLEMS = [
    (97, 37, np.arange(1, 4), 101),            # 1-based labels
    (64, 24, np.array([4, 9]), 102),           # binary: one row
    (40, 64, np.arange(4), 103),               # n < d
    (210, 33, np.arange(70), 204),             # classes across a 64-wide tile edge
    (300, 202, np.arange(101), 905),           # the stacked-scores shape
    (257, 129, np.arange(5), 606),             # every extent one past a power of two
]
N_TEST = 200


def make(n, d, names, seed):
    rng = np.random.RandomState(seed)
    k = len(names)
    mu = rng.randn(k, d)
    idx = np.concatenate([np.arange(k), rng.randint(0, k, size=n + N_TEST - k)])  # every class present in the training rows
    head = rng.permutation(n)
    idx[:n] = idx[:n][head]
    X = np.maximum(0.0, 0.3 * mu[idx] + rng.randn(n + N_TEST, d))
    X[:, d // 3] = 0.0                    # one all-zero column
    X[n - 1], idx[n - 1] = X[0], idx[0]   # one repeated row
    X = X.astype(np.float16)
    assert len(np.unique(idx[:n])) == k
    return X[:n], names[idx[:n]], X[n:]


def main():
    import sklearn
    from sklearn import svm
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for p, (n, d, names, seed) in enumerate(PROBLEMS, 1):
        X16, labels, T16 = make(n, d, names, seed)
        X, T = X16.astype(np.float64), T16.astype(np.float64)
        clf = svm.LinearSVC(tol=1e-12, max_iter=5_000_000, dual=False).fit(X, labels)
        gn, g0 = so.model_gradient_norms(clf.coef_, clf.intercept_, X, labels, clf.classes_)
        s = T @ clf.coef_.T + clf.intercept_
        margin = np.abs(s[:, 0]).min() if s.shape[1] == 1 else np.diff(np.sort(s, axis=1)[:, -2:], axis=1).min()
        xnorm = np.sqrt((T * T).sum(1) + 1.0).max()
        print("problem %d: n %d d %d classes %d rows %d  max |g| %.3g (|g0| >= %.3g)  held-out margin %.3g  max |[x,1]| %.3g"
              % (p, n, d, len(names), clf.coef_.shape[0], gn.max(), g0.min(), margin, xnorm))
        assert gn.max() <= 1e-5, "problem %d: sklearn's gradient %g" % (p, gn.max())
        assert margin >= 1e-3, "problem %d: held-out margin %g" % (p, margin)
        assert np.array_equal(clf.classes_, names)
        out.update({"p%d_X" % p: X16, "p%d_labels" % p: labels.astype(np.int32), "p%d_X_test" % p: T16, "p%d_coef" % p: clf.coef_,
                    "p%d_intercept" % p: clf.intercept_, "p%d_classes" % p: clf.classes_.astype(np.int32)})
    path = os.path.join(HERE, "svm_fit_small.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
