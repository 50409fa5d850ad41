"""NMF (non-negative matrix factorisation by multiplicative updates): the base clusterer of
"consensus NMF" (Brunet et al., PNAS 2004), as an estimator to pass to ``ConsensusClustering``.

``NMF`` restates sklearn's ``NMF(init='random', solver='mu', beta_loss='frobenius')`` with all
regularisation 0 in float64, operation by operation (sklearn/decomposition/_nmf.py, sklearn 1.7:
_initialize_nmf, _fit_multiplicative_update, _multiplicative_update_w, _multiplicative_update_h and
_beta_divergence): stated in DESIGN.md K14.  An estimator of exactly this type runs on the device
inside ``ConsensusClustering.fit`` (csrc/nmf.hip, ``backend_ == 'gpu-nmf'``); its own ``fit`` is
the host form of the same algorithm in numpy, the same numpy calls sklearn makes, so at
``n_init=1`` W, H and n_iter equal sklearn's bitwise.  The module imports neither torch nor the
engine, so a host worker process (_hostfit) and the oracle can use the estimator with numpy alone.

All arithmetic is float64: X is cast to float64 whatever its dtype.
"""
from __future__ import annotations

import numpy as np

from .gmm import _float_param, _int_param
from .pam import refuse_not_finite

NEGATIVE = "Negative values in data passed to NMF (input X)."
EPS = float(np.finfo(np.float32).eps)  # sklearn's EPSILON: what a zero denominator becomes


def init_normals(rs, m, d, K):
    """|N| for H [K, d], drawn first, then for W [m, K], from the RandomState rs: _initialize_nmf's
    draws for init='random' without the factor avg."""
    H = np.abs(rs.standard_normal(size=(K, d)))
    W = np.abs(rs.standard_normal(size=(m, K)))
    return W, H


def error(X, W, H):
    """sqrt(squared_norm(X - W H)): _beta_divergence(X, W, H, 2, square_root=True), whose halving
    and doubling are exact."""
    diff = (X - np.dot(W, H)).ravel()
    return np.sqrt(np.dot(diff, diff))  # a numpy scalar: 0 / 0 in the stopping test is NaN, not an exception


def update_w(X, W, H):
    """W *= (X H^T) / (W (H H^T)), a zero denominator replaced by EPS: a division, then a
    multiplication."""
    numerator = np.dot(X, H.T)
    denominator = np.dot(W, np.dot(H, H.T))
    denominator[denominator == 0] = EPS
    numerator /= denominator
    W *= numerator
    return W


def update_h(X, W, H):
    """H *= (W^T X) / multi_dot([W^T, W, H]), a zero denominator replaced by EPS."""
    numerator = np.dot(W.T, X)
    denominator = np.linalg.multi_dot([W.T, W, H])
    denominator[denominator == 0] = EPS
    numerator /= denominator
    H *= numerator
    return H


def mu(X, W, H, tol, max_iter):
    """_fit_multiplicative_update from W, H (updated in place): dict(W, H, reconstruction_err,
    n_iter, converged).  The stopping test runs at every iteration that is a multiple of 10 when
    tol > 0; a NaN ratio (X identically 0) compares false."""
    error_at_init = error(X, W, H)
    previous_error = error_at_init
    converged, n_iter = False, 0
    for n_iter in range(1, max_iter + 1):
        update_w(X, W, H)
        update_h(X, W, H)
        if tol > 0 and n_iter % 10 == 0:
            err = error(X, W, H)
            with np.errstate(invalid="ignore", divide="ignore"):
                if (previous_error - err) / error_at_init < tol:
                    converged = True
                    break
            previous_error = err
    return dict(W=W, H=H, reconstruction_err=float(error(X, W, H)), n_iter=n_iter, converged=converged,
                error_at_init=float(error_at_init))


def labels_of(W, H):
    """argmax_k W[i, k] * sqrt(sum_j H[k, j]^2), the first index on ties."""
    return np.argmax(W * np.sqrt(np.diag(np.dot(H, H.T))), axis=1)


def fit_from_normals(X, normals, K, tol=1e-4, max_iter=200):
    """The fit from each init's (|N_W| [m, K], |N_H| [K, d]): (best run, winning init, labels, every
    init's run).  The strictly smallest reconstruction error wins and the first init always counts."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    avg = np.sqrt(X.mean() / K)
    best, win, runs = None, 0, []
    for i, (NW, NH) in enumerate(normals):
        run = mu(X, np.abs(avg * NW), np.abs(avg * NH), tol, max_iter)
        runs.append(run)
        if best is None or run["reconstruction_err"] < best["reconstruction_err"]:
            best, win = run, i
    return best, win, labels_of(best["W"], best["H"]), runs


def check_params(p):
    """The refusals of the parameter dict p, in sklearn's wording."""
    _int_param("n_components", p["n_components"], 1, "NMF")
    _int_param("max_iter", p["max_iter"], 1, "NMF")
    _int_param("n_init", p["n_init"], 1, "NMF")
    _float_param("tol", p["tol"], "NMF")


def validate(X):
    """NMF's refusals from host values: X that is not finite, and a negative entry."""
    X = np.asarray(X)
    refuse_not_finite(X)
    if X.size and X.min() < 0:
        raise ValueError(NEGATIVE)


class NMF:
    """Non-negative matrix factorisation X ~ W H by multiplicative updates under the Frobenius loss
    from a random initialisation: sklearn's ``NMF(init='random', solver='mu')`` in float64.

    Parameters: ``n_components``, ``tol``, ``max_iter`` (at least 1), ``n_init`` (restarts that
    continue one RandomState stream; ``n_init=1`` is sklearn's fit), ``random_state``.

    The label of row i is ``argmax_k W[i, k] * sqrt(sum_j H[k, j]**2)``, the first index on ties:
    the factor, the norm of component k's row of H, makes the label independent of the arbitrary
    scale between a column of W and its row of H (Xu, Liu & Gong 2003).  It is not
    ``W.argmax(1)``.

    After ``fit``: ``labels_``, ``W_`` (what ``fit_transform`` returns), ``components_`` (H),
    ``reconstruction_err_``, ``n_iter_``, ``converged_`` (the stopping test ended the fit) and
    ``best_init_`` (the init with the strictly smallest error; the first always counts)."""

    def __init__(self, n_components=1, tol=1e-4, max_iter=200, n_init=1, random_state=None):
        self.n_components = n_components
        self.tol = tol
        self.max_iter = max_iter
        self.n_init = n_init
        self.random_state = random_state

    def get_params(self, deep=True):
        return dict(n_components=self.n_components, tol=self.tol, max_iter=self.max_iter, n_init=self.n_init,
                    random_state=self.random_state)

    def set_params(self, **params):
        valid = self.get_params()
        for key, value in params.items():
            if key not in valid:
                raise ValueError(f"Invalid parameter {key!r} for estimator {type(self).__name__}(). "
                                 f"Valid parameters are: {sorted(valid)!r}.")
            setattr(self, key, value)
        return self

    def __repr__(self):
        return f"{type(self).__name__}(" + ", ".join(f"{k}={v!r}" for k, v in self.get_params().items()) + ")"

    def fit(self, X, y=None):
        from sklearn.utils import check_random_state

        p = self.get_params()
        check_params(p)
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError(f"Expected 2D array, got {X.ndim}D array instead.")
        if X.dtype.kind == 'f':
            refuse_not_finite(X)  # in X's own dtype, as check_array words it
        X = np.ascontiguousarray(X, dtype=np.float64)
        validate(X)
        K = int(p["n_components"])
        rs = check_random_state(p["random_state"])
        m, d = X.shape
        normals = [init_normals(rs, m, d, K) for _ in range(int(p["n_init"]))]
        best, self.best_init_, self.labels_, _ = fit_from_normals(X, normals, K, float(p["tol"]), int(p["max_iter"]))
        self.W_, self.components_ = best["W"], best["H"]
        self.reconstruction_err_, self.n_iter_ = best["reconstruction_err"], best["n_iter"]
        self.converged_ = best["converged"]
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def fit_transform(self, X, y=None):
        return self.fit(X).W_
