"""GMM and FullGMM (Gaussian mixtures with diagonal and with full covariances, fitted by EM): the
second base clusterer of the reference's own demonstration next to KMeans, as estimators to pass to
``ConsensusClustering``.

``GMM`` restates sklearn's ``GaussianMixture(covariance_type='diag', init_params='kmeans')`` in
float64, operation by operation (sklearn/mixture/_gaussian_mixture.py and _base.py, sklearn 1.7):
stated in DESIGN.md K12.  An estimator of exactly this type runs on the device inside
``ConsensusClustering.fit`` (csrc/gmm.hip, ``backend_ == 'gpu-gmm'``); its own ``fit`` is the host
form of the same algorithm in numpy, with sklearn's ``KMeans`` for the initialisation and scipy's
``logsumexp``.  The module imports neither torch nor the engine, so a host worker process (_hostfit)
and the oracle can use the estimator with numpy, scipy and sklearn alone.

All arithmetic is float64: X is cast to float64 whatever its dtype (sklearn computes float32 input
in float32).  The sums of an E- or M-step run over md or m terms, so this form and the device's,
which add in another order, agree on the lower bound to about m * 2^-52 relative and decide alike
(converged or not, which init wins, which component a row goes to) except where a margin is
that small.

``FullGMM`` is the same for ``covariance_type='full'`` (sklearn's default, the model the reference
demonstrates): the weighted covariance of every component, its Cholesky factor, the triangular
inverse as the precision factor and ``(x - mu) P`` in the E-step (csrc/gmm_full.hip).
It is a type of its own: ``GMM`` keeps refusing every ``covariance_type`` but 'diag'.
"""
from __future__ import annotations

import numpy as np

from .pam import refuse_not_finite

_ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical "
                "covariance (for instance caused by singleton or collapsed samples). Try to decrease the "
                "number of components, increase reg_covar, or scale the input data.")


def m_step(X, resp, reg_covar):
    """_estimate_gaussian_parameters for 'diag': (nk, means, covariances) of the responsibilities
    resp [m, K]; raises sklearn's ValueError when a variance is not positive."""
    nk = resp.sum(axis=0) + 10 * np.finfo(np.float64).eps
    means = np.dot(resp.T, X) / nk[:, np.newaxis]
    avg_X2 = np.dot(resp.T, X * X) / nk[:, np.newaxis]
    covariances = avg_X2 - means**2 + reg_covar
    if np.any(np.less_equal(covariances, 0.0)):
        raise ValueError(_ILL_DEFINED)
    return nk, means, covariances


def e_step(X, weights, means, covariances):
    """(mean of the row log-norms, log responsibilities [m, K]) under the parameters: sklearn's
    _estimate_log_gaussian_prob for 'diag' plus the log weights, and scipy's logsumexp."""
    from scipy.special import logsumexp

    d = X.shape[1]
    pchol = 1.0 / np.sqrt(covariances)
    log_det = np.sum(np.log(pchol), axis=1)
    prec = pchol**2
    log_prob = np.sum((means**2 * prec), 1) - 2.0 * np.dot(X, (means * prec).T) + np.dot(X**2, prec.T)
    weighted = (-0.5 * (d * np.log(2 * np.pi) + log_prob) + log_det) + np.log(weights)
    norm = logsumexp(weighted, axis=1)
    with np.errstate(under="ignore"):
        log_resp = weighted - norm[:, np.newaxis]
    return np.mean(norm), log_resp


def m_step_full(X, resp, reg_covar):
    """_estimate_gaussian_parameters for 'full' and _compute_precision_cholesky: (nk, means,
    (covariances [K, d, d], precision factors [K, d, d])).  Component k's covariance is
    dot(resp[:, k] * diff.T, diff) / nk[k] with diff = X - means[k] and reg_covar on the diagonal;
    its precision factor is the transposed inverse of the lower Cholesky factor.  A covariance that
    LAPACK finds not positive definite raises sklearn's ValueError."""
    from scipy import linalg

    nk = resp.sum(axis=0) + 10 * np.finfo(np.float64).eps
    means = np.dot(resp.T, X) / nk[:, np.newaxis]
    K, d = means.shape
    covariances = np.empty((K, d, d))
    pchol = np.empty((K, d, d))
    for k in range(K):
        diff = X - means[k]
        covariances[k] = np.dot(resp[:, k] * diff.T, diff) / nk[k]
        covariances[k].flat[:: d + 1] += reg_covar
        try:
            cov_chol = linalg.cholesky(covariances[k], lower=True)
        except linalg.LinAlgError:
            raise ValueError(_ILL_DEFINED)
        pchol[k] = linalg.solve_triangular(cov_chol, np.eye(d), lower=True).T
    return nk, means, (covariances, pchol)


def e_step_full(X, weights, means, cov):
    """e_step for 'full': cov is m_step_full's pair, of which the precision factors P are read.
    _estimate_log_gaussian_prob: sum(square(dot(X, P_k) - dot(mu_k, P_k)), 1), the log determinant
    from the diagonal of P_k."""
    from scipy.special import logsumexp

    d = X.shape[1]
    pchol = cov[1]
    K = means.shape[0]
    log_det = np.sum(np.log(pchol.reshape(K, -1)[:, :: d + 1]), axis=1)
    log_prob = np.empty((X.shape[0], K))
    for k in range(K):
        y = np.dot(X, pchol[k]) - np.dot(means[k], pchol[k])
        log_prob[:, k] = np.sum(np.square(y), axis=1)
    weighted = (-0.5 * (d * np.log(2 * np.pi) + log_prob) + log_det) + np.log(weights)
    norm = logsumexp(weighted, axis=1)
    with np.errstate(under="ignore"):
        log_resp = weighted - norm[:, np.newaxis]
    return np.mean(norm), log_resp


_STEPS = {'diag': (m_step, e_step), 'full': (m_step_full, e_step_full)}


def em(X, labels, K, tol, reg_covar, max_iter, covariance_type='diag'):
    """One init from the k-means labels: dict(weights, means, covariances, lower_bound, n_iter,
    converged), under 'full' also precisions_cholesky.  _initialize on the one-hot
    responsibilities, then E-step, M-step and the test abs(lower bound - previous) < tol, at most
    max_iter times."""
    m_step, e_step = _STEPS[covariance_type]
    m = X.shape[0]
    resp = np.zeros((m, K))
    resp[np.arange(m), labels] = 1
    weights, means, cov = m_step(X, resp, reg_covar)
    weights = weights / m
    lower, converged, n_iter = -np.inf, False, 0
    for n_iter in range(1, max_iter + 1):
        prev = lower
        lower, log_resp = e_step(X, weights, means, cov)
        weights, means, cov = m_step(X, np.exp(log_resp), reg_covar)
        weights = weights / weights.sum()
        if abs(lower - prev) < tol:
            converged = True
            break
    run = dict(weights=weights, means=means, covariances=cov, lower_bound=float(lower), n_iter=n_iter,
               converged=converged)
    if covariance_type == 'full':
        run["covariances"], run["precisions_cholesky"] = cov
    return run


def final_labels(X, run, covariance_type='diag'):
    """The argmax (first index) of a final E-step under the parameters of em's result."""
    cov = run["covariances"]
    if covariance_type == 'full':
        cov = (cov, run["precisions_cholesky"])
    _, log_resp = _STEPS[covariance_type][1](X, run["weights"], run["means"], cov)
    return log_resp.argmax(axis=1)


def fit_from_labels(X, init_labels, K, tol=1e-3, reg_covar=1e-6, max_iter=100, covariance_type='diag'):
    """The fit from each init's k-means labels (a sequence of int arrays [m]): (best, winning
    init, labels).  A strictly larger lower bound wins and the first init always counts; the
    labels are the argmax (first index) of a final E-step under the winning parameters."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    best, win, top = None, 0, -np.inf
    for i, lab in enumerate(init_labels):
        run = em(X, np.asarray(lab), K, tol, reg_covar, max_iter, covariance_type)
        if run["lower_bound"] > top or top == -np.inf:
            best, win, top = run, i, run["lower_bound"]
    return best, win, final_labels(X, best, covariance_type)


def _int_param(name, v, lo, who="GMM"):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo:
        raise ValueError(f"The {name!r} parameter of {who} must be an int in the range [{lo}, inf). Got {v!r} instead.")


def _float_param(name, v, who="GMM"):
    ok = not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))
    if not ok or not v >= 0:
        raise ValueError(f"The {name!r} parameter of {who} must be a float in the range [0.0, inf). Got {v!r} instead.")


def check_params(p, who="GMM"):
    """The refusals of the parameter dict p, in sklearn's wording (FullGMM's has no
    covariance_type)."""
    if p.get("covariance_type", 'diag') != 'diag':
        raise ValueError(f"GMM fits diagonal covariances only (covariance_type='diag'), got "
                         f"{p['covariance_type']!r}; sklearn's GaussianMixture fits the other types (on the host)")
    _int_param("n_components", p["n_components"], 1, who)
    _int_param("max_iter", p["max_iter"], 1, who)
    _int_param("n_init", p["n_init"], 1, who)
    _float_param("tol", p["tol"], who)
    _float_param("reg_covar", p["reg_covar"], who)


def validate(X, m, Ks, who="GMM"):
    """GMM's refusals from host values: X that is not finite (X None = checked elsewhere), fewer
    than 2 samples, and a K above the number of samples."""
    d = 0
    if X is not None:
        X = np.asarray(X)
        refuse_not_finite(X)
        d = X.shape[1] if X.ndim == 2 else 0
    if m < 2:
        raise ValueError(f"Found array with {m} sample(s) (shape=({m}, {d})) while a minimum of 2 is "
                         f"required by {who}.")
    for K in Ks:
        if K > m:
            raise ValueError(f"Expected n_samples >= n_components but got n_components = {K}, n_samples = {m}")


def _fit(est, X, covariance_type, who):
    """``fit`` of GMM ('diag') and FullGMM ('full'): the refusals in the estimator's name `who`, one
    KMeans(n_init=1) fit per init from one RandomState, em from its labels, the strictly largest
    bound (the first init always counts), the attributes and the labels of a final E-step."""
    from sklearn.cluster import KMeans
    from sklearn.utils import check_random_state

    p = est.get_params()
    check_params(p, who)
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"Expected 2D array, got {X.ndim}D array instead.")
    if X.dtype.kind == 'f':
        refuse_not_finite(X)  # in X's own dtype, as check_array words it
    X = np.ascontiguousarray(X, dtype=np.float64)
    K = int(p["n_components"])
    validate(X, X.shape[0], [K], who)
    rs = check_random_state(p["random_state"])
    tol, reg, max_iter = float(p["tol"]), float(p["reg_covar"]), int(p["max_iter"])
    best, top, inits = None, -np.inf, []
    for i in range(int(p["n_init"])):
        inits.append(KMeans(n_clusters=K, n_init=1, random_state=rs).fit(X).labels_)
        run = em(X, inits[-1], K, tol, reg, max_iter, covariance_type)
        if run["lower_bound"] > top or top == -np.inf:
            best, top, est.best_init_ = run, run["lower_bound"], i
    est.init_labels_ = inits
    est.weights_, est.means_, est.covariances_ = best["weights"], best["means"], best["covariances"]
    if covariance_type == 'full':
        est.precisions_cholesky_ = best["precisions_cholesky"]
    est.lower_bound_, est.n_iter_, est.converged_ = best["lower_bound"], best["n_iter"], best["converged"]
    est.labels_ = final_labels(X, best, covariance_type)
    return est


class GMM:
    """Gaussian mixture with diagonal covariances by EM from a k-means initialisation.

    Parameters as sklearn's ``GaussianMixture``: ``n_components``, ``covariance_type`` ('diag'
    only), ``tol``, ``reg_covar``, ``max_iter`` (at least 1), ``n_init``, ``random_state``.

    After ``fit``: ``labels_``, ``weights_``, ``means_``, ``covariances_``, ``lower_bound_``,
    ``n_iter_``, ``converged_`` (no warning when the best init did not converge), and
    ``init_labels_`` (each init's k-means labels) with ``best_init_``."""

    def __init__(self, n_components=1, covariance_type='diag', tol=1e-3, reg_covar=1e-6, max_iter=100,
                 n_init=1, random_state=None):
        self.n_components = n_components
        self.covariance_type = covariance_type
        self.tol = tol
        self.reg_covar = reg_covar
        self.max_iter = max_iter
        self.n_init = n_init
        self.random_state = random_state

    def get_params(self, deep=True):
        return dict(n_components=self.n_components, covariance_type=self.covariance_type, tol=self.tol,
                    reg_covar=self.reg_covar, max_iter=self.max_iter, n_init=self.n_init,
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
        return _fit(self, X, 'diag', "GMM")

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_


class FullGMM:
    """Gaussian mixture with full covariances by EM from a k-means initialisation: sklearn's
    ``GaussianMixture(covariance_type='full', init_params='kmeans')`` in float64.

    Parameters: ``n_components``, ``tol``, ``reg_covar``, ``max_iter`` (at least 1), ``n_init``,
    ``random_state``.  ``covariance_type`` is the read-only 'full'.

    After ``fit``: as ``GMM``, with ``covariances_`` [K, d, d] and ``precisions_cholesky_``
    [K, d, d] (upper triangular: the transposed inverse of each covariance's Cholesky factor)."""

    covariance_type = 'full'

    def __init__(self, n_components=1, tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, random_state=None):
        self.n_components = n_components
        self.tol = tol
        self.reg_covar = reg_covar
        self.max_iter = max_iter
        self.n_init = n_init
        self.random_state = random_state

    def get_params(self, deep=True):
        return dict(n_components=self.n_components, tol=self.tol, reg_covar=self.reg_covar, max_iter=self.max_iter,
                    n_init=self.n_init, random_state=self.random_state)

    set_params = GMM.set_params
    __repr__ = GMM.__repr__

    def fit(self, X, y=None):
        return _fit(self, X, 'full', "FullGMM")

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_
