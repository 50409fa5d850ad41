"""PAM (partitioning around medoids, k-medoids): the third clustering algorithm of
ConsensusClusterPlus next to ``hc`` and ``km``, as an estimator to pass to ``ConsensusClustering``.

``PAM`` clusters from a dissimilarity matrix alone: Kaufman & Rousseeuw's BUILD and SWAP (R's
``pam`` with ``pamonce = 0``), stated in DESIGN.md K11.  An estimator of exactly this type runs
on the device inside ``ConsensusClustering.fit`` (csrc/pam.hip, ``backend_ == 'gpu-pam'``); its own
``fit`` is the host form of the same algorithm in numpy, over ``scipy.spatial.distance.pdist``.
The module imports neither torch nor the engine, so a host worker process (_hostfit) and the
oracle can use the estimator with numpy and scipy alone.

All arithmetic is float64.  A decision compares sums of m terms, so this form and the device's,
which add in another order, can decide differently only where the margin is below about
m * 2^-52 of the sums; on integer-valued distances every sum is exact and the tie rules decide.
"""
from __future__ import annotations

import numpy as np

# sklearn's metric spellings -> scipy's pdist names (the device trees accept the same)
METRICS = dict(euclidean='euclidean', l2='euclidean', manhattan='cityblock', l1='cityblock',
               cityblock='cityblock', cosine='cosine', correlation='correlation')

_ROWS = 1024  # candidate rows per block of the SWAP evaluation (bounds its m x m temporaries)


def degenerate_rows(X, metric):
    """Why pdist(X, metric) has a row without distances, or None, from the host array X: an
    all-zero row under cosine (sklearn's own refusal, in its words) and a constant row under
    correlation (it centres to zero, so its distances are 0 / 0)."""
    if metric == "cosine":
        if np.any(~np.any(X, axis=1)):
            return "Cosine affinity cannot be used when X contains zero vectors"
    elif metric == "correlation":
        const = np.flatnonzero((X == X[:, :1]).all(axis=1))
        if const.size:
            return (f"the correlation metric cannot be used when X contains constant rows (row {int(const[0])} "
                    "is constant: its correlation distances are undefined)")
    return None


def build(D, K):
    """The BUILD chain: K medoid items in the order they are chosen.  Medoid 0 is the first index
    of the smallest row sum; every further one the first index of the largest gain
    sum_j max(near[j] - D[i, j], 0) over the non-medoids.  Greedy: build(D, K)[:k] == build(D, k)."""
    m = D.shape[0]
    first = int(np.argmin(D.sum(axis=1)))
    chain, near = [first], D[first].copy()
    is_medoid = np.zeros(m, dtype=bool)
    is_medoid[first] = True
    for _ in range(1, K):
        gain = np.maximum(near[None, :] - D, 0.0).sum(axis=1)
        gain[is_medoid] = -np.inf
        i = int(np.argmax(gain))
        chain.append(i)
        is_medoid[i] = True
        near = np.minimum(near, D[i])
    return chain


def _nearest(D, med):
    """near, second and the nearest slot of every item for the medoid items med (in slot order).
    A medoid takes its own slot, whatever else lies at distance 0."""
    Dm = D[med]  # [K, m]
    K, m = Dm.shape
    slot = np.argmin(Dm, axis=0)
    slot[med] = np.arange(K)
    cols = np.arange(m)
    near = Dm[slot, cols]
    if K > 1:
        rest = Dm.copy()
        rest[slot, cols] = np.inf
        second = rest.min(axis=0)
    else:
        second = np.full(m, np.inf)
    return near, second, slot


def swap(D, med, max_iter):
    """SWAP from the medoid items med (slot order; changed in place): (med, swaps made).  Each
    iteration takes the pair (medoid i, non-medoid h) of the smallest dTD, a tie to the lowest h,
    then to the medoid with the lowest item index, and swaps when dTD < 0.  FastPAM1's one pass
    per h: dTD(i, h) = shared(h) + corr(h, i) with shared(h) = sum_j min(D[h, j] - near[j], 0) and
    corr(h, i) = sum over the j nearest to i of (min(D[h, j], second[j]) - near[j]) -
    min(D[h, j] - near[j], 0).  The medoid of an h is chosen by its corr, as the device does, which
    is the choice by dTD except where adding shared(h) rounds two different corr to one sum."""
    m = D.shape[0]
    K = len(med)
    n_iter = 0
    while n_iter < max_iter:
        near, second, slot = _nearest(D, med)
        onehot = np.zeros((m, K))
        onehot[np.arange(m), slot] = 1.0
        by_item = np.argsort(med)  # slots by ascending medoid item index: the tie rule
        delta = np.empty(m)
        which = np.empty(m, dtype=np.int64)
        for a in range(0, m, _ROWS):
            Dh = D[a:a + _ROWS]
            s0 = np.minimum(Dh - near, 0.0)
            corr = (((np.minimum(Dh, second) - near) - s0) @ onehot)[:, by_item]
            c = np.argmin(corr, axis=1)  # the first of the smallest: the lowest medoid item index
            which[a:a + _ROWS] = by_item[c]
            delta[a:a + _ROWS] = s0.sum(axis=1) + corr[np.arange(len(c)), c]
        delta[med] = np.inf  # a medoid is no candidate
        h = int(np.argmin(delta))  # the first of the smallest: the lowest h
        i = int(which[h])
        if not delta[h] < 0.0:
            break
        med[i] = h
        n_iter += 1
    return med, n_iter


def assign(D, med):
    """(medoid items ascending, labels, inertia): item j gets the rank, by ascending item index,
    of its nearest medoid (a tie goes to the lowest item index; a medoid labels itself)."""
    med = np.sort(np.asarray(med))
    near, _, labels = _nearest(D, med)  # argmin's first index = the lowest item index
    return med, labels.astype(np.int64), float(near.sum())


def pam(D, K, max_iter=300):
    """PAM on the symmetric float64 dissimilarities D [m, m] with a zero diagonal:
    (medoid_indices ascending, labels, inertia, n_iter)."""
    D = np.ascontiguousarray(D, dtype=np.float64)
    med, n_iter = swap(D, build(D, K), max_iter)
    return assign(D, med) + (n_iter,)


class PAM:
    """k-medoids by PAM (BUILD, then SWAP until no swap lowers the total deviation).

    Parameters: ``n_clusters``; ``metric``: 'euclidean' ('l2'), 'manhattan' ('l1', 'cityblock'),
    'cosine' or 'correlation', computed by scipy's ``pdist``; ``max_iter``: the most swaps made
    (0 = BUILD only).  PAM is deterministic, so there is no ``random_state``.

    After ``fit``: ``labels_`` (the rank of the nearest medoid by ascending item index),
    ``medoid_indices_`` (ascending), ``inertia_`` (the total deviation) and ``n_iter_`` (swaps)."""

    def __init__(self, n_clusters=8, metric='euclidean', max_iter=300):
        self.n_clusters = n_clusters
        self.metric = metric
        self.max_iter = max_iter

    def get_params(self, deep=True):
        return dict(n_clusters=self.n_clusters, metric=self.metric, max_iter=self.max_iter)

    def set_params(self, **params):
        valid = self.get_params()
        for key, value in params.items():
            if key not in valid:
                raise ValueError(f"Invalid parameter {key!r} for estimator {type(self).__name__}(). "
                                 f"Valid parameters are: {sorted(valid)!r}.")
            setattr(self, key, value)
        return self

    def __repr__(self):
        return f"{type(self).__name__}(n_clusters={self.n_clusters!r}, metric={self.metric!r}, " \
               f"max_iter={self.max_iter!r})"

    def fit(self, X, y=None):
        from scipy.spatial.distance import pdist, squareform

        K, max_iter = self.n_clusters, self.max_iter
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
            raise ValueError(f"The 'n_clusters' parameter of PAM must be an int in the range [1, inf). Got {K!r} "
                             "instead.")
        if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
            raise ValueError(f"The 'max_iter' parameter of PAM must be an int in the range [0, inf). Got "
                             f"{max_iter!r} instead.")
        if not isinstance(self.metric, str) or self.metric not in METRICS:
            raise ValueError(f"The 'metric' parameter of PAM must be a str among {sorted(METRICS)!r}. Got "
                             f"{self.metric!r} instead.")
        metric = METRICS[self.metric]
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError(f"Expected 2D array, got {X.ndim}D array instead.")
        if X.dtype.kind != 'f':
            X = X.astype(np.float64)
        validate(X, X.shape[0], [K])
        why = degenerate_rows(X, metric)
        if why is not None:
            raise ValueError(why)
        D = squareform(pdist(X, metric))
        if not np.isfinite(D).all():
            raise ValueError(f"the {metric} distances between the rows of X are not all finite")
        self.medoid_indices_, self.labels_, self.inertia_, self.n_iter_ = pam(D, int(K), int(max_iter))
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_


def refuse_not_finite(X):
    """check_array's refusal of a float array that holds a NaN or an infinity, in its words."""
    if X.dtype.kind == 'f' and not np.isfinite(X).all():
        if np.isnan(X).any():
            raise ValueError("Input X contains NaN.")
        raise ValueError(f"Input X contains infinity or a value too large for dtype('{X.dtype}').")


def validate(X, m, Ks):
    """PAM's refusals from host values: X that is not finite (X None = checked elsewhere), fewer
    than 2 samples, and a K above the number of samples."""
    d = 0
    if X is not None:
        X = np.asarray(X)
        refuse_not_finite(X)
        d = X.shape[1] if X.ndim == 2 else 0
    if m < 2:
        raise ValueError(f"Found array with {m} sample(s) (shape=({m}, {d})) while a minimum of 2 is "
                         "required by PAM.")
    for K in Ks:
        if K > m:
            raise ValueError(f"Cannot extract more clusters than samples: {K} clusters were given for {m} samples.")
