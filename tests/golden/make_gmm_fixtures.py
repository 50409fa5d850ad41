"""sklearn-side fixtures for the GMM base clusterer (tests/test_gmm_host.py, tests/test_gpu_gmm.py),
generated ONCE on a CPU like make_sk_feature_fixtures.py's, whose row recipe and resample draw
this file shares.

Every problem is the host loop's call for resample h and K: ``GaussianMixture(n_components=K,
covariance_type='diag', n_init=n_init, random_state=seed)`` in float64 on one thread, on
``ascontiguousarray(X[idx[h]][:, cols[h]])`` with ``cols = post.feature_indices(seed, d, md, H)``
(all columns when md = d), for n_init 1 and 3.

The stability screen.  Next to sklearn the generator runs the host form (gmm.fit_from_labels on the
k-means labels sklearn's own initialisation produced) on the same rows, and once more with the
rows permuted and the columns reversed, which adds every sum in another order.  A case is KEPT
ONLY IF the three agree on the labels, n_iter, converged and the winning init of every one of its
problems; a case that does not gets another noise seed (``noise`` below), never a weaker rule.
A case is also dropped when an init with other k-means labels than the winner's comes within
2 lb_rtol of the winner's lower bound without equalling it: two inits that reach the same optimum
with their components numbered differently then differ by rounding alone, and which of them is
"strictly larger" falls to the order of the sums.  Inits with identical k-means labels compute
identical values in any implementation, and a bound that is bitwise the same under two numberings
in the host form AND in the reordered host form (well separated components: one term carries each
row's logsumexp) does not feel the order of the sums; those exact ties go to the earlier init
everywhere and are kept.
This is a condition on the inputs, checked on the CPU, so that the exact comparisons of the GPU
tests leave out no problem.  ``lb_rtol`` is 64 times the largest relative difference of the lower
bound among the three over the case, floored at 1e-13: headroom for a third order of the same sums,
the device's.  It is the only tolerance the tests use.

``tests/golden/sk/gmm_<case>.npz``: idx int32 [H, m], cols int32 [H, md], Ks, km_labels uint8
[3, nK, H, m] (each init's k-means labels), and for n_init = i in (1, 3) labels_i uint8 [nK, H, m],
n_iter_i int32, converged_i bool, lower_bound_i float64, win_i int32 (all [nK, H]), lb_rtol, meta
(JSON: the recipe, the X digest, the versions).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_gmm_fixtures.py [case ...]
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "sk")
sys.path.insert(0, ROOT)

from consensus_clustering_amd import gmm as G  # noqa: E402
from consensus_clustering_amd import post  # noqa: E402

SEED = 3
N_INITS = (1, 3)
# case: n, d, k_true, m, md, Ks, H, noise seed (0 = make_sk_fixtures._f64_noisy's rows)
CASES = {f"n96_md{md}": (96, 13, 3, 76, md, [1, 2, 3, 7, 16, 17], 3, 0) for md in (1, 3, 4, 5, 12, 13)}
CASES["n96_md3"] = CASES["n96_md3"][:-1] + (1,)  # noise 0: two inits of (h 0, K 3) within 2e-16
CASES["n300_md120"] = (300, 150, 3, 240, 120, [2, 3, 5], 3, 0)
CASES["n160_k127"] = (160, 3, 3, 130, 3, [127], 3, 0)


def digest(a) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.view(np.uint8).tobytes() + str(a.dtype).encode() + str(a.shape).encode()).hexdigest()


def rows_of(n, d, k, noise=0):
    """make_sk_fixtures._f64_noisy: blobs at seed n + d (float32, then float64) plus N(0, 0.5^2)
    noise from default_rng(noise)."""
    from sklearn.datasets import make_blobs

    X, _ = make_blobs(n_samples=n, n_features=d, centers=k, cluster_std=1.0, center_box=(-10, 10), shuffle=True,
                      random_state=n + d)
    X = X.astype(np.float32).astype(np.float64)
    X += np.random.default_rng(noise).normal(scale=0.5, size=X.shape)
    return X


def indices(n, m, seed, h):
    return np.random.RandomState(seed + h).choice(n, size=m, replace=False)


def columns(d, md, H, seed=SEED):
    if md == d:
        return np.tile(np.arange(d, dtype=np.int32), (H, 1))
    return post.feature_indices(seed, d, md, H)


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), np.finfo(np.float64).tiny)


def problem(rows, K, n_init, seed, km_labels, perm):
    """sklearn's fit, the host form and the reordered host form of one problem: (result dict,
    agree, largest relative lower-bound difference, the smallest relative distance of the winner's
    bound to that of an init with other k-means labels)."""
    from sklearn.mixture import GaussianMixture
    from threadpoolctl import threadpool_limits

    with threadpool_limits(1), warnings.catch_warnings():
        warnings.simplefilter("ignore")  # sklearn's ConvergenceWarning: converged_ records it
        sk = GaussianMixture(n_components=K, covariance_type='diag', n_init=n_init, random_state=seed).fit(rows)
        sk_labels = sk.predict(rows)
        best, win, lab = G.fit_from_labels(rows, km_labels[:n_init], K)
        rows2 = np.ascontiguousarray(rows[perm][:, ::-1])
        best2, win2, lab2 = G.fit_from_labels(rows2, [l[perm] for l in km_labels[:n_init]], K)
    agree = (np.array_equal(sk_labels, lab) and np.array_equal(lab[perm], lab2)
             and sk.n_iter_ == best["n_iter"] == best2["n_iter"]
             and bool(sk.converged_) == best["converged"] == best2["converged"] and win == win2)
    lbs = (float(sk.lower_bound_), best["lower_bound"], best2["lower_bound"])
    rel = max(_rel(lbs[0], lbs[1]), _rel(lbs[0], lbs[2]), _rel(lbs[1], lbs[2]))
    margin = np.inf
    for j in range(n_init):
        if j != win and not np.array_equal(km_labels[j], km_labels[win]):
            a = _rel(G.em(rows, km_labels[j], K, 1e-3, 1e-6, 100)["lower_bound"], lbs[1])
            b = _rel(G.em(rows2, km_labels[j][perm], K, 1e-3, 1e-6, 100)["lower_bound"], lbs[2])
            if a == 0.0 and b == 0.0:
                continue  # an exact tie under both orders of the sums
            margin = min(margin, a if a > 0.0 else np.finfo(np.float64).tiny, b if b > 0.0 else np.finfo(np.float64).tiny)
    return dict(labels=sk_labels, n_iter=int(sk.n_iter_), converged=bool(sk.converged_), lower_bound=lbs[0],
                win=win), agree, rel, margin


def kmeans_labels(rows, K, seed):
    """The labels of the three KMeans(n_init=1) fits a 3-init mixture draws from one RandomState."""
    from sklearn.cluster import KMeans
    from sklearn.utils import check_random_state
    from threadpoolctl import threadpool_limits

    rs = check_random_state(seed)
    with threadpool_limits(1):
        return [KMeans(n_clusters=K, n_init=1, random_state=rs).fit(rows).labels_ for _ in range(max(N_INITS))]


def make(case):
    import scipy
    import sklearn

    n, d, k_true, m, md, Ks, H, noise = CASES[case]
    X = rows_of(n, d, k_true, noise)
    idx = np.stack([indices(n, m, SEED, h) for h in range(H)]).astype(np.int32)
    cols = columns(d, md, H)
    nK = len(Ks)
    km = np.zeros((max(N_INITS), nK, H, m), dtype=np.uint8)
    out = {i: dict(labels=np.zeros((nK, H, m), dtype=np.uint8), n_iter=np.zeros((nK, H), dtype=np.int32),
                   converged=np.zeros((nK, H), dtype=bool), lower_bound=np.zeros((nK, H)),
                   win=np.zeros((nK, H), dtype=np.int32)) for i in N_INITS}
    worst, unstable, margins = 0.0, [], []
    t0 = time.time()
    for h in range(H):
        rows = np.ascontiguousarray(X[idx[h]][:, cols[h]])
        perm = np.random.default_rng(1000 + h).permutation(m)
        for k, K in enumerate(Ks):
            km[:, k, h] = kmeans_labels(rows, K, SEED)
            for i in N_INITS:
                res, agree, rel, margin = problem(rows, K, i, SEED, list(km[:, k, h].astype(np.int64)), perm)
                worst = max(worst, rel)
                margins.append((margin, (h, K, i)))
                if not agree:
                    unstable.append((h, K, i))
                for key, v in res.items():
                    out[i][key][k, h] = v
    lb_rtol = max(64 * worst, 1e-13)
    unstable += [("init margin", margin) + at for margin, at in margins if margin <= 2 * lb_rtol]
    if unstable:
        raise SystemExit(f"gmm_{case}: NOT KEPT, sklearn, the host form and the reordered host form disagree on "
                         f"(h, K, n_init) {unstable}: give the case another noise seed")
    meta = dict(kind="gmm", case=case, n=n, d=d, k_true=k_true, m=m, md=md, Ks=Ks, seed=SEED, H=H, noise=noise,
                n_inits=list(N_INITS), x_sha256=digest(X), lb_rel_seen=worst,
                init_margin_seen=min(m for m, _ in margins), threads=1, sklearn=sklearn.__version__,
                numpy=np.__version__, scipy=scipy.__version__,
                note="make_sk_fixtures._f64_noisy rows (noise seed = noise); sklearn GaussianMixture('diag') float64, "
                     "1 thread, on ascontiguousarray(X[idx[h]][:, cols[h]]); kept only because sklearn, gmm.py and "
                     "gmm.py on permuted rows / reversed columns agree on every problem")
    arrays = dict(idx=idx, cols=cols.astype(np.int32), Ks=np.asarray(Ks, dtype=np.int32), km_labels=km,
                  lb_rtol=np.float64(lb_rtol), meta=np.array(json.dumps(meta)))
    for i in N_INITS:
        for key, v in out[i].items():
            arrays[f"{key}_{i}"] = v
    np.savez_compressed(os.path.join(OUT, f"gmm_{case}.npz"), **arrays)
    print(f"gmm_{case}: {nK * H * len(N_INITS)} problems ({time.time() - t0:.0f} s); n_iter "
          f"{min(o['n_iter'].min() for o in out.values())}..{max(o['n_iter'].max() for o in out.values())}, "
          f"lower bound within {worst:.2e}, lb_rtol {lb_rtol:.2e}", flush=True)


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    os.makedirs(OUT, exist_ok=True)
    for c in sys.argv[1:] or list(CASES):
        make(c)
