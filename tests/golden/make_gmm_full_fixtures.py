"""sklearn-side fixtures for the full-covariance GMM base clusterer (tests/test_gmm_full_host.py,
tests/test_gpu_gmm_full.py), generated ONCE on a CPU.  The rows recipe, the resample draw, the
column draw and the stability screen are make_gmm_fixtures.py's; only the model differs.

Every problem is the host loop's call for resample h and K: ``GaussianMixture(n_components=K,
covariance_type='full', n_init=n_init, random_state=seed)`` in float64 on one thread, on
``ascontiguousarray(X[idx[h]][:, cols[h]])`` with ``cols = post.feature_indices(seed, d, md, H)``
(all columns when md = d), for n_init 1 and 3.

The stability screen.  Next to sklearn the generator runs the host form (gmm.fit_from_labels with
covariance_type='full' on the k-means labels sklearn's own initialisation produced) on the same
rows, and once more with the rows permuted and the columns reversed, which adds every sum in
another order and factors every covariance from its other corner.  A case is KEPT ONLY IF the
three agree on the labels, n_iter, converged and the winning init of every one of its problems; a
case that does not gets another noise seed, never a weaker rule.  A case is also dropped when an
init with other k-means labels than the winner's comes within 2 lb_rtol of the winner's lower
bound without equalling it under both orders (make_gmm_fixtures.py states why).  ``lb_rtol`` is 64
times the largest relative difference of the lower bound among the three over the case, floored at
1e-13.  It is the only tolerance the tests use.

The cases sit on the kernels' edges: md 1, 3, 4, 5 (partial steps of 4 of the matrix-core chains),
15, 16, 17 (one and two 16-wide tiles), 33 (three tile rows, six triangle tiles), K = 17 and 20
(the second component tile) and md = 128 (the limit, the largest staged factor).

``tests/golden/sk/fullgmm_<case>.npz``: the arrays of gmm_<case>.npz (idx, cols, Ks, km_labels,
labels_i, n_iter_i, converged_i, lower_bound_i, win_i, lb_rtol, meta).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_gmm_full_fixtures.py [case ...]
"""
from __future__ import annotations

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
sys.path.insert(0, HERE)

from make_gmm_fixtures import N_INITS, SEED, _rel, columns, digest, indices, kmeans_labels, rows_of  # noqa: E402

from consensus_clustering_amd import gmm as G  # noqa: E402

# case: n, d, k_true, m, md, Ks, H, noise seed
CASES = {f"n200_md{md}": (200, 17, 3, 160, md, [1, 2, 3, 5], 3, 0) for md in (1, 3, 4, 5, 15, 16, 17)}
CASES["n400_md33"] = (400, 40, 3, 320, 33, [2, 3, 4], 2, 0)
CASES["n400_k20"] = (400, 3, 3, 320, 3, [17, 20], 2, 0)
CASES["n700_md128"] = (700, 128, 3, 560, 128, [2, 3], 2, 0)


def problem(rows, K, n_init, seed, km_labels, perm):
    """make_gmm_fixtures.problem for covariance_type='full'."""
    from sklearn.mixture import GaussianMixture
    from threadpoolctl import threadpool_limits

    with threadpool_limits(1), warnings.catch_warnings():
        warnings.simplefilter("ignore")  # sklearn's ConvergenceWarning: converged_ records it
        sk = GaussianMixture(n_components=K, covariance_type='full', n_init=n_init, random_state=seed).fit(rows)
        sk_labels = sk.predict(rows)
        best, win, lab = G.fit_from_labels(rows, km_labels[:n_init], K, covariance_type='full')
        rows2 = np.ascontiguousarray(rows[perm][:, ::-1])
        km2 = [l[perm] for l in km_labels]
        best2, win2, lab2 = G.fit_from_labels(rows2, km2[:n_init], K, covariance_type='full')
        agree = (np.array_equal(sk_labels, lab) and np.array_equal(lab[perm], lab2)
                 and sk.n_iter_ == best["n_iter"] == best2["n_iter"]
                 and bool(sk.converged_) == best["converged"] == best2["converged"] and win == win2)
        lbs = (float(sk.lower_bound_), best["lower_bound"], best2["lower_bound"])
        rel = max(_rel(lbs[0], lbs[1]), _rel(lbs[0], lbs[2]), _rel(lbs[1], lbs[2]))
        margin = np.inf
        tiny = np.finfo(np.float64).tiny
        for j in range(n_init):
            if j != win and not np.array_equal(km_labels[j], km_labels[win]):
                a = _rel(G.em(rows, km_labels[j], K, 1e-3, 1e-6, 100, 'full')["lower_bound"], lbs[1])
                b = _rel(G.em(rows2, km2[j], K, 1e-3, 1e-6, 100, 'full')["lower_bound"], lbs[2])
                if a == 0.0 and b == 0.0:
                    continue  # an exact tie under both orders of the sums
                margin = min(margin, a if a > 0.0 else tiny, b if b > 0.0 else tiny)
    return dict(labels=sk_labels, n_iter=int(sk.n_iter_), converged=bool(sk.converged_), lower_bound=lbs[0],
                win=win), agree, rel, margin


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
        raise SystemExit(f"fullgmm_{case}: NOT KEPT, sklearn, the host form and the reordered host form disagree on "
                         f"(h, K, n_init) {unstable}: give the case another noise seed")
    meta = dict(kind="fullgmm", case=case, n=n, d=d, k_true=k_true, m=m, md=md, Ks=Ks, seed=SEED, H=H, noise=noise,
                n_inits=list(N_INITS), x_sha256=digest(X), lb_rel_seen=worst,
                init_margin_seen=min(m for m, _ in margins), threads=1, sklearn=sklearn.__version__,
                numpy=np.__version__, scipy=scipy.__version__,
                note="make_sk_fixtures._f64_noisy rows (noise seed = noise); sklearn GaussianMixture('full') float64, "
                     "1 thread, on ascontiguousarray(X[idx[h]][:, cols[h]]); kept only because sklearn, gmm.py and "
                     "gmm.py on permuted rows / reversed columns agree on every problem")
    arrays = dict(idx=idx, cols=cols.astype(np.int32), Ks=np.asarray(Ks, dtype=np.int32), km_labels=km,
                  lb_rtol=np.float64(lb_rtol), meta=np.array(json.dumps(meta)))
    for i in N_INITS:
        for key, v in out[i].items():
            arrays[f"{key}_{i}"] = v
    np.savez_compressed(os.path.join(OUT, f"fullgmm_{case}.npz"), **arrays)
    print(f"fullgmm_{case}: {nK * H * len(N_INITS)} problems ({time.time() - t0:.0f} s); n_iter "
          f"{min(o['n_iter'].min() for o in out.values())}..{max(o['n_iter'].max() for o in out.values())}, "
          f"lower bound within {worst:.2e}, lb_rtol {lb_rtol:.2e}", flush=True)


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    os.makedirs(OUT, exist_ok=True)
    for c in sys.argv[1:] or list(CASES):
        make(c)
