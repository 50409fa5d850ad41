"""sklearn-side fixtures for the NMF base clusterer (tests/test_nmf_host.py, tests/test_gpu_nmf.py),
generated ONCE on a CPU like make_gmm_fixtures.py's, whose resample draw and column draw this file
reuses.

Every problem is the host loop's call for resample h and K: ``NMF(n_components=K, n_init=n_init,
random_state=seed, tol, max_iter)`` in float64 on one thread, on ``ascontiguousarray(X[idx[h]][:,
cols[h]])`` with ``cols = post.feature_indices(seed, d, md, H)`` (all columns when md = d).  At
n_init = 1 that is ``sklearn.decomposition.NMF(K, init='random', solver='mu', random_state=seed,
tol=tol, max_iter=max_iter)`` with the label rule of nmf.py applied to its W and H.

The rows are non-negative blobs that are exact in float32: abs(centres ~ U(0, 10) + N(0, 1)) rounded
through float32, with one row (the first item of resample 0) and one column (column 1) set to 0, so
that the zero-denominator substitution and an all-zero row of W occur.

n_init is 1 for every problem, and also 3 for the problems with K >= 2 and md >= 3.  The rest (K = 1,
and md = 1 where the fit is exact) have a single optimum that every init reaches, so which init is
"strictly smaller" is decided by rounding; they stay at n_init = 1 (``has3`` marks the others).

The stability screen.  Per problem the generator runs sklearn's NMF (for n_init = 1), the host form
and the host form with the rows permuted and the columns reversed (the init arrays permuted alike,
so only the order of the sums changes).  A case is KEPT ONLY IF all three agree on every problem's
labels, n_iter, converged and winning init, and no losing init's error comes within 2 err_tol of
the winner's; a case that does not gets another noise seed (``noise`` below), never a weaker rule.
This is a condition on the inputs, checked on the CPU, so that the exact comparisons of the GPU
tests leave out no problem.  ``err_tol`` is 64 times the largest difference of reconstruction_err_
among the three over the case, measured relative to the error at init (the scale of the stopping
test; at md = 1 the error itself is about 1e-15), floored at 1e-13: headroom for a third order of
the same sums, the device's.  It is the only tolerance the tests use.

``tests/golden/sk/nmf_<case>.npz``: idx int32 [H, m], cols int32 [H, md], Ks, has3 bool [nK], and for
n_init = i in (1, 3) labels_i uint8 [nK, H, m], n_iter_i int32, converged_i bool, err_i float64
(reconstruction_err_), err0_i float64 (the winner's error at init), win_i int32 (all [nK, H]; the
n_init = 3 arrays are filled where has3), err_tol, meta (JSON: the recipe, the X digest, the
versions).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_nmf_fixtures.py [case ...]
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

from consensus_clustering_amd import nmf as N  # noqa: E402
from make_gmm_fixtures import columns, digest, indices  # noqa: E402

SEED = 3
N_INITS = (1, 3)
# case: n, d, k_true, m, md, Ks, H, noise seed, tol, max_iter
CASES = {f"n96_md{md}": (96, 13, 3, 76, md, [1, 2, 3, 7, 16, 17], 3, 0, 1e-3, 200) for md in (1, 3, 4, 5, 12, 13)}
CASES["n300_md120"] = (300, 150, 3, 240, 120, [2, 3, 5], 3, 0, 1e-3, 200)
CASES["n160_k127"] = (160, 3, 3, 130, 3, [127], 3, 0, 1e-3, 200)
CASES["n96_md5_default"] = CASES["n96_md5"][:-2] + (1e-4, 200)  # NMF's defaults: mostly runs to max_iter


def rows_of(n, d, k, m, noise=0, seed=SEED):
    """abs(centres ~ U(0, 10) + N(0, 1)) from default_rng([n, d, noise]), through float32; the first
    item of resample 0 and column 1 % d set to 0."""
    rng = np.random.default_rng([n, d, noise])
    centres = rng.uniform(0.0, 10.0, size=(k, d))
    member = rng.integers(0, k, size=n)
    X = np.abs(centres[member] + rng.standard_normal((n, d))).astype(np.float32).astype(np.float64)
    X[indices(n, m, seed, 0)[0]] = 0.0
    X[:, 1 % d] = 0.0
    return X


def problem(rows, K, n_init, seed, tol, max_iter, perm):
    """sklearn's fit (n_init = 1), the host form and the reordered host form of one problem:
    (result dict, agree, the largest error difference relative to the error at init, the smallest
    such distance of a losing init's error to the winner's)."""
    from sklearn.decomposition import NMF as SkNMF
    from threadpoolctl import threadpool_limits

    m, md = rows.shape
    rs = np.random.RandomState(seed)
    normals = [N.init_normals(rs, m, md, K) for _ in range(n_init)]
    with threadpool_limits(1), warnings.catch_warnings():
        warnings.simplefilter("ignore")  # sklearn's ConvergenceWarning: converged records it
        est = N.NMF(n_components=K, n_init=n_init, random_state=seed, tol=tol, max_iter=max_iter).fit(rows)
        best, win, lab, runs = N.fit_from_normals(rows, normals, K, tol, max_iter)
        rows2 = np.ascontiguousarray(rows[perm][:, ::-1])
        normals2 = [(np.ascontiguousarray(W[perm]), np.ascontiguousarray(H[:, ::-1])) for W, H in normals]
        best2, win2, lab2, runs2 = N.fit_from_normals(rows2, normals2, K, tol, max_iter)
        agree = (np.array_equal(est.labels_, lab) and est.n_iter_ == best["n_iter"] and est.best_init_ == win
                 and est.reconstruction_err_ == best["reconstruction_err"])
        errs = [best["reconstruction_err"], best2["reconstruction_err"]]
        if n_init == 1:
            sk = SkNMF(K, init='random', solver='mu', random_state=seed, tol=tol, max_iter=max_iter)
            W = sk.fit_transform(rows)
            agree = (agree and np.array_equal(N.labels_of(W, sk.components_), lab) and sk.n_iter_ == best["n_iter"]
                     and np.array_equal(W, best["W"]) and np.array_equal(sk.components_, best["H"]))
            errs.append(float(sk.reconstruction_err_))
    agree = (agree and np.array_equal(lab[perm], lab2) and best["n_iter"] == best2["n_iter"]
             and best["converged"] == best2["converged"] and win == win2)
    err0 = best["error_at_init"]
    scale = err0 if err0 > 0 else 1.0
    rel = (max(errs) - min(errs)) / scale
    margin = np.inf
    for j in range(n_init):
        if j != win:
            margin = min(margin, abs(runs[j]["reconstruction_err"] - errs[0]) / scale)
        if j != win2:
            margin = min(margin, abs(runs2[j]["reconstruction_err"] - errs[1]) / scale)
    return dict(labels=lab, n_iter=int(best["n_iter"]), converged=bool(best["converged"]), err=errs[0], err0=err0,
                win=win), agree, rel, margin


def make(case):
    import scipy
    import sklearn

    n, d, k_true, m, md, Ks, H, noise, tol, max_iter = CASES[case]
    X = rows_of(n, d, k_true, m, noise)
    idx = np.stack([indices(n, m, SEED, h) for h in range(H)]).astype(np.int32)
    cols = columns(d, md, H)
    nK = len(Ks)
    has3 = np.array([K >= 2 and md >= 3 for K in Ks])
    out = {i: dict(labels=np.zeros((nK, H, m), dtype=np.uint8), n_iter=np.zeros((nK, H), dtype=np.int32),
                   converged=np.zeros((nK, H), dtype=bool), err=np.zeros((nK, H)), err0=np.zeros((nK, H)),
                   win=np.zeros((nK, H), dtype=np.int32)) for i in N_INITS}
    worst, unstable, margins, count = 0.0, [], [], 0
    t0 = time.time()
    for h in range(H):
        rows = np.ascontiguousarray(X[idx[h]][:, cols[h]])
        perm = np.random.default_rng(1000 + h).permutation(m)
        for k, K in enumerate(Ks):
            for i in N_INITS:
                if i > 1 and not has3[k]:
                    continue
                res, agree, rel, margin = problem(rows, K, i, SEED, tol, max_iter, perm)
                count += 1
                worst = max(worst, rel)
                margins.append((margin, (h, K, i)))
                if not agree:
                    unstable.append((h, K, i))
                for key, v in res.items():
                    out[i][key][k, h] = v
    err_tol = max(64 * worst, 1e-13)
    unstable += [("init margin", margin) + at for margin, at in margins if margin <= 2 * err_tol]
    if unstable:
        raise SystemExit(f"nmf_{case}: NOT KEPT, sklearn, the host form and the reordered host form disagree on "
                         f"(h, K, n_init) {unstable}: give the case another noise seed")
    meta = dict(kind="nmf", case=case, n=n, d=d, k_true=k_true, m=m, md=md, Ks=Ks, seed=SEED, H=H, noise=noise,
                tol=tol, max_iter=max_iter, n_inits=list(N_INITS), x_sha256=digest(X), err_rel_seen=worst,
                init_margin_seen=min(v for v, _ in margins), threads=1, sklearn=sklearn.__version__,
                numpy=np.__version__, scipy=scipy.__version__,
                note="rows_of(n, d, k_true, m, noise); sklearn NMF(init='random', solver='mu') float64, 1 thread, on "
                     "ascontiguousarray(X[idx[h]][:, cols[h]]); kept only because sklearn, nmf.py and nmf.py on "
                     "permuted rows / reversed columns agree on every problem")
    arrays = dict(idx=idx, cols=cols.astype(np.int32), Ks=np.asarray(Ks, dtype=np.int32), has3=has3,
                  err_tol=np.float64(err_tol), meta=np.array(json.dumps(meta)))
    for i in N_INITS:
        for key, v in out[i].items():
            arrays[f"{key}_{i}"] = v
    np.savez_compressed(os.path.join(OUT, f"nmf_{case}.npz"), **arrays)
    nit = np.concatenate([out[1]["n_iter"].ravel(), out[3]["n_iter"][has3].ravel()])
    print(f"nmf_{case}: {count} problems ({time.time() - t0:.0f} s); n_iter {nit.min()}..{nit.max()}, "
          f"converged {int(out[1]['converged'].sum())} of {nK * H} at n_init 1, error within {worst:.2e} of the error "
          f"at init, err_tol {err_tol:.2e}, smallest init margin {min(v for v, _ in margins):.2e}", flush=True)


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    os.makedirs(OUT, exist_ok=True)
    for c in sys.argv[1:] or list(CASES):
        make(c)
