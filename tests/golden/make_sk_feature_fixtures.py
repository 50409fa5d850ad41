"""sklearn-side fixtures for the float64 k-means under feature subsampling
(tests/test_gpu_kmeans_features.py), generated ONCE in the development container like
make_sk_fixtures.py's, whose row recipe, resample draw and counting fit this file imports.

Every fit is the host loop's call for resample h and K: ``KMeans(n_clusters=K, random_state=3,
n_init=3)`` in float64 on one thread, on ``ascontiguousarray(X[indices(n, 3, h)][:, cols[h]])``
with ``cols = post.feature_indices(3, d, md, H)`` and ``md = int(fraction * d)``.  The fit runs
under make_sk_fixtures._fit_lowest_index, which counts the rows sklearn relocates into empty
clusters: the generator asserts that there are none, so numpy's order among tied farthest rows
cannot enter these fixtures.

``tests/golden/sk/f64_feat_<case>.npz``: labels int8 [nK, H, m], digest64 [nK, H], n_iter int32
[nK, H], inertia float64 [nK, H], cols int32 [H, md], meta (JSON: the X digest, the versions).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sk_feature_fixtures.py [case ...]
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

from make_sk_fixtures import _f64_noisy, _fit_lowest_index, digest, indices  # noqa: E402

from consensus_clustering_amd import post  # noqa: E402

SEED = 3
# case: n, d, k_true, fraction, Ks, H (the widths md = int(fraction * d): 9, 23, 120, 3)
CASES = {
    "n600_d12": (600, 12, 4, 0.8, [2, 3, 4, 6, 9], 4),
    "n29_d29": (29, 29, 3, 0.8, [2, 3, 4, 5, 6, 7, 8, 9, 10], 6),
    "n300_d150": (300, 150, 3, 0.8, [2, 3, 5], 3),
    "n200_d4": (200, 4, 3, 0.75, [2, 3, 5], 4),
}


def make(case):
    import sklearn

    n, d, k_true, fraction, Ks, H = CASES[case]
    X = _f64_noisy(n, d, k_true)
    m, md = int(0.8 * n), int(fraction * d)
    cols = post.feature_indices(SEED, d, md, H)
    labels = np.zeros((len(Ks), H, m), dtype=np.int8)
    dig = np.full((len(Ks), H), "", dtype="U64")
    nit = np.zeros((len(Ks), H), dtype=np.int32)
    inert = np.zeros((len(Ks), H), dtype=np.float64)
    t0 = time.time()
    for h in range(H):
        rows = np.ascontiguousarray(X[indices(n, SEED, h)][:, cols[h]])
        assert rows.dtype == np.float64 and rows.shape == (m, md)
        assert len(np.unique(rows, axis=0)) == m, (case, h, "duplicate rows")
        for k, K in enumerate(Ks):
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                lab, it, ine, relocated, _ = _fit_lowest_index(rows, K, SEED)
            assert relocated == 0, (case, K, h, relocated)
            labels[k, h], dig[k, h], nit[k, h], inert[k, h] = lab, digest(lab), it, ine
    meta = dict(kind="f64_feat", case=case, n=n, d=d, k_true=k_true, fraction=fraction, md=md, Ks=Ks, seed=SEED,
                frac=0.8, H=H, x_sha256=digest(X), relocated_rows=0, threads=1, sklearn=sklearn.__version__,
                numpy=np.__version__,
                note="make_sk_fixtures._f64_noisy rows; sklearn KMeans(n_init=3) float64, 1 thread, on "
                     "ascontiguousarray(X[idx[h]][:, cols[h]]), cols = post.feature_indices(seed, d, md, H)")
    np.savez_compressed(os.path.join(OUT, f"f64_feat_{case}.npz"), labels=labels, digest64=dig, n_iter=nit,
                        inertia=inert, cols=cols, meta=np.array(json.dumps(meta)))
    print(f"f64_feat_{case}: {len(Ks) * H} fits at md = {md} ({time.time() - t0:.0f} s); n_iter {nit.min()}..{nit.max()}, "
          f"no relocated row", flush=True)


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    os.makedirs(OUT, exist_ok=True)
    for c in sys.argv[1:] or list(CASES):
        make(c)
