"""sklearn-side n_iter and inertia fixtures for the float32-class k-means engines, next to the
label fixtures of make_sk_fixtures.py (same rows, seed 7, frac 0.8, n_init 3, one thread), for the
cases tests/test_gpu_kmeans_bigk.py runs.  One file per case, tests/golden/sk/fit_<case>.npz:

* ``n_iter [nK, H]``: ``KMeans.n_iter_`` of sklearn's float32 fit of (K, h).
* ``exempt [nK, H]``: True where sklearn's float64 fit of the same rows has another ``n_iter_``
  (rounding decides the iteration count there, so the engines are not held to it).  At most 5 %
  of a case's problems may be exempt; the generator refuses more.
* ``inertia64 [nK, H]``: sum_r |x_r - c_label(r)|^2 in float64, x the float32 rows and c sklearn's
  float32 ``cluster_centers_``.
* ``sigma [nK, H]``: the rounding model of the engines' inertia.  An engine adds, per row, the
  float32 terms |x|^2 + (|c|^2 - 2 x.c) of the globally centred rows; the result is rounded once
  at the magnitude of the cancelling terms, u_r = 2^-24 (|x_r| + |c_r|)^2, and independent
  roundings add in quadrature: sigma = sqrt(sum_r u_r^2) / inertia64.
* ``emu_err [nK, H]``: a CPU emulation of the engines' documented arithmetic minus inertia64:
  |x|^2 the sequential float32 fma over the centred row (tests/row_image_ref.py), |c|^2 the same
  over the float32 centre, x.c at the f16 hi/lo operand precision and the engine's scale exponent
  (tests/sk_parity._dot22), one float32 subtraction and one float32 add per row, summed in
  float64.  tests/test_sk_fit_fixtures_host.py holds it to the bound the GPU test holds the
  engines to, |err| / inertia64 <= 8 sigma + 2^-19.
* ``digest [nK, H]``: the label digest of each fit.  The generator asserts that these fits are the
  ones the label fixture <case>.npz describes (``ref32`` / ``ref_digest``).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sk_fit_fixtures.py [case ...]
"""
from __future__ import annotations

import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "sk")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_sk_fixtures import CASES, digest, indices  # noqa: E402

# case -> resamples, as tests/test_gpu_kmeans_bigk.py runs them
FIT_CASES = {
    "bigk_n1536_d16": 3, "bigk_n1536_d40": 3, "bigk_n1536_d100": 3, "range_n1536_d16": 3,
    "bigk5_n1024_d300": 2, "bigk_n1024_d300": 2, "range_n1024_d300": 2,
}
N_INIT = 3
MAX_EXEMPT = 0.05

_X, _IMG = {}, {}


def _task(args):
    from sklearn.cluster import KMeans
    from threadpoolctl import threadpool_limits

    from tests.row_image_ref import xnorm_fma
    from tests.sk_parity import _dot22

    case, K, h = args
    X, img, seed = _X[case], _IMG[case], CASES[case]["seed"]
    d = X.shape[1]
    idx = indices(X.shape[0], seed, h)
    rows = X[idx]
    with threadpool_limits(1):
        km = KMeans(n_clusters=K, random_state=seed, n_init=N_INIT).fit(rows)
        km64 = KMeans(n_clusters=K, random_state=seed, n_init=N_INIT).fit(rows.astype(np.float64))
        lab = km.labels_.astype(np.int64)
        C = np.asarray(km.cluster_centers_, dtype=np.float32)
        inertia64 = float(((rows.astype(np.float64) - C.astype(np.float64)[lab]) ** 2).sum())
        # the engines' coordinates: rows and centres less the column means of all n rows
        xd = img["Xd"][idx][:, :d]
        c = (C - img["mean"][None, :]).astype(np.float32)
        xl = np.sqrt((xd.astype(np.float64) ** 2).sum(axis=1))
        cl = np.sqrt((c.astype(np.float64) ** 2).sum(axis=1))[lab]
        u = 2.0 ** -24 * (xl + cl) ** 2
        sigma = float(np.sqrt((u ** 2).sum()) / inertia64)
        cn = xnorm_fma(c)[0]
        xc = _dot22(xd, c, img["e"])[np.arange(len(lab)), lab]
        dist = (cn[lab] - np.float32(2) * xc).astype(np.float32)
        per_row = (img["xnorm"][idx] + dist).astype(np.float32)
        emu = float(per_row.astype(np.float64).sum())
    return (case, K, h, km.labels_.astype(np.int8), int(km.n_iter_), int(km64.n_iter_),
            bool(np.array_equal(km.labels_, km64.labels_)), inertia64, sigma, emu - inertia64)


def make(case, ex):
    from tests.sk_parity import load_sk_fixture

    spec, H = CASES[case], FIT_CASES[case]
    Ks, X = spec["Ks"], _X[case]
    lf = load_sk_fixture(case)
    meta = lf["meta"]
    assert digest(X) == meta["x_sha256"] and meta["Ks"] == Ks and meta["seed"] == spec["seed"]
    assert sorted(meta["classify"] + meta["ref"]) == list(range(H)), (case, meta["classify"], meta["ref"])
    t0 = time.time()
    res = list(ex.map(_task, [(case, K, h) for K in Ks for h in range(H)]))
    shape = (len(Ks), H)
    nit = np.zeros(shape, np.int32)
    exempt = np.zeros(shape, bool)
    inertia64, sigma, emu_err = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    dig = np.full(shape, "", dtype="U64")
    for (_, K, h, lab, it, it64, same64, i64, sg, err) in res:
        k = Ks.index(K)
        # both fixtures describe the same fits
        if h in meta["classify"]:
            assert np.array_equal(lab, lf["ref32"][k, meta["classify"].index(h)]), (case, K, h)
        else:
            assert digest(lab) == lf["ref_digest"][k, meta["ref"].index(h)], (case, K, h)
        nit[k, h], exempt[k, h] = it, it != it64
        inertia64[k, h], sigma[k, h], emu_err[k, h], dig[k, h] = i64, sg, err, digest(lab)
        if not same64:
            print(f"  {case} K={K} h={h}: sklearn's float64 labels differ from its float32 ones", flush=True)
    assert exempt.mean() <= MAX_EXEMPT, (case, np.argwhere(exempt).tolist())
    import sklearn

    fmeta = dict(kind="fit", case=case, n=X.shape[0], d=X.shape[1], Ks=Ks, H=H, seed=spec["seed"], frac=0.8,
                 n_init=N_INIT, x_sha256=digest(X), scale_exp=int(_IMG[case]["e"]), threads=1,
                 sklearn=sklearn.__version__, numpy=np.__version__)
    np.savez_compressed(os.path.join(OUT, f"fit_{case}.npz"), n_iter=nit, exempt=exempt, inertia64=inertia64,
                        sigma=sigma, emu_err=emu_err, digest=dig, x_sha256=np.array(digest(X)),
                        meta=np.array(json.dumps(fmeta)))
    ratio = np.abs(emu_err) / inertia64 / (8 * sigma + 2.0 ** -19)
    print(f"fit_{case}: {len(res)} fits ({time.time() - t0:.0f} s); n_iter {nit.min()}..{nit.max()}, "
          f"{int(exempt.sum())} exempt; 8 sigma {8 * sigma.min():.2e}..{8 * sigma.max():.2e}; emulation "
          f"max |err| / sigma {np.max(np.abs(emu_err) / inertia64 / sigma):.2f}, max |err| / bound {ratio.max():.3f}",
          flush=True)


def main(argv):
    from tests.row_image_ref import row_image

    os.makedirs(OUT, exist_ok=True)
    want = argv or list(FIT_CASES)
    for c in want:
        _X[c] = CASES[c]["X"]()
        _IMG[c] = row_image(_X[c])
    with ProcessPoolExecutor(int(os.environ.get("SK_WORKERS", "8"))) as ex:  # fork: the workers see _X
        for c in want:
            make(c, ex)


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main(sys.argv[1:])
