"""The host form of the GMM base clusterer (consensus_clustering_amd/gmm.py) against the sklearn
fixtures of tests/golden/make_gmm_fixtures.py, the estimator's protocol and refusals, the device
route's decision (_gmm_spec), the declared entry points and the batch planner.  No GPU."""
import glob
import json
import os
import pickle
import re

import numpy as np
import pytest
from sklearn.base import clone

import consensus_clustering_amd
from consensus_clustering_amd import GMM, _lib, api, engine
from consensus_clustering_amd import gmm as G

HERE = os.path.dirname(os.path.abspath(__file__))
SK = os.path.join(HERE, "golden", "sk")
CASES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(SK, "gmm_*.npz")))
ENTRY_POINTS = ("cc_gmm_workspace_bytes", "cc_gmm_gather", "cc_gmm_start", "cc_gmm_em_step", "cc_gmm_active",
                "cc_gmm_finish")


class SubGMM(GMM):
    """A subclass: never routed to the device."""


def load_case(case):
    """(fixture arrays, meta, X): the rows are rebuilt from the recorded recipe and checked
    against the recorded digest."""
    import hashlib

    from sklearn.datasets import make_blobs

    fx = np.load(os.path.join(SK, f"gmm_{case}.npz"))
    meta = json.loads(str(fx["meta"]))
    n, d = meta["n"], meta["d"]
    X, _ = make_blobs(n_samples=n, n_features=d, centers=meta["k_true"], cluster_std=1.0, center_box=(-10, 10),
                      shuffle=True, random_state=n + d)
    X = X.astype(np.float32).astype(np.float64)
    X += np.random.default_rng(meta["noise"]).normal(scale=0.5, size=X.shape)
    a = np.ascontiguousarray(X)
    sha = hashlib.sha256(a.view(np.uint8).tobytes() + str(a.dtype).encode() + str(a.shape).encode()).hexdigest()
    assert sha == meta["x_sha256"], "the fixture's rows are not reproduced here"
    return fx, meta, X


def test_the_fixture_cases_are_all_there():
    assert CASES == sorted([f"n96_md{md}" for md in (1, 3, 4, 5, 12, 13)] + ["n300_md120", "n160_k127"])


@pytest.mark.parametrize("case", CASES)
def test_host_form_equals_sklearn_fixture(case):
    fx, meta, X = load_case(case)
    rtol = float(fx["lb_rtol"])
    assert 1e-13 <= rtol < 1e-6
    for h in range(meta["H"]):
        rows = np.ascontiguousarray(X[fx["idx"][h]][:, fx["cols"][h]])
        for k, K in enumerate(meta["Ks"]):
            for n_init in meta["n_inits"]:
                est = GMM(n_components=K, n_init=n_init, random_state=meta["seed"]).fit(rows)
                tag = f"h={h} K={K} n_init={n_init}"
                for i in range(n_init):
                    np.testing.assert_array_equal(est.init_labels_[i], fx["km_labels"][i, k, h], err_msg=tag)
                np.testing.assert_array_equal(est.labels_, fx[f"labels_{n_init}"][k, h], err_msg=tag)
                assert est.n_iter_ == fx[f"n_iter_{n_init}"][k, h], tag
                assert est.converged_ == fx[f"converged_{n_init}"][k, h], tag
                assert est.best_init_ == fx[f"win_{n_init}"][k, h], tag
                lb = fx[f"lower_bound_{n_init}"][k, h]
                print(f"{case} {tag}: lower bound {est.lower_bound_!r} against {lb!r}")
                assert abs(est.lower_bound_ - lb) <= rtol * abs(lb), tag
                assert est.weights_.shape == (K,) and est.means_.shape == est.covariances_.shape == (K, rows.shape[1])


def test_float32_input_is_computed_in_float64():
    X = np.random.RandomState(0).randn(40, 3)
    a = GMM(2, random_state=0).fit(X.astype(np.float32))
    b = GMM(2, random_state=0).fit(X.astype(np.float32).astype(np.float64))
    assert a.means_.dtype == np.float64 and a.lower_bound_ == b.lower_bound_
    np.testing.assert_array_equal(a.labels_, b.labels_)


def test_params_clone_pickle_repr():
    est = GMM(n_components=3, tol=1e-4, n_init=2, random_state=7)
    p = est.get_params()
    assert p == dict(n_components=3, covariance_type='diag', tol=1e-4, reg_covar=1e-6, max_iter=100, n_init=2,
                     random_state=7)
    assert GMM().set_params(**p).get_params() == p
    assert clone(est).get_params() == p and type(clone(SubGMM(2))) is SubGMM
    assert pickle.loads(pickle.dumps(est)).get_params() == p
    assert repr(est) == ("GMM(n_components=3, covariance_type='diag', tol=0.0001, reg_covar=1e-06, max_iter=100, "
                         "n_init=2, random_state=7)")
    assert repr(SubGMM()).startswith("SubGMM(")
    with pytest.raises(ValueError, match=r"Invalid parameter 'n_clusters' for estimator GMM\(\)"):
        est.set_params(n_clusters=2)
    assert consensus_clustering_amd.GMM is GMM


def test_set_clusterer_K_with_the_default_options():
    cc = consensus_clustering_amd.ConsensusClustering(clusterer=GMM(), K_range=[4], random_state=11, plot_cdf=False)
    cc._K = 4
    cc._set_clusterer_K()
    p = cc.clusterer.get_params()
    assert (p["n_components"], p["random_state"], p["n_init"]) == (4, 11, 3)


@pytest.mark.parametrize("params, match", [
    (dict(covariance_type='full'), "sklearn's GaussianMixture"),
    (dict(n_components=0), "'n_components' parameter of GMM must be an int in the range \\[1, inf\\)"),
    (dict(n_components=2.0), "'n_components' parameter"),
    (dict(n_components=True), "'n_components' parameter"),
    (dict(max_iter=0), "'max_iter' parameter of GMM must be an int in the range \\[1, inf\\)"),
    (dict(n_init=0), "'n_init' parameter"),
    (dict(n_init=1.5), "'n_init' parameter"),
    (dict(tol=-1e-3), "'tol' parameter of GMM must be a float in the range \\[0.0, inf\\)"),
    (dict(reg_covar=-1.0), "'reg_covar' parameter"),
    (dict(reg_covar=float('nan')), "'reg_covar' parameter"),
])
def test_parameter_refusals(params, match):
    X = np.random.RandomState(0).randn(20, 2)
    with pytest.raises(ValueError, match=match):
        GMM(**{**dict(n_components=2), **params}).fit(X)


def test_data_refusals():
    X = np.random.RandomState(0).randn(20, 2)
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="Input X contains NaN."):
        GMM(2).fit(bad)
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="Input X contains infinity"):
        GMM(2).fit(bad)
    with pytest.raises(ValueError, match=r"Found array with 1 sample\(s\) .* minimum of 2 is required by GMM"):
        GMM(1).fit(X[:1])
    with pytest.raises(ValueError, match="Expected n_samples >= n_components but got n_components = 21, n_samples = 20"):
        GMM(21).fit(X)
    with pytest.raises(ValueError, match="Expected 2D array"):
        GMM(2).fit(X[:, 0])
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        GMM(2, reg_covar=0.0, random_state=0).fit(np.repeat(np.array([[0.0, 1.0], [4.0, 2.0]]), 5, axis=0))


def test_gmm_spec_table():
    from sklearn.mixture import GaussianMixture

    assert api._gmm_spec(GMM()) == dict(n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6)
    assert api._gmm_spec(GMM(n_init=np.int64(3), tol=0, max_iter=7)) == dict(n_init=3, max_iter=7, tol=0.0,
                                                                            reg_covar=1e-6)
    for est in (SubGMM(), GMM(covariance_type='full'), GMM(max_iter=0), GMM(n_init=True), GMM(n_init=0),
                GMM(tol=-1.0), GMM(tol=float('inf')), GMM(reg_covar=float('nan')), GMM(tol='x'), GMM(max_iter=2.0),
                GaussianMixture(covariance_type='diag'), object()):
        assert api._gmm_spec(est) is None, est


def test_entry_points_declared_and_exported():
    with open(os.path.join(os.path.dirname(HERE), "include", "ccmi.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"^(int|size_t) " + name + r"\(", header, re.M), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def test_workspace_bytes_and_plan():
    lib = _lib.load()

    def ws(m, md, B, Ks):
        a = np.asarray(Ks, dtype=np.int32)
        return int(lib.cc_gmm_workspace_bytes(m, md, B, a.ctypes.data, len(a)))

    for m, md, Ks in ((76, 5, [1, 2, 3, 7, 16, 17]), (240, 120, [2, 3, 5]), (130, 3, [127]), (8000, 64, range(2, 16))):
        Ks = list(Ks)
        per = engine.gmm_bytes(m, md, Ks)
        for B in (1, 3, 64):
            got = ws(m, md, B, Ks)
            # the rows [m, md] and the indices are the engine's own; the rest is the workspace
            assert 0 < got <= 512 + B * (per - 8 * m * md), (m, md, B)
            assert got > B * 8 * m * sum((K + 15) // 16 * 16 for K in Ks)
    assert ws(76, 5, 1, [77]) == 0 and ws(76, 5, 1, [128]) == 0 and ws(76, 5, 1, [0]) == 0
    assert ws(76, 0, 1, [2]) == 0 and ws(76, 5, 0, [2]) == 0 and ws(200, 5, 600, list(range(1, 128))) == 0

    n, m, md, Ks = 96, 76, 5, [2, 3, 17]
    per = engine.gmm_bytes(m, md, Ks) + len(Ks) * n
    fixed = 1024 + 127 * len(Ks) * n
    assert engine.gmm_plan(n, m, 7, Ks, md, fixed + per) == 1
    assert engine.gmm_plan(n, m, 7, Ks, md, fixed + 3 * per + per - 1) == 3
    assert engine.gmm_plan(n, m, 7, Ks, md, 1 << 40) == 7
    assert engine.gmm_plan(n, m, 60000, [2] * 100, md, 1 << 50) == 655
    with pytest.raises(ValueError, match=r"workspace_budget = \d+ bytes cannot hold the GMM clusterer: one resample of "
                                         r"m = 76 over 5 features \(\d+ bytes\) is needed"):
        engine.gmm_plan(n, m, 7, Ks, md, fixed + per - 1)
