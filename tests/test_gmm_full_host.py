"""The host form of the full-covariance GMM base clusterer (consensus_clustering_amd/gmm.py,
FullGMM) against the sklearn fixtures of tests/golden/make_gmm_full_fixtures.py, the estimator's
protocol and refusals, the device route's decision (_gmm_full_spec), the declared entry points and
the batch planner.  No GPU."""
import glob
import hashlib
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
from sklearn.base import clone

import consensus_clustering_amd
from consensus_clustering_amd import GMM, FullGMM, _lib, api, engine
from consensus_clustering_amd import gmm as G

HERE = os.path.dirname(os.path.abspath(__file__))
SK = os.path.join(HERE, "golden", "sk")
CASES = sorted(os.path.basename(p)[8:-4] for p in glob.glob(os.path.join(SK, "fullgmm_*.npz")))
ENTRY_POINTS = ("cc_gmm_full_workspace_bytes", "cc_gmm_full_start", "cc_gmm_full_em_step", "cc_gmm_full_finish")


class SubFullGMM(FullGMM):
    """A subclass: never routed to the device."""


def load_case(case):
    """(fixture arrays, meta, X): the rows are rebuilt from the recorded recipe and checked
    against the recorded digest."""
    from sklearn.datasets import make_blobs

    fx = np.load(os.path.join(SK, f"fullgmm_{case}.npz"))
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
    assert CASES == sorted([f"n200_md{md}" for md in (1, 3, 4, 5, 15, 16, 17)] + ["n400_md33", "n400_k20",
                                                                                  "n700_md128"])
    for case in CASES:
        meta = json.loads(str(np.load(os.path.join(SK, f"fullgmm_{case}.npz"))["meta"]))
        assert meta["noise"] == 0 and meta["kind"] == "fullgmm"


def test_the_small_cases_iterate_well_past_two():
    for case in ("n200_md3", "n200_md4", "n200_md5", "n400_k20"):
        fx = np.load(os.path.join(SK, f"fullgmm_{case}.npz"))
        assert max(int(fx["n_iter_1"].max()), int(fx["n_iter_3"].max())) >= 20, case


@pytest.mark.parametrize("case", CASES)
def test_host_form_equals_sklearn_fixture(case):
    fx, meta, X = load_case(case)
    rtol = float(fx["lb_rtol"])
    assert 1e-13 <= rtol < 1e-6
    for h in range(meta["H"]):
        rows = np.ascontiguousarray(X[fx["idx"][h]][:, fx["cols"][h]])
        for k, K in enumerate(meta["Ks"]):
            for n_init in meta["n_inits"]:
                est = FullGMM(n_components=K, n_init=n_init, random_state=meta["seed"]).fit(rows)
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
                md = rows.shape[1]
                assert est.weights_.shape == (K,) and est.means_.shape == (K, md)
                assert est.covariances_.shape == est.precisions_cholesky_.shape == (K, md, md)
                assert not np.tril(est.precisions_cholesky_, -1).any()  # upper triangular


def test_the_diagonal_calls_keep_their_results():
    """em and fit_from_labels without the covariance argument are the diagonal model's, and a
    diagonal covariance gives both models the same mixture up to rounding."""
    rs = np.random.RandomState(0)
    X = np.concatenate([rs.randn(30, 3) * [1.0, 2.0, 0.5], rs.randn(30, 3) + 6.0])
    lab = (np.arange(60) >= 30).astype(np.int64)
    a = G.em(X, lab, 2, 1e-3, 1e-6, 100)
    b = G.em(X, lab, 2, 1e-3, 1e-6, 100, 'diag')
    assert a["lower_bound"] == b["lower_bound"] and a["covariances"].shape == (2, 3) and "precisions_cholesky" not in a
    best, win, labels = G.fit_from_labels(X, [lab], 2)
    assert best["lower_bound"] == a["lower_bound"] and win == 0
    np.testing.assert_array_equal(labels, lab)
    np.testing.assert_array_equal(labels, G.final_labels(X, a))
    full = G.em(X, lab, 2, 1e-3, 1e-6, 100, 'full')
    assert full["covariances"].shape == full["precisions_cholesky"].shape == (2, 3, 3)
    # the full model's bound is at least the diagonal model's optimum on the same start, up to tol
    assert full["lower_bound"] > a["lower_bound"] - 1e-2


def test_float32_input_is_computed_in_float64():
    X = np.random.RandomState(0).randn(40, 3)
    a = FullGMM(2, random_state=0).fit(X.astype(np.float32))
    b = FullGMM(2, random_state=0).fit(X.astype(np.float32).astype(np.float64))
    assert a.means_.dtype == a.covariances_.dtype == np.float64 and a.lower_bound_ == b.lower_bound_
    np.testing.assert_array_equal(a.labels_, b.labels_)


def test_params_clone_pickle_repr():
    est = FullGMM(n_components=3, tol=1e-4, n_init=2, random_state=7)
    p = est.get_params()
    assert p == dict(n_components=3, tol=1e-4, reg_covar=1e-6, max_iter=100, n_init=2, random_state=7)
    assert FullGMM().set_params(**p).get_params() == p
    assert clone(est).get_params() == p and type(clone(SubFullGMM(2))) is SubFullGMM
    assert pickle.loads(pickle.dumps(est)).get_params() == p
    assert pickle.loads(pickle.dumps(est.fit(np.random.RandomState(1).randn(30, 2)))).covariances_.shape == (3, 2, 2)
    assert repr(est) == "FullGMM(n_components=3, tol=0.0001, reg_covar=1e-06, max_iter=100, n_init=2, random_state=7)"
    assert repr(SubFullGMM()).startswith("SubFullGMM(")
    with pytest.raises(ValueError, match=r"Invalid parameter 'n_clusters' for estimator FullGMM\(\)"):
        est.set_params(n_clusters=2)
    with pytest.raises(ValueError, match=r"Invalid parameter 'covariance_type' for estimator FullGMM\(\)"):
        est.set_params(covariance_type='diag')
    assert est.covariance_type == FullGMM.covariance_type == 'full'
    assert consensus_clustering_amd.FullGMM is FullGMM and not issubclass(FullGMM, GMM)


def test_set_clusterer_K_with_the_default_options():
    cc = consensus_clustering_amd.ConsensusClustering(clusterer=FullGMM(), K_range=[4], random_state=11,
                                                      plot_cdf=False)
    cc._K = 4
    cc._set_clusterer_K()
    p = cc.clusterer.get_params()
    assert (p["n_components"], p["random_state"], p["n_init"]) == (4, 11, 3)


@pytest.mark.parametrize("params, match", [
    (dict(n_components=0), "'n_components' parameter of FullGMM must be an int in the range \\[1, inf\\)"),
    (dict(n_components=2.0), "'n_components' parameter"),
    (dict(n_components=True), "'n_components' parameter"),
    (dict(max_iter=0), "'max_iter' parameter of FullGMM must be an int in the range \\[1, inf\\)"),
    (dict(n_init=0), "'n_init' parameter"),
    (dict(n_init=1.5), "'n_init' parameter"),
    (dict(tol=-1e-3), "'tol' parameter of FullGMM must be a float in the range \\[0.0, inf\\)"),
    (dict(reg_covar=-1.0), "'reg_covar' parameter"),
    (dict(reg_covar=float('nan')), "'reg_covar' parameter"),
])
def test_parameter_refusals(params, match):
    X = np.random.RandomState(0).randn(20, 2)
    with pytest.raises(ValueError, match=match):
        FullGMM(**{**dict(n_components=2), **params}).fit(X)


def test_data_refusals():
    X = np.random.RandomState(0).randn(20, 2)
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="Input X contains NaN."):
        FullGMM(2).fit(bad)
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="Input X contains infinity"):
        FullGMM(2).fit(bad)
    with pytest.raises(ValueError, match=r"Found array with 1 sample\(s\) .* minimum of 2 is required by FullGMM"):
        FullGMM(1).fit(X[:1])
    with pytest.raises(ValueError, match="Expected n_samples >= n_components but got n_components = 21, n_samples = 20"):
        FullGMM(21).fit(X)
    with pytest.raises(ValueError, match="Expected 2D array"):
        FullGMM(2).fit(X[:, 0])


def test_ill_defined_covariance():
    X = np.repeat(np.array([[0.0, 1.0], [4.0, 2.0]]), 5, axis=0)  # duplicated points: zero covariances
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        FullGMM(2, reg_covar=0.0, random_state=0).fit(X)
    assert FullGMM(2, random_state=0).fit(X).converged_  # reg_covar carries them


def test_gmm_full_spec_table():
    from sklearn.mixture import GaussianMixture

    assert api._gmm_full_spec(FullGMM()) == dict(n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6)
    assert api._gmm_full_spec(FullGMM(n_init=np.int64(3), tol=0, max_iter=7)) == dict(n_init=3, max_iter=7, tol=0.0,
                                                                                      reg_covar=1e-6)
    for est in (GMM(), GMM(covariance_type='full'), SubFullGMM(), FullGMM(max_iter=0), FullGMM(n_init=True),
                FullGMM(n_init=0), FullGMM(tol=-1.0), FullGMM(tol=float('inf')), FullGMM(reg_covar=float('nan')),
                FullGMM(tol='x'), FullGMM(max_iter=2.0), GaussianMixture(), GaussianMixture(covariance_type='full'),
                object()):
        assert api._gmm_full_spec(est) is None, est
    # and the diagonal route is what it was
    assert api._gmm_spec(FullGMM()) is None and api._gmm_spec(GMM(covariance_type='full')) is None
    assert api._gmm_spec(GMM()) == dict(n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6)


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
        return int(lib.cc_gmm_full_workspace_bytes(m, md, B, a.ctypes.data, len(a)))

    def up256(v):
        return (v + 255) & ~255

    for m, md, Ks in ((160, 5, [1, 2, 3, 5]), (320, 33, [2, 3, 4]), (320, 3, [17, 20]), (560, 128, [2, 3]),
                      (130, 3, [127]), (8000, 64, range(2, 16))):
        Ks = list(Ks)
        per = engine.gmm_full_bytes(m, md, Ks)
        for B in (1, 3, 64):
            # the planner's count of one resample is the workspace's share plus the engine's own
            # rows [m, md] and indices (and 16 spare bytes per 48-byte state)
            got = ws(m, md, B, Ks)
            own = 8 * m * md + 4 * m + 4 * md
            assert got == 256 + up256(48 * B * len(Ks)) + B * (per - own - 64 * len(Ks)), (m, md, B)
            assert got > B * 8 * sum(K * md * md + m * ((K + 15) // 16 * 16) for K in Ks)
    assert ws(76, 5, 1, [77]) == 0 and ws(76, 5, 1, [128]) == 0 and ws(76, 5, 1, [0]) == 0
    assert ws(76, 0, 1, [2]) == 0 and ws(76, 5, 0, [2]) == 0 and ws(200, 5, 600, list(range(1, 128))) == 0
    assert ws(300, 128, 1, [2]) > 0 and ws(300, 129, 1, [2]) == 0  # the md limit
    assert engine.GMM_FULL_MD_MAX == 128

    n, m, md, Ks = 200, 160, 5, [2, 3, 17]
    per = engine.gmm_full_bytes(m, md, Ks) + len(Ks) * n
    fixed = 1024 + 127 * len(Ks) * n
    assert engine.gmm_full_plan(n, m, 7, Ks, md, fixed + per) == 1
    assert engine.gmm_full_plan(n, m, 7, Ks, md, fixed + 3 * per + per - 1) == 3
    assert engine.gmm_full_plan(n, m, 7, Ks, md, 1 << 40) == 7
    assert engine.gmm_full_plan(n, m, 60000, [2] * 100, md, 1 << 50) == 655
    assert engine.gmm_plan(n, m, 7, Ks, md, fixed + per, 'full') == 1
    with pytest.raises(ValueError, match=r"workspace_budget = \d+ bytes cannot hold the GMM clusterer: one resample of "
                                         r"m = 160 over 5 features \(\d+ bytes\) is needed"):
        engine.gmm_full_plan(n, m, 7, Ks, md, fixed + per - 1)


def test_module_imports_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "import importlib.util as u, os\n"
            "root = os.path.join(sys.argv[1], 'consensus_clustering_amd')\n"
            "import types; pkg = types.ModuleType('consensus_clustering_amd'); pkg.__path__ = [root]\n"
            "sys.modules['consensus_clustering_amd'] = pkg\n"
            "from consensus_clustering_amd.gmm import FullGMM\n"
            "import numpy as np\n"
            "X = np.random.RandomState(0).randn(30, 2)\n"
            "assert FullGMM(2, random_state=0).fit(X).covariances_.shape == (2, 2, 2)\n"
            "assert 'consensus_clustering_amd.engine' not in sys.modules\n")
    subprocess.run([sys.executable, "-c", code, os.path.dirname(HERE)], check=True, timeout=120)
