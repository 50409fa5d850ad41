"""The host form of the PAM base clusterer (consensus_clustering_amd/pam.py) against the
brute-force reference of tests/pam_ref.py, the estimator's protocol and refusals, the device
route's decision (_pam_spec) and batch planner, and the host loop with a PAM subclass.  No GPU."""
import pickle
import sys

import numpy as np
import pytest
from scipy.spatial.distance import pdist, squareform
from sklearn.base import clone
from sklearn.cluster import KMeans

import consensus_clustering_amd
from consensus_clustering_amd import PAM, api, engine
from consensus_clustering_amd import pam as P
from tests.pam_ref import pam_ref

METRICS = ["euclidean", "manhattan", "cosine", "correlation"]


class SubPAM(PAM):
    """A subclass: never routed to the device."""


def lattice(half_rows=16, seed=1):
    """An integer lattice with every row twice: under cityblock every sum is exact, and equal
    distances are everywhere."""
    half = np.random.RandomState(seed).randint(0, 3, size=(half_rows, 2)).astype(np.float64)
    return np.concatenate([half, half])


def same_partition(a, b):
    return np.array_equal(a[:, None] == a[None, :], b[:, None] == b[None, :])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m", [2, 3, 10, 33])
def test_pam_equals_the_brute_force_reference(m, metric):
    X = np.random.RandomState(m).randn(m, 5)
    D = squareform(pdist(X, P.METRICS[metric]))
    for K in range(1, m + 1):
        ref = pam_ref(D, K)
        est = PAM(n_clusters=K, metric=metric).fit(X)
        np.testing.assert_array_equal(est.medoid_indices_, ref.medoids, err_msg=f"K={K}")
        assert same_partition(est.labels_, ref.labels), K
        np.testing.assert_array_equal(est.labels_, ref.labels, err_msg=f"K={K}")
        assert est.n_iter_ == ref.n_iter, K
        assert abs(est.inertia_ - ref.inertia) <= m * 2.0 ** -52 * ref.inertia, K
        np.testing.assert_array_equal(est.labels_[est.medoid_indices_], np.arange(K))


def test_build_prefix_property():
    D = squareform(pdist(np.random.RandomState(0).randn(40, 4)))
    chain = P.build(D, 40)
    assert sorted(chain) == list(range(40))
    for K in (1, 2, 7, 39):
        assert P.build(D, K) == chain[:K]
        ref = pam_ref(D, K, max_iter=0)
        np.testing.assert_array_equal(ref.medoids, sorted(chain[:K]))


def test_lattice_is_exact_tie_rules_included():
    X = lattice()
    D = squareform(pdist(X, "cityblock"))
    ties = 0
    for K in range(1, len(X) + 1):
        ref = pam_ref(D, K)
        ties += ref.ties
        est = PAM(n_clusters=K, metric="manhattan").fit(X)
        np.testing.assert_array_equal(est.medoid_indices_, ref.medoids, err_msg=f"K={K}")
        np.testing.assert_array_equal(est.labels_, ref.labels, err_msg=f"K={K}")
        assert (est.n_iter_, est.inertia_) == (ref.n_iter, ref.inertia), K
    assert ties > 100  # the input does exercise the tie rules


def test_max_iter():
    X = np.random.RandomState(3).randn(60, 3)
    D = squareform(pdist(X))
    full = PAM(n_clusters=6).fit(X)
    assert full.n_iter_ >= 2  # the seed is chosen so that SWAP has work to do
    b = PAM(n_clusters=6, max_iter=0).fit(X)
    assert b.n_iter_ == 0
    np.testing.assert_array_equal(b.medoid_indices_, sorted(P.build(D, 6)))
    one = PAM(n_clusters=6, max_iter=1).fit(X)
    ref = pam_ref(D, 6, max_iter=1)
    assert one.n_iter_ == ref.n_iter == 1
    np.testing.assert_array_equal(one.medoid_indices_, ref.medoids)
    assert full.inertia_ < one.inertia_ < b.inertia_


def test_estimator_protocol():
    est = PAM(n_clusters=3, metric="cosine", max_iter=7)
    assert est.get_params() == dict(n_clusters=3, metric="cosine", max_iter=7)
    c = clone(est)
    assert type(c) is PAM and c is not est and c.get_params() == est.get_params()
    assert est.set_params(n_clusters=4, max_iter=9) is est and (est.n_clusters, est.max_iter) == (4, 9)
    with pytest.raises(ValueError, match="Invalid parameter 'random_state'"):
        est.set_params(random_state=0)
    assert "random_state" not in est.get_params()
    X = np.random.RandomState(0).randn(20, 3)
    est.fit(X)
    back = pickle.loads(pickle.dumps(est))
    np.testing.assert_array_equal(back.labels_, est.labels_)
    np.testing.assert_array_equal(back.fit_predict(X), est.labels_)
    assert clone(SubPAM(n_clusters=2)).get_params()["n_clusters"] == 2
    assert consensus_clustering_amd.PAM is PAM


def test_the_module_does_not_import_torch():
    import subprocess

    code = ("import sys; import consensus_clustering_amd.pam, consensus_clustering_amd._hostfit; "
            "from consensus_clustering_amd import PAM; assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=api.os.path.dirname(api.os.path.dirname(api.__file__)))


def test_pam_spec():
    assert api._pam_spec(PAM()) == "euclidean"
    assert api._pam_spec(PAM(metric="l1")) == "cityblock"
    assert api._pam_spec(PAM(metric="manhattan", max_iter=0)) == "cityblock"
    assert api._pam_spec(PAM(metric="correlation")) == "correlation"
    assert api._pam_spec(SubPAM()) is None
    assert api._pam_spec(PAM(metric="chebyshev")) is None
    assert api._pam_spec(PAM(max_iter=-1)) is None
    assert api._pam_spec(KMeans()) is None
    X = np.random.RandomState(0).randn(6, 3)
    Xz = X.copy()
    Xz[2] = 0.0
    assert api._pam_route("cosine", X) == "cosine" and api._pam_route("cosine", Xz) is None
    assert api._pam_route("euclidean", Xz) == "euclidean" and api._pam_route("cosine", None) == "cosine"
    Xz[2] = 1.5
    assert api._pam_route("correlation", Xz) is None


def test_refusals():
    X = np.random.RandomState(0).randn(8, 3)
    Xn, Xi, Xz, Xc = X.copy(), X.astype(np.float32), X.copy(), X.copy()
    Xn[1, 1] = np.nan
    Xi[2, 0] = np.inf
    Xz[4] = 0.0
    Xc[3] = 1.5
    with pytest.raises(ValueError, match=r"Input X contains NaN\."):
        PAM(2).fit(Xn)
    with pytest.raises(ValueError, match=r"Input X contains infinity or a value too large for dtype\('float32'\)\."):
        PAM(2).fit(Xi)
    with pytest.raises(ValueError, match=r"Found array with 1 sample\(s\) \(shape=\(1, 3\)\) while a minimum of 2 is "
                                         "required by PAM"):
        PAM(1).fit(X[:1])
    with pytest.raises(ValueError, match="Cannot extract more clusters than samples: 9 clusters were given for 8 "
                                         "samples"):
        PAM(9).fit(X)
    with pytest.raises(ValueError, match="Cosine affinity cannot be used when X contains zero vectors"):
        PAM(2, metric="cosine").fit(Xz)
    with pytest.raises(ValueError, match="row 3 is constant"):
        PAM(2, metric="correlation").fit(Xc)
    PAM(2, metric="manhattan").fit(Xz)  # a zero row is degenerate under cosine alone
    with pytest.raises(ValueError, match="'n_clusters' parameter of PAM"):
        PAM(0).fit(X)
    with pytest.raises(ValueError, match="'max_iter' parameter of PAM"):
        PAM(2, max_iter=-1).fit(X)
    with pytest.raises(ValueError, match="'metric' parameter of PAM"):
        PAM(2, metric="chebyshev").fit(X)
    with pytest.raises(ValueError, match="euclidean distances between the rows of X are not all finite"):
        PAM(2).fit(np.array([[1e200, 0.0], [-1e200, 0.0], [0.0, 1.0]]) * 1e108)


def test_pam_plan_arithmetic():
    n, m, nh, nK, Kmax = 1000, 800, 60, 6, 7
    per = engine.pam_tree_bytes(m, nK, Kmax)
    assert per > 8 * m * m + nK * 52 * m
    full = 8 * n * n
    assert engine.pam_plan(n, m, nh, nK, Kmax, full + 1000 * per) == 60
    assert engine.pam_plan(n, m, nh, nK, Kmax, full + 20 * per + per // 2) == 20
    assert engine.pam_plan(n, m, nh, nK, Kmax, full + per) == 1
    assert engine.pam_plan(n, m, 3, nK, Kmax, full + 1000 * per) == 3
    with pytest.raises(ValueError, match="cannot hold the PAM clusterer: the n x n"):
        engine.pam_plan(n, m, nh, nK, Kmax, full + per - 1)
    md = 12
    perf = per + engine.hc_feature_bytes(m, md)
    assert engine.pam_plan(n, m, nh, nK, Kmax, 2 * perf, md=md) == 2
    with pytest.raises(ValueError, match="cannot hold the PAM clusterer: one tree"):
        engine.pam_plan(n, m, nh, nK, Kmax, perf - 1, md=md)


def test_host_loop_with_a_subclass_does_not_depend_on_n_jobs():
    rs = np.random.RandomState(4)
    X = rs.randn(50, 4).astype(np.float32)
    idx = np.stack([rs.permutation(50)[:40] for _ in range(6)])
    est = SubPAM(n_clusters=3, metric="correlation")
    serial = api.host_fit_predict(est, X, idx, 1)
    assert serial.shape == (6, 40) and serial.dtype == np.int32
    for h in range(6):
        np.testing.assert_array_equal(serial[h], PAM(3, metric="correlation").fit_predict(X[idx[h]]))
    np.testing.assert_array_equal(api.host_fit_predict(est, X, idx, 2), serial)
    np.testing.assert_array_equal(api.host_fit_predict(est, X, idx, 2, "multiprocessing"), serial)
