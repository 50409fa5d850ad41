"""The hierarchical base clusterer's manhattan, cosine and correlation metrics on the device
(cc_pdist): the distances against scipy's pdist bit for bit, the trees over them against scipy's
linkage exactly, and whole fits against the oracle with the same sklearn estimator as its
clusterer and against the host loop.  tests/test_hc_metrics_host.py holds the recipes to the
installed scipy on the CPU."""
import functools

import numpy as np
import pytest
import torch
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import pdist, squareform
from sklearn.cluster import AgglomerativeClustering

from consensus_clustering_amd import ConsensusClustering, _lib, engine, post
from oracle import cc_oracle as O
from tests.conftest import load_fixture

pytestmark = pytest.mark.gpu

METRICS = ["cityblock", "cosine", "correlation"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _scipy(X, metric):
    with np.errstate(invalid="ignore", divide="ignore"):
        return squareform(pdist(X, metric))


# ---------------------------------------------------------------- distances

SHAPES = [(257, 37, np.float32), (65, 150, np.float32), (200, 12, np.float64), (64, 16, np.float64),
          (63, 17, np.float64), (129, 33, np.float64), (2, 3, np.float64), (70, 32, np.float32),
          (130, 1, np.float32), (40, 2, np.float64)]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,d,dtype", SHAPES)
def test_pdist_equals_scipy_bit_for_bit(n, d, dtype, metric):
    """Tile (64) and k slab (16) edges, exactly one of each, the odd last column alone (d = 1:
    correlation is NaN off the diagonal there, and equal NaNs compare equal), after one slab and
    after two, one pair of lanes with no tail, both dtypes."""
    X = np.random.RandomState(n + d).randn(n, d).astype(dtype)
    got = engine.pdist(_dev(X), metric).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (n, n)
    np.testing.assert_array_equal(got, _scipy(X, metric))
    np.testing.assert_array_equal(got, got.T)
    np.testing.assert_array_equal(np.diag(got), 0.0)


def test_pdist_euclidean_is_cc_euclidean():
    X = np.random.RandomState(5).randn(70, 9).astype(np.float32)
    np.testing.assert_array_equal(engine.pdist(_dev(X), "euclidean").cpu().numpy(), _scipy(X, "euclidean"))


def test_pdist_refuses_unknown_metrics():
    X = _dev(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match="metric must be one of"):
        engine.pdist(X, "chebyshev")
    D = torch.empty((4, 4), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.CCMIError, match="unknown metric 7"):
        _lib.call("cc_pdist", X.data_ptr(), 0, 4, 3, 7, D.data_ptr(), None, engine.stream_ptr())
    with pytest.raises(_lib.CCMIError, match="needs norms"):
        _lib.call("cc_pdist", X.data_ptr(), 0, 4, 3, 2, D.data_ptr(), None, engine.stream_ptr())


def test_cosine_clip():
    """Rows, the same rows again and their negatives: cosines of magnitude 1 up to rounding, which
    the clip turns into exact 0 and 2."""
    R = np.random.RandomState(0).randn(20, 7)
    X = np.concatenate([R, R, -R])
    got = engine.pdist(_dev(X), "cosine").cpu().numpy()
    np.testing.assert_array_equal(got, _scipy(X, "cosine"))
    assert (got[np.triu_indices(60, 1)] == 0.0).any() and (got == 2.0).any()
    assert got.min() == 0.0 and got.max() == 2.0


# ---------------------------------------------------------------- trees

def _trees(X, idx, link, metric):
    D = engine.pdist(_dev(X), metric)
    Db = engine.hc_gather(D, _dev(idx))
    Z = engine.hc_nnchain_batched(Db, link).cpu().numpy()
    return [post.linkage_finish(Z[b], idx.shape[1]) for b in range(len(idx))]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("link", ["average", "complete"])
@pytest.mark.parametrize("m", [2, 3, 33])
def test_trees_equal_scipy(m, link, metric):
    rs = np.random.RandomState(m)
    n, B = m + 7, 3
    X = rs.randn(n, 5).astype(np.float32)
    idx = np.stack([rs.permutation(n)[:m] for _ in range(B)]).astype(np.int32)
    for b, Z in enumerate(_trees(X, idx, link, metric)):
        np.testing.assert_array_equal(Z, linkage(X[idx[b]], link, metric), err_msg=f"tree {b}")


@pytest.mark.parametrize("link", ["average", "complete"])
def test_trees_with_ties(link):
    """An integer lattice with every row twice, under cityblock: equal distances everywhere."""
    rs = np.random.RandomState(1)
    half = rs.randint(0, 3, size=(32, 2)).astype(np.float64)
    X = np.concatenate([half, half])
    idx = np.stack([rs.permutation(64) for _ in range(3)]).astype(np.int32)
    for b, Z in enumerate(_trees(X, idx, link, "cityblock")):
        np.testing.assert_array_equal(Z, linkage(X[idx[b]], link, "cityblock"), err_msg=f"tree {b}")


# ---------------------------------------------------------------- end to end

E2E = dict(K_range=list(range(2, 8)), n_iterations=24, subsampling=0.8, random_state=3)
CASES = [("average", "correlation", "correlation"), ("complete", "cosine", "cosine"),
         ("average", "manhattan", "cityblock")]


@functools.lru_cache(maxsize=None)
def _e2e_X(dtype):
    return np.ascontiguousarray(load_fixture("blobs_n400_d8_k4")["X"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def _e2e_fit(link, metric, dtype, hierarchical="auto"):
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage=link, metric=metric), clusterer_options={},
                             plot_cdf=False, hierarchical=hierarchical, **E2E)
    return cc.fit(_e2e_X(dtype))


def _assert_same_results(a, b):
    for K in E2E["K_range"]:
        for key in ("mij", "iij", "cij", "hist", "cdf", "bin_edges"):
            np.testing.assert_array_equal(a.cdf_at_K_data[K][key], b.cdf_at_K_data[K][key], err_msg=f"{key} K={K}")
        assert a.cdf_at_K_data[K]["pac_area"] == b.cdf_at_K_data[K]["pac_area"]
        np.testing.assert_array_equal(a.pair_counts_[K], b.pair_counts_[K])
    assert a.best_k_ == b.best_k_


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("link,metric,canonical", CASES)
def test_fit_equals_oracle_and_host(link, metric, canonical, dtype):
    X = _e2e_X(dtype)
    n = X.shape[0]
    cc = _e2e_fit(link, metric, dtype)
    assert cc.backend_ == "gpu-hc" and cc.hc_metric_ == canonical
    assert cc.hc_stats_["route"] == "batched" and cc.hc_stats_["batch"] == E2E["n_iterations"]
    ref, _ = O.fit(X, E2E["K_range"], E2E["n_iterations"], E2E["subsampling"], E2E["random_state"],
                   clusterer=lambda Xs, K: AgglomerativeClustering(n_clusters=K, linkage=link,
                                                                   metric=metric).fit_predict(Xs))
    for K in E2E["K_range"]:
        d, r = cc.cdf_at_K_data[K], ref[K]
        np.testing.assert_array_equal(d["mij"], r["mij"], err_msg=f"K={K}")
        np.testing.assert_array_equal(d["iij"], r["iij"])
        np.testing.assert_array_equal(post.pair_counts_to_hist_counts(cc.pair_counts_[K], n),
                                      O.bin_counts(r["cij"]), err_msg=f"K={K}")
        np.testing.assert_array_equal(d["hist"], r["hist"], err_msg=f"K={K}")
        np.testing.assert_array_equal(d["cdf"], r["cdf"], err_msg=f"K={K}")
        assert d["pac_area"] == r["pac_area"], K
        assert np.max(np.abs(d["cij"] - r["cij"])) <= 1e-6
    host = _e2e_fit(link, metric, dtype, "host")
    assert host.backend_ == "host-clusterer" and host.hc_stats_ is None and host.hc_metric_ is None
    _assert_same_results(cc, host)


def test_fit_on_a_device_tensor_with_correlation():
    """X already in device memory (copied to the host for the centring) gives the host array's
    results."""
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="average", metric="correlation"),
                             clusterer_options={}, plot_cdf=False, **E2E)
    cc.fit(torch.from_numpy(_e2e_X(np.float32)).cuda())
    assert cc.backend_ == "gpu-hc" and cc.hc_metric_ == "correlation"
    _assert_same_results(cc, _e2e_fit("average", "correlation", np.float32))


def test_refusals():
    X = _e2e_X(np.float32)
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="ward", metric="manhattan"),
                             clusterer_options={}, plot_cdf=False, hierarchical="device", **E2E)
    with pytest.raises(ValueError, match="hierarchical='device'"):
        cc.fit(X)
    Xz = X.copy()
    Xz[0] = 0.0
    sentence = "Cosine affinity cannot be used when X contains zero vectors"
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="average", metric="cosine"),
                             clusterer_options={}, plot_cdf=False, hierarchical="device", **E2E)
    with pytest.raises(ValueError, match=sentence):
        cc.fit(Xz)
    # 'auto': the host loop, where sklearn refuses the first resample that holds row 0 (24
    # resamples of 80 %: one of them does)
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="average", metric="cosine"),
                             clusterer_options={}, plot_cdf=False, **E2E)
    with pytest.raises(ValueError, match=sentence):
        cc.fit(Xz)
    assert cc.backend_ == "host-clusterer" and cc.hc_metric_ is None
    Xc = X.copy()
    Xc[3] = 1.5
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="average", metric="correlation"),
                             clusterer_options={}, plot_cdf=False, hierarchical="device", **E2E)
    with pytest.raises(ValueError, match="row 3 is constant"):
        cc.fit(Xc)
