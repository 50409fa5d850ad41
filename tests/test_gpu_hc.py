"""Hierarchical base clusterer on the device (cc_euclidean, cc_hc_gather, cc_hc_nnchain_batched,
cc_hc_cut): every stage against scipy / sklearn on the host, exactly, and the whole fit against
the oracle with AgglomerativeClustering as its clusterer.  Every batched run goes through
cc_hc_check, so a tree with a set status word fails the test that ran it."""
import functools

import numpy as np
import pytest
import torch
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import pdist, squareform
from sklearn.cluster import AgglomerativeClustering

from consensus_clustering_amd import ConsensusClustering, engine, post
from oracle import cc_oracle as O
from tests.conftest import load_fixture

pytestmark = pytest.mark.gpu

LINKS = ["ward", "average", "complete"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- distances, gather

@pytest.mark.parametrize("n,d,dtype", [(257, 37, np.float32), (130, 1, np.float32), (65, 150, np.float32),
                                       (200, 12, np.float64)])
def test_euclidean_equals_pdist_bit_for_bit(n, d, dtype):
    """One tile (64), a tile edge, d below, at and across the k slab (16), both dtypes."""
    X = np.random.RandomState(n + d).randn(n, d).astype(dtype)
    got = engine.euclidean(_dev(X)).cpu().numpy()
    np.testing.assert_array_equal(got, squareform(pdist(X, "euclidean")))
    np.testing.assert_array_equal(got, got.T)
    np.testing.assert_array_equal(np.diag(got), 0.0)


def test_euclidean_k_slab_edge():
    """d exactly one and exactly two k slabs."""
    for d in (16, 32):
        X = np.random.RandomState(d).randn(70, d).astype(np.float32)
        np.testing.assert_array_equal(engine.euclidean(_dev(X)).cpu().numpy(), squareform(pdist(X, "euclidean")))


def test_gather_equals_fancy_indexing():
    rs = np.random.RandomState(0)
    n, m, B = 50, 33, 3
    D = rs.rand(n, n)
    idx = np.stack([rs.permutation(n)[:m] for _ in range(B)]).astype(np.int32)
    got = engine.hc_gather(_dev(D), _dev(idx)).cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(got[b], D[idx[b]][:, idx[b]])


# ---------------------------------------------------------------- batched nn_chain

def _trees(X, idx, link):
    """Finished linkage matrices of the device trees over X[idx[b]]."""
    D = engine.euclidean(_dev(X))
    Db = engine.hc_gather(D, _dev(idx))
    Z = engine.hc_nnchain_batched(Db, link).cpu().numpy()
    return [post.linkage_finish(Z[b], idx.shape[1]) for b in range(len(idx))]


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("m", [2, 3, 33, 1025])
def test_batched_nn_chain_equals_scipy(link, m):
    """m = 1025: the 1024-thread form, one leaf more than a pass (and than the 256-thread form's
    last m); 2, 3, 33: the 256-thread form.  Children, distances and sizes, exactly."""
    rs = np.random.RandomState(m)
    n, B = m + 7, 3
    X = rs.randn(n, 5).astype(np.float32)
    idx = np.stack([rs.permutation(n)[:m] for _ in range(B)]).astype(np.int32)
    for b, Z in enumerate(_trees(X, idx, link)):
        np.testing.assert_array_equal(Z, linkage(X[idx[b]], link, "euclidean"), err_msg=f"tree {b}")


@pytest.mark.parametrize("link", LINKS)
def test_batched_nn_chain_with_ties(link):
    """An integer lattice with every row twice: equal distances everywhere, so the first-minimum
    scan, the previous chain element's precedence and the stable sort all decide."""
    rs = np.random.RandomState(1)
    half = rs.randint(0, 3, size=(32, 2)).astype(np.float64)
    X = np.concatenate([half, half])
    idx = np.stack([rs.permutation(64) for _ in range(3)]).astype(np.int32)
    for b, Z in enumerate(_trees(X, idx, link)):
        np.testing.assert_array_equal(Z, linkage(X[idx[b]], link, "euclidean"), err_msg=f"tree {b}")


# ---------------------------------------------------------------- cut

CUT_KS = list(range(1, 10)) + [127]


@functools.lru_cache(maxsize=None)
def _cut_case():
    rs = np.random.RandomState(4)
    n, d, H = 300, 8, 5
    centers = rs.uniform(-6, 6, size=(4, d))
    X = (centers[rs.randint(0, 4, n)] + rs.randn(n, d)).astype(np.float32)
    idx = engine.resample_indices(11, n, 240, 0, H)
    return X, idx


def _labels_for(link, ranges, route="auto"):
    X, idx = _cut_case()
    n, H = X.shape[0], len(idx)
    D = engine.euclidean(_dev(X))
    L = engine.new_label_matrix(len(CUT_KS), n, engine.pad_h(H), "cuda")
    for a, b in ranges:
        engine.hc_labels(D, _dev(idx), a, b, CUT_KS, link, L, route=route)
    return L.cpu().numpy()


def _same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len({p for p, _ in pairs}) == len({q for _, q in pairs})


@pytest.mark.parametrize("link", LINKS)
def test_cut_equals_sklearn_fit_predict(link):
    X, idx = _cut_case()
    L = _labels_for(link, [(0, 5)])
    for h in range(len(idx)):
        unsampled = np.setdiff1d(np.arange(X.shape[0]), idx[h])
        assert (L[:, unsampled, h] == 0xFF).all()
        for k, K in enumerate(CUT_KS):
            got = L[k, idx[h], h]
            assert sorted(set(got.tolist())) == list(range(K)), (h, K)  # ids in [0, K), all used
            want = AgglomerativeClustering(n_clusters=K, linkage=link).fit_predict(X[idx[h]])
            assert _same_partition(got, want), (h, K)
    assert (L[:, :, len(idx):] == 0xFF).all()  # the padding columns stay unsampled


def test_range_split_and_routes_agree():
    """Resamples [0, 5) in one call = [0, 2) + [2, 5) in two = one tree at a time through
    cc_linkage_nnchain (CC_LINK_WARD)."""
    whole = _labels_for("ward", [(0, 5)])
    np.testing.assert_array_equal(_labels_for("ward", [(0, 2), (2, 5)]), whole)
    np.testing.assert_array_equal(_labels_for("ward", [(0, 5)], route="sequential"), whole)


# ---------------------------------------------------------------- end to end

E2E = dict(K_range=list(range(2, 8)), n_iterations=24, subsampling=0.8, random_state=3)


@functools.lru_cache(maxsize=None)
def _e2e_X(dtype):
    return np.ascontiguousarray(load_fixture("blobs_n400_d8_k4")["X"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def _e2e_fit(link, dtype, hierarchical="auto", budget=None):
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage=link), clusterer_options={},
                             plot_cdf=False, hierarchical=hierarchical, workspace_budget=budget, **E2E)
    return cc.fit(_e2e_X(dtype))


def _assert_same_results(a, b):
    for K in E2E["K_range"]:
        for key in ("mij", "iij", "cij", "hist", "cdf", "bin_edges"):
            np.testing.assert_array_equal(a.cdf_at_K_data[K][key], b.cdf_at_K_data[K][key], err_msg=f"{key} K={K}")
        assert a.cdf_at_K_data[K]["pac_area"] == b.cdf_at_K_data[K]["pac_area"]
        np.testing.assert_array_equal(a.pair_counts_[K], b.pair_counts_[K])
    assert a.best_k_ == b.best_k_


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("link", LINKS)
def test_fit_equals_oracle_and_host(link, dtype):
    X = _e2e_X(dtype)
    n = X.shape[0]
    cc = _e2e_fit(link, dtype)
    assert cc.backend_ == "gpu-hc"
    assert cc.hc_stats_["route"] == "batched" and cc.hc_stats_["batch"] == E2E["n_iterations"]
    assert cc.kmeans_inertia_ is None and cc.kmeans_n_iter_ is None and cc.kmeans_stats_ is None
    assert set(cc.timings_) == {"resample", "cluster", "coassoc", "post", "total"}
    ref, _ = O.fit(X, E2E["K_range"], E2E["n_iterations"], E2E["subsampling"], E2E["random_state"],
                   clusterer=lambda Xs, K: AgglomerativeClustering(n_clusters=K, linkage=link).fit_predict(Xs))
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
    host = _e2e_fit(link, dtype, "host")
    assert host.backend_ == "host-clusterer" and host.hc_stats_ is None
    _assert_same_results(cc, host)
    lab = cc.predict()
    assert lab.shape == (n,) and len(set(lab.tolist())) == cc.best_k_
    icl = cc.icl([cc.best_k_])[cc.best_k_]
    assert icl["item_consensus"].shape == (n, cc.best_k_)


def test_fit_sequential_route_under_a_one_tree_budget():
    """A budget with room for the distances and one tree: the resamples go one at a time through
    cc_linkage_nnchain with CC_LINK_WARD, and give the batched fit's results."""
    n = _e2e_X(np.float32).shape[0]
    m = int(E2E["subsampling"] * n)
    budget = 8 * n * n + engine.hc_tree_bytes(m, len(E2E["K_range"])) + 100
    cc = _e2e_fit("ward", np.float32, "device", budget)
    assert cc.backend_ == "gpu-hc" and cc.hc_stats_ == dict(route="sequential", batch=1, launches=24)
    _assert_same_results(cc, _e2e_fit("ward", np.float32))


def test_fit_on_a_device_tensor():
    """X already in device memory gives the host array's results."""
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="average"), clusterer_options={},
                             plot_cdf=False, **E2E).fit(torch.from_numpy(_e2e_X(np.float32)).cuda())
    assert cc.backend_ == "gpu-hc"
    _assert_same_results(cc, _e2e_fit("average", np.float32))


def test_device_is_refused_for_other_estimators_and_small_budgets():
    X = _e2e_X(np.float32)
    Xn = X.copy()
    Xn[5, 2] = np.nan  # refused from the host array: no distance or tree kernel sees it
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(), clusterer_options={}, plot_cdf=False, **E2E)
    with pytest.raises(ValueError, match=r"Input X contains NaN\."):
        cc.fit(Xn)
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="single"), clusterer_options={},
                             plot_cdf=False, hierarchical="device", **E2E)
    with pytest.raises(ValueError, match="hierarchical='device'"):
        cc.fit(X)
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(), clusterer_options={}, plot_cdf=False,
                             workspace_budget=1 << 20, **E2E)
    with pytest.raises(ValueError, match="workspace_budget = 1048576"):
        cc.fit(X)
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(), clusterer_options={}, plot_cdf=False,
                             K_range=[2, 9], n_iterations=4, random_state=0)
    with pytest.raises(ValueError, match="Cannot extract more clusters than samples: 9 clusters were given "
                                         "for a tree with 8 leaves"):
        cc.fit(X[:10])
