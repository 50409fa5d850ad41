"""Hierarchical base clusterer on the device (cc_euclidean, cc_hc_gather, cc_hc_nnchain_batched,
cc_hc_cut): every stage against scipy / sklearn on the host, exactly, and the whole fit against
the oracle with AgglomerativeClustering as its clusterer.  Every batched run goes through
cc_hc_check, so a tree with a set status word fails the test that ran it
(test_check_reads_every_status_word shows that it does).  The trees and cuts that only large m
reach (state or links in the workspace, a second row pass) and the deep synthetic trees of
tests/hc_ref.py are here too."""
import functools

import numpy as np
import pytest
import torch
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import pdist, squareform
from sklearn.cluster import AgglomerativeClustering

from consensus_clustering_amd import ConsensusClustering, _lib, engine, post
from oracle import cc_oracle as O
from tests import hc_ref
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


@pytest.mark.parametrize("n,d,dtype", [(1, 1, np.float32), (2, 3, np.float64), (64, 16, np.float64),
                                       (63, 17, np.float64), (129, 33, np.float64)])
def test_euclidean_at_the_edges(n, d, dtype):
    """A single row (one tile, one stored entry), two rows, exactly one tile of exactly one k slab,
    one row and one k short of / past them, and a third tile row with a third k slab of one."""
    X = np.random.RandomState(n + d).randn(n, d).astype(dtype)
    got = engine.euclidean(_dev(X)).cpu().numpy()
    np.testing.assert_array_equal(got, squareform(pdist(X, "euclidean")))
    np.testing.assert_array_equal(got, got.T)
    np.testing.assert_array_equal(np.diag(got), 0.0)


def _gather_case(n, m, B):
    rs = np.random.RandomState(0)
    D = rs.rand(n, n)
    idx = np.stack([rs.permutation(n)[:m] for _ in range(B)]).astype(np.int32)
    got = engine.hc_gather(_dev(D), _dev(idx)).cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(got[b], D[idx[b]][:, idx[b]])


def test_gather_equals_fancy_indexing():
    _gather_case(50, 33, 3)


def test_gather_second_column_block():
    """m = 300: a second 256-wide column block with a ragged edge."""
    _gather_case(400, 300, 2)


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


@pytest.mark.parametrize("m,link", [(6050, "complete"), (8195, "ward"), (8195, "average"), (8195, "complete")])
def test_batched_nn_chain_large_trees_equal_scipy(m, link):
    """The two paths of the batched nn_chain that only a large tree takes: where hclust.hip's
    nnchain_batched_kernel puts the chain state, and the second row pass of the shared loop
    (cc_link::nn_chain, linkage_shared.hpp).

    Chain state in the workspace: state_in_lds(m) asks 4 ceil(m / 32) bytes of live mask plus 8 m
    bytes of sizes and chain to fit HC_LDS_STATE_MAX = 49152.  m = 6049 has 190 mask words,
    760 + 48392 = 49152, the last m in LDS; m = 6050 takes 49160 bytes, the first whose
    size[] / chain[] sit in global memory at state + b * 2 * m.

    A second row pass: row_argmin<T, NBH> and the Lance-Williams loop step by T * NBH =
    HC_T_LARGE * NBH = 1024 * 8 = 8192 slots, so m <= 8192 is one pass and m = 8193 the first
    with two; m = 8195 puts three leaves (not one lane's worth) into the second pass.  Ward is the
    method whose update reads size[i] there.

    Two trees: the second one's state is at a non-zero offset.  Against scipy, exactly."""
    rs = np.random.RandomState(m)
    n, B = m + 7, 2
    X = rs.randn(n, 5).astype(np.float32)
    idx = np.stack([rs.permutation(n)[:m] for _ in range(B)]).astype(np.int32)
    trees = _trees(X, idx, link)
    torch.cuda.empty_cache()  # about 1.6 GB of distances at m = 8195
    for b, Z in enumerate(trees):
        np.testing.assert_array_equal(Z, linkage(X[idx[b]], link, "euclidean"), err_msg=f"tree {b}")


def test_check_reads_every_status_word():
    """cc_hc_check over more trees than one of its 1024-word chunks: 1030 trees of three leaves.
    All finite: the trees on both sides of the chunk edge equal scipy.  A tree whose distances
    are all +inf finds no neighbour (the loop's defined error return in every form: the scan's sentinel is
    refused before anything is indexed), and the call raises naming the first such tree, also
    when that tree's status word lies in the second chunk."""
    rs = np.random.RandomState(7)
    B, m = 1030, 3
    P = rs.rand(B, m, 2)
    Db = np.stack([squareform(pdist(P[b], "euclidean")) for b in range(B)])
    Z = engine.hc_nnchain_batched(_dev(Db), "average").cpu().numpy()
    for b in (0, 1023, 1024, 1029):
        np.testing.assert_array_equal(post.linkage_finish(Z[b], m), linkage(P[b], "average", "euclidean"),
                                      err_msg=f"tree {b}")
    off = ~np.eye(m, dtype=bool)
    for trees, first in (((1027,), 1027), ((5, 1027), 5)):
        bad = Db.copy()
        for b in trees:
            bad[b][off] = np.inf
        with pytest.raises(_lib.CCMIError, match=f"tree {first} found no neighbour"):
            engine.hc_nnchain_batched(_dev(bad), "average")


# ---------------------------------------------------------------- cut

def _cut_synthetic(m, Zs, Ks, seed):
    """cc_hc_cut alone on the raw merges Zs (one tree each) against hc_ref.reference_cut: leaf r
    of tree b is item idx[b, r] of n > m, the trees fill columns [3, 3 + B) of 128, and the
    whole label matrix is compared, so every cell the call does not own must still be 0xFF."""
    rs = np.random.RandomState(seed)
    B, n, h_begin = len(Zs), m + 9, 3
    idx = np.stack([rs.permutation(n)[:m] for _ in range(B)]).astype(np.int32)
    L = engine.new_label_matrix(len(Ks), n, engine.pad_h(8), "cuda")
    engine.hc_cut(_dev(np.stack(Zs)), _dev(idx), torch.tensor(Ks, dtype=torch.int32, device="cuda"), h_begin, L)
    want = np.full((len(Ks), n, engine.pad_h(8)), 0xFF, dtype=np.uint8)
    for b, Z in enumerate(Zs):
        for k, K in enumerate(Ks):
            ref = hc_ref.reference_cut(Z, m, K)
            assert sorted(set(ref.tolist())) == list(range(K))
            if K == m:  # every leaf alone: its id is its slot's rank
                np.testing.assert_array_equal(ref, np.arange(m))
            want[k, idx[b], h_begin + b] = ref
    np.testing.assert_array_equal(L.cpu().numpy(), want)


def _synthetic_pair(m, kind, ties=False):
    """Two trees of one kind with different merges: a caterpillar with increasing distances
    (the cut keeps the bottom of the chain) and with decreasing ones (it keeps the top); two
    draws of random merges, with distances in [0, 4) for ties."""
    rs = np.random.RandomState(m)
    Zs = [hc_ref.synthetic_merges(m, kind, rs) for _ in range(2)]
    if kind != "random":
        Zs[1][:, 2] = Zs[1][::-1, 2].copy()
    if ties:
        for Z in Zs:
            Z[:, 2] = rs.randint(0, 4, size=m - 1)
    return Zs


@pytest.mark.parametrize("kind", ["chain", "bypass", "random"])
@pytest.mark.parametrize("m", [2, 3, 63, 64, 65, 1023, 1024, 1025])
def test_cut_of_synthetic_trees(kind, m):
    """ceil(log2 m) rounds of pointer jumping on both sides of a power of two; the caterpillars
    (slot j dies into j + 1) are m - 1 and m - 2 links deep, which no tree of blob data is.  A
    round too few shows in 'bypass' at K = 2 (tests/hc_ref.py says why not in 'chain') where
    ceil(log2 (m - 2)) = ceil(log2 m): m = 63, 64, 1023, 1024; at 2^p + 1 the kernel has a round
    to spare."""
    Ks = sorted({K for K in (1, 2, 3, 5, min(m, 127)) if K <= m})
    _cut_synthetic(m, _synthetic_pair(m, kind), Ks, m)


@pytest.mark.parametrize("kind", ["chain", "bypass", "random"])
def test_cut_at_k_equal_to_m(kind):
    """K = m = 127 keeps no merge: every leaf's id is its slot; K = m - 1 keeps one."""
    _cut_synthetic(127, _synthetic_pair(127, kind), [1, 126, 127], 127)


def test_cut_ranks_tied_distances_stably():
    _cut_synthetic(300, _synthetic_pair(300, "random", ties=True), [1, 2, 3, 5, 127], 300)


@pytest.mark.parametrize("kind", ["chain", "bypass", "random"])
@pytest.mark.parametrize("m", [11915, 11916])
def test_cut_with_links_in_lds_and_in_the_workspace(kind, m):
    """link_in_lds(m) asks 4 ceil(m / 32) bytes of root mask plus 4 m bytes of links to fit
    HC_LDS_LINK_MAX = 49152: m = 11915 has 373 mask words, 1492 + 47660 = 49152, the last m with
    the links in LDS; m = 11916 is the first that jumps pointers in global memory, at
    links + (b * nK + k) * m.  The caterpillars there are the deep trees on that path, and need
    every one of its ceil(log2 m) = 14 rounds (2^13 < m - 2)."""
    _cut_synthetic(m, _synthetic_pair(m, kind), [1, 2, 7, 127], m)


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


def test_planner_split_with_a_short_last_batch():
    """A budget for two trees and five resamples: hc_labels itself launches 2, 2 and 1 trees on
    a workspace sized for two, and fills the labels of the one-launch run."""
    X, idx = _cut_case()
    n = X.shape[0]
    per = engine.hc_tree_bytes(idx.shape[1], len(CUT_KS))
    L = engine.new_label_matrix(len(CUT_KS), n, engine.pad_h(len(idx)), "cuda")
    stats = engine.hc_labels(engine.euclidean(_dev(X)), _dev(idx), 0, 5, CUT_KS, "ward", L,
                             budget=8 * n * n + 2 * per + per // 2)
    assert stats == dict(route="batched", batch=2, launches=3)
    np.testing.assert_array_equal(L.cpu().numpy(), _labels_for("ward", [(0, 5)]))


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
