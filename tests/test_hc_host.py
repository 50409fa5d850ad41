"""Host side of the hierarchical base clusterer (no GPU): which estimators are routed to the
device trees, ``_set_clusterer_K`` on an estimator without ``random_state``, sklearn's refusals
raised from host values, the batch planner, and the reference cut of tests/hc_ref.py that the
device cut is held to."""
import numpy as np
import pytest
from sklearn.cluster import AgglomerativeClustering, KMeans

from consensus_clustering_amd import ConsensusClustering, api, engine


@pytest.mark.parametrize("link", ["ward", "average", "complete"])
def test_predicate_true_for_euclidean_linkages(link):
    assert api._is_device_hierarchical(AgglomerativeClustering(linkage=link))
    assert api._hc_linkage(AgglomerativeClustering(linkage=link, metric="euclidean")) == link
    if link != "ward":  # sklearn itself refuses ward with any other spelling at fit time
        assert api._is_device_hierarchical(AgglomerativeClustering(linkage=link, metric="l2"))


class _Sub(AgglomerativeClustering):
    pass


@pytest.mark.parametrize("est", [
    AgglomerativeClustering(linkage="single"),
    AgglomerativeClustering(linkage="average", metric="manhattan"),
    AgglomerativeClustering(linkage="ward", connectivity=np.eye(4)),
    AgglomerativeClustering(linkage="average", distance_threshold=1.0, n_clusters=None),
    _Sub(linkage="average"),
    KMeans(),
], ids=["single", "manhattan", "connectivity", "distance_threshold", "subclass", "kmeans"])
def test_predicate_false(est):
    assert not api._is_device_hierarchical(est)
    assert api._hc_linkage(est) is None


def test_clusterer_options_are_honoured_by_the_predicate():
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="single"),
                             clusterer_options={"linkage": "average"}, K_range=[3], random_state=0,
                             plot_cdf=False)
    assert not api._is_device_hierarchical(cc.clusterer)
    assert cc._kmeans_params() is None  # applies the options, as fit does before routing
    assert api._hc_linkage(cc.clusterer) == "average"
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="ward"),
                             clusterer_options={"linkage": "single"}, K_range=[3], random_state=0,
                             plot_cdf=False)
    cc._kmeans_params()
    assert not api._is_device_hierarchical(cc.clusterer)


def test_set_clusterer_k_without_random_state():
    est = AgglomerativeClustering()
    assert "random_state" not in est.get_params()
    cc = ConsensusClustering(clusterer=est, clusterer_options={}, K_range=[5], random_state=7,
                             plot_cdf=False)
    cc._K = 5
    cc._set_clusterer_K()  # raised "Invalid parameter 'random_state'" before
    assert est.n_clusters == 5
    # an estimator that has the parameter still receives the seed
    km = KMeans()
    cc = ConsensusClustering(clusterer=km, K_range=[4], random_state=7, plot_cdf=False)
    cc._K = 4
    cc._set_clusterer_K()
    assert km.n_clusters == 4 and km.random_state == 7 and km.n_init == 3


def test_hierarchical_keyword_is_validated():
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(), clusterer_options={}, K_range=[2],
                             random_state=0, plot_cdf=False, hierarchical="gpu")
    with pytest.raises(ValueError, match="hierarchical must be"):
        cc.fit(np.zeros((10, 2), np.float32))


def test_validation_messages_on_host_arrays():
    X = np.zeros((10, 3), np.float32)
    api._hc_validate(X, 8, [1, 2, 8])
    Xn = X.copy()
    Xn[3, 1] = np.nan
    with pytest.raises(ValueError, match=r"Input X contains NaN\."):
        api._hc_validate(Xn, 8, [2])
    Xi = X.astype(np.float64)
    Xi[0, 0] = np.inf
    with pytest.raises(ValueError, match=r"Input X contains infinity or a value too large for dtype\('float64'\)"):
        api._hc_validate(Xi, 8, [2])
    with pytest.raises(ValueError, match=r"Found array with 1 sample\(s\) .* minimum of 2 is required by "
                                         "AgglomerativeClustering"):
        api._hc_validate(X, 1, [1])
    with pytest.raises(ValueError, match="Cannot extract more clusters than samples: 9 clusters were given "
                                         "for a tree with 8 leaves"):
        api._hc_validate(X, 8, [2, 9])


def test_validation_messages_are_sklearns():
    """The three refusals carry sklearn's own wording."""
    X = np.zeros((4, 2))
    X[1, 1] = np.nan
    with pytest.raises(ValueError) as e:
        AgglomerativeClustering().fit(X)
    assert str(e.value).startswith("Input X contains NaN.")
    with pytest.raises(ValueError) as e:
        AgglomerativeClustering().fit(np.zeros((1, 2)))
    with pytest.raises(ValueError) as mine:
        api._hc_validate(np.zeros((1, 2)), 1, [1])
    assert str(mine.value) == str(e.value)
    with pytest.raises(ValueError) as e:
        AgglomerativeClustering(n_clusters=5).fit(np.arange(8.0).reshape(4, 2))
    with pytest.raises(ValueError) as mine:
        api._hc_validate(np.zeros((4, 2)), 4, [5])
    assert str(mine.value) == str(e.value)


def test_batch_planner():
    n, m, nh, nK = 3000, 2400, 60, 11
    per = engine.hc_tree_bytes(m, nK)
    assert per >= 8 * m * m + 32 * (m - 1) + 8 * m + 4 * nK * m  # distances, merges, state, links
    full = 8 * n * n
    # many trees fit: every resample of the rank in one launch
    assert engine.hc_plan(n, m, nh, nK, full + 1000 * per) == (60, "batched")
    # the budget binds but still fills the GPU
    assert engine.hc_plan(n, m, nh, nK, full + 20 * per + per // 2) == (20, "batched")
    # fewer trees than the crossover: one at a time through cc_linkage_nnchain
    B, route = engine.hc_plan(n, m, nh, nK, full + (engine.HC_BATCH_CROSSOVER - 1) * per)
    assert (B, route) == (engine.HC_BATCH_CROSSOVER - 1, "sequential")
    assert engine.hc_plan(n, m, nh, nK, full + per) == (1, "sequential")
    # a rank with few resamples, all of which fit, keeps the one launch
    assert engine.hc_plan(n, m, 3, nK, full + 1000 * per) == (3, "batched")
    assert engine.hc_plan(n, m, 1, nK, full + per) == (1, "batched")
    # not even the distances and one tree: an error that names the budget
    with pytest.raises(ValueError, match=f"workspace_budget = {full + per - 1} bytes"):
        engine.hc_plan(n, m, nh, nK, full + per - 1)
    with pytest.raises(ValueError, match="workspace_budget"):
        engine.hc_plan(n, m, nh, nK, 1 << 20)


def _same_partition(a, b):
    pairs = set(zip(np.asarray(a).tolist(), np.asarray(b).tolist()))
    return len(pairs) == len({p for p, _ in pairs}) == len({q for _, q in pairs})


@pytest.mark.parametrize("kind", ["chain", "bypass", "random"])
@pytest.mark.parametrize("m", [2, 3, 64, 65, 300])
def test_reference_cut_is_the_cut_of_the_finished_tree(kind, m):
    """tests/hc_ref.py, which the device cut is compared with: reference_cut's partition of a
    synthetic tree (the caterpillars with increasing distances; random merges with tied ones) is
    sklearn's _hc_cut of the tree that linkage() finishes from the same merges, and its ids are
    exactly [0, K)."""
    from consensus_clustering_amd import post
    from tests import hc_ref

    rs = np.random.RandomState(m)
    Z = hc_ref.synthetic_merges(m, kind, rs)
    assert Z.shape == (m - 1, 4) and (Z[:, 0] < Z[:, 1]).all() and Z[-1, 3] == m
    assert len(set(Z[:, 0].tolist())) == m - 1  # every slot dies at most once
    if kind == "random":
        Z[:, 2] = rs.randint(0, 4, size=m - 1)
    children = post.linkage_finish(Z, m)[:, :2].astype(np.int64)
    for K in sorted({K for K in (1, 2, 3, min(m, 127)) if K <= m}):
        got = hc_ref.reference_cut(Z, m, K)
        assert sorted(set(got.tolist())) == list(range(K)), (m, K)
        assert _same_partition(got, post.hc_cut(K, children, m)), (m, K)
