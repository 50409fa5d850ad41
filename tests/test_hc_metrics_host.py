"""Host side of the hierarchical base clusterer's manhattan, cosine and correlation metrics (no
GPU): which (linkage, metric) pairs ``api._hc_spec`` routes to the device trees, that the
euclidean-only predicates answer as before, the degenerate-row routing, and the summation
recipes of cc_pdist restated in numpy and held to the installed scipy, exactly.  If a future scipy
sums differently, the recipe test here fails rather than the kernel's."""
import numpy as np
import pytest
from scipy.spatial.distance import pdist, squareform
from sklearn.cluster import AgglomerativeClustering, KMeans

from consensus_clustering_amd import ConsensusClustering, api


# ---------------------------------------------------------------- the predicate

SPELLINGS = [("euclidean", "euclidean"), ("l2", "euclidean"), ("manhattan", "cityblock"), ("l1", "cityblock"),
             ("cityblock", "cityblock"), ("cosine", "cosine"), ("correlation", "correlation")]


@pytest.mark.parametrize("link", ["average", "complete"])
@pytest.mark.parametrize("spelling,canonical", SPELLINGS)
def test_spec_maps_every_spelling(link, spelling, canonical):
    assert api._hc_spec(AgglomerativeClustering(linkage=link, metric=spelling)) == (link, canonical)


def test_spec_default_metric_and_ward():
    assert api._hc_spec(AgglomerativeClustering()) == ("ward", "euclidean")
    assert api._hc_spec(AgglomerativeClustering(linkage="ward", metric="euclidean")) == ("ward", "euclidean")
    for spelling, canonical in SPELLINGS:
        if canonical != "euclidean":  # sklearn refuses these itself: the host path raises its message
            assert api._hc_spec(AgglomerativeClustering(linkage="ward", metric=spelling)) is None


class _Sub(AgglomerativeClustering):
    pass


@pytest.mark.parametrize("est", [
    AgglomerativeClustering(linkage="single"),
    AgglomerativeClustering(linkage="single", metric="cosine"),
    _Sub(linkage="average", metric="cosine"),
    AgglomerativeClustering(linkage="average", metric="correlation", connectivity=np.eye(4)),
    AgglomerativeClustering(linkage="average", metric="cosine", distance_threshold=1.0, n_clusters=None),
    AgglomerativeClustering(linkage="average", metric="chebyshev"),
    AgglomerativeClustering(linkage="average", metric="precomputed"),
    AgglomerativeClustering(linkage="average", metric=lambda X: X),
    KMeans(),
], ids=["single", "single-cosine", "subclass", "connectivity", "distance_threshold", "chebyshev", "precomputed",
        "callable", "kmeans"])
def test_spec_is_none(est):
    assert api._hc_spec(est) is None


def test_spec_honours_clusterer_options():
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="single"),
                             clusterer_options={"linkage": "average", "metric": "correlation"}, K_range=[3],
                             random_state=0, plot_cdf=False)
    assert api._hc_spec(cc.clusterer) is None
    assert cc._kmeans_params() is None  # applies the options, as fit does before routing
    assert api._hc_spec(cc.clusterer) == ("average", "correlation")
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="complete", metric="cosine"),
                             clusterer_options={"linkage": "ward"}, K_range=[3], random_state=0, plot_cdf=False)
    assert api._hc_spec(cc.clusterer) == ("complete", "cosine")
    cc._kmeans_params()
    assert api._hc_spec(cc.clusterer) is None


def test_euclidean_predicates_keep_their_answers():
    """_hc_linkage and _is_device_hierarchical speak of the euclidean device trees alone."""
    for metric in ("manhattan", "cosine", "correlation"):
        est = AgglomerativeClustering(linkage="average", metric=metric)
        assert api._hc_linkage(est) is None
        assert not api._is_device_hierarchical(est)
        assert api._hc_spec(est) is not None
    for link in ("ward", "average", "complete"):
        assert api._hc_linkage(AgglomerativeClustering(linkage=link)) == link
        assert api._is_device_hierarchical(AgglomerativeClustering(linkage=link))
    assert api._hc_linkage(AgglomerativeClustering(linkage="single")) is None


# ---------------------------------------------------------------- degenerate rows

def _rows():
    X = np.random.RandomState(0).randn(12, 5)
    Z = X.copy()
    Z[7] = 0.0
    Z[7, 2] = -0.0
    C = X.copy()
    C[4] = 0.3
    return X, Z, C


def test_degenerate_rows_are_named():
    X, Z, C = _rows()
    for metric in ("euclidean", "cityblock", "cosine", "correlation"):
        assert api._hc_degenerate(X, metric) is None
    assert api._hc_degenerate(Z, "cosine") == "Cosine affinity cannot be used when X contains zero vectors"
    assert api._hc_degenerate(Z, "correlation") is not None  # a zero row is a constant row
    assert api._hc_degenerate(Z, "cityblock") is None and api._hc_degenerate(Z, "euclidean") is None
    assert api._hc_degenerate(C, "cosine") is None
    assert "row 4" in api._hc_degenerate(C, "correlation")
    assert api._hc_degenerate(X[:, :1], "correlation") is not None  # d = 1: every row is constant


def test_cosine_message_is_sklearns():
    _, Z, _ = _rows()
    with pytest.raises(ValueError) as e:
        AgglomerativeClustering(linkage="average", metric="cosine").fit(Z)
    assert str(e.value) == api._hc_degenerate(Z, "cosine")


@pytest.mark.parametrize("metric,which", [("cosine", 1), ("correlation", 2)])
def test_degenerate_row_routing(metric, which):
    """'auto' sends the fit to the host loop, 'device' raises, 'host' is the host loop anyway; a
    clean X is routed to the device by both; every decision is made without a GPU."""
    rows = _rows()
    X, bad = rows[0], rows[which]
    spec = ("average", metric)
    assert api._hc_route(spec, X, "auto") == spec
    assert api._hc_route(spec, X, "device") == spec
    assert api._hc_route(spec, X, "host") is None
    assert api._hc_route(spec, bad, "auto") is None
    assert api._hc_route(spec, bad, "host") is None
    want = "Cosine affinity cannot be used when X contains zero vectors" if metric == "cosine" else "constant row"
    with pytest.raises(ValueError, match=want):
        api._hc_route(spec, bad, "device")
    # the other metrics take such rows, and do not read X at all (it may live on the device)
    for other in (("average", "cityblock"), ("ward", "euclidean")):
        assert api._hc_route(other, bad, "device") == other
        assert api._hc_route(other, None, "auto") == other


def test_route_refuses_other_estimators_under_device():
    X = _rows()[0]
    assert api._hc_route(None, X, "auto") is None and api._hc_route(None, X, "host") is None
    with pytest.raises(ValueError, match="hierarchical='device'") as e:
        api._hc_route(None, X, "device")
    for word in ("manhattan", "cosine", "correlation", "euclidean"):
        assert word in str(e.value)


# ---------------------------------------------------------------- the recipes against scipy

def _dot2(U, V):
    """scipy's dot product of the float64 rows of U with those of V: products of even k and of odd
    k < (d & ~1) in two accumulators, each in increasing k; their sum; then an odd last column."""
    d = U.shape[1]
    a0 = np.zeros(U.shape[0])
    a1 = np.zeros(U.shape[0])
    for k in range(0, d & ~1, 2):
        a0 = a0 + U[:, k] * V[:, k]
        a1 = a1 + U[:, k + 1] * V[:, k + 1]
    t = a0 + a1
    if d & 1:
        t = t + U[:, d - 1] * V[:, d - 1]
    return t


def _cosine(X64):
    n = X64.shape[0]
    i, j = np.triu_indices(n, 1)
    norms = np.sqrt(_dot2(X64, X64))
    with np.errstate(invalid="ignore", divide="ignore"):
        c = _dot2(X64[i], X64[j]) / (norms[i] * norms[j])
    c = np.where(np.abs(c) > 1.0, np.copysign(1.0, c), c)
    return squareform(1.0 - c)


def restate(X, metric):
    """cc_pdist's arithmetic in numpy: float64 [n, n]."""
    X64 = np.asarray(X, dtype=np.float64)
    if metric == "cityblock":
        i, j = np.triu_indices(X64.shape[0], 1)
        acc = np.zeros(len(i))
        for k in range(X64.shape[1]):
            acc = acc + np.abs(X64[i, k] - X64[j, k])
        return squareform(acc)
    if metric == "correlation":
        return _cosine(X64 - X64.mean(axis=1, keepdims=True))
    assert metric == "cosine"
    return _cosine(X64)


@pytest.mark.parametrize("metric", ["cityblock", "cosine", "correlation"])
@pytest.mark.parametrize("n,d,dtype", [(65, 37, np.float32), (50, 2, np.float64), (50, 3, np.float64),
                                       (64, 16, np.float64)])
def test_recipes_equal_scipy_exactly(metric, n, d, dtype):
    X = np.random.RandomState(n + d).randn(n, d).astype(dtype)
    np.testing.assert_array_equal(restate(X, metric), squareform(pdist(X, metric)))
