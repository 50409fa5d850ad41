"""ConsensusClustering.predict on the routes the other tests never take: 'complete' linkage,
distance='1-C', 'single' over '1-C', and every refusal, against sklearn's AgglomerativeClustering
on the fit's own consensus matrix (exact label equality: cc_manhattan's distances and the device
nn_chain / Prim must take scipy's and sklearn's decisions, ties included)."""
import copy

import numpy as np
import pytest
from sklearn.cluster import AgglomerativeClustering

from tests.conftest import load_fixture

pytestmark = pytest.mark.gpu

KS = [2, 3, 4]


@pytest.fixture(scope="module")
def fitted():
    """One fit of blobs_n400_d8_k4; predict() reads agg_clustering_linkage when it is called."""
    from consensus_clustering_amd import ConsensusClustering

    f = load_fixture("blobs_n400_d8_k4")
    meta = f["meta"]
    cc = ConsensusClustering(K_range=[int(k) for k in f["K_range"]], n_iterations=meta["H"],
                             subsampling=meta["subsampling"], random_state=meta["random_state"],
                             plot_cdf=False)
    cc.fit(f["X"])
    assert cc.cdf_at_K_data[2]["cij"] is not None
    return cc


def _with_linkage(cc, link):
    cc = copy.copy(cc)
    cc.agg_clustering_linkage = link
    return cc


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("link", ["average", "complete"])
def test_predict_manhattan_matches_sklearn(fitted, link, K):
    """Default distance: cc_manhattan (predict.hip:35) on the rows of C, then cc_linkage_nnchain
    with CC_LINK_AVERAGE / CC_LINK_COMPLETE (predict.hip:441) -- 'complete' is never run by the
    other predict tests -- against the reference's own call (CC.py:306-312)."""
    C = fitted.cdf_at_K_data[K]["cij"]
    want = AgglomerativeClustering(n_clusters=K, linkage=link, metric="manhattan").fit_predict(C)
    np.testing.assert_array_equal(_with_linkage(fitted, link).predict(K), want)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("link", ["average", "complete", "single"])
def test_predict_one_minus_c_matches_sklearn(fitted, link, K):
    """distance='1-C' (api.py: D = 1 - f64(C), no cc_manhattan): the linkage over the consensus
    distance itself, whose values are heavily tied (C is 0 or 1 for most pairs of well separated
    blobs), against sklearn on the same precomputed matrix; 'single' runs Prim on the device
    (cc_linkage_mst, predict.hip:467) where sklearn runs scipy's linkage for a precomputed
    metric, and both must cut to the same labels."""
    C = fitted.cdf_at_K_data[K]["cij"]
    D = 1.0 - C.astype(np.float64)
    want = AgglomerativeClustering(n_clusters=K, linkage=link, metric="precomputed").fit_predict(D)
    np.testing.assert_array_equal(_with_linkage(fitted, link).predict(K, distance="1-C"), want)


@pytest.mark.parametrize("link,K,kwargs,exc,message", [
    ("average", True, {}, ValueError, "must be an int in the range [1, inf) or None. Got True instead."),
    ("average", 0, {}, ValueError, "must be an int in the range [1, inf) or None. Got 0 instead."),
    ("average", -3, {}, ValueError, "must be an int in the range [1, inf) or None. Got -3 instead."),
    ("average", 2.0, {}, ValueError, "must be an int in the range [1, inf) or None. Got 2.0 instead."),
    ("average", 401, {}, ValueError, "Cannot extract more clusters than samples: 401 clusters were given "
                                     "for a tree with 400 leaves."),
    ("average", 7, {}, KeyError, "K = 7 is not in K_range of the fit"),
    ("ward", 3, {}, ValueError, "ward linkage needs the euclidean metric"),
    ("average", 3, {"distance": "euclidean"}, ValueError, "distance must be 'manhattan' or '1-C'"),
    ("centroid", 3, {}, ValueError, "unknown linkage 'centroid'"),
], ids=["bool", "zero", "negative", "float", "above-n", "not-fitted", "ward", "distance", "linkage"])
def test_predict_refusals_before_device_work(fitted, monkeypatch, link, K, kwargs, exc, message):
    """Every ValueError / KeyError branch of predict (api.py:671-697) with the message in the
    code, raised before C is built or any kernel is called."""
    from consensus_clustering_amd import engine

    cc = _with_linkage(fitted, link)

    def device_work(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(cc, "_consensus_device", device_work)
    for name in ("manhattan", "linkage", "linkage_single", "consensus", "cosample", "coassoc"):
        monkeypatch.setattr(engine, name, device_work)
    with pytest.raises(exc) as e:
        cc.predict(K, **kwargs)
    assert message in str(e.value)
