"""Feature subsampling on the device: cc_pdist_batched against scipy's pdist of every resample's
own rows and columns bit for bit, the trees over those distances against scipy's linkage exactly,
the feature route of engine.hc_labels across shards and routes, and whole fits against a reference
built from the oracle's pieces and against the host loop.  tests/test_feature_subsampling_host.py
holds the recipes to the installed numpy and scipy on the CPU."""
import functools
import warnings

import numpy as np
import pytest
import torch
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import pdist, squareform
from sklearn.cluster import AgglomerativeClustering, KMeans

from consensus_clustering_amd import ConsensusClustering, _lib, engine, post
from oracle import cc_oracle as O
from tests.conftest import load_fixture

pytestmark = pytest.mark.gpu

METRICS = ["euclidean", "cityblock", "cosine", "correlation"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _scipy(Xs, metric):
    with np.errstate(invalid="ignore", divide="ignore"):
        return squareform(pdist(np.ascontiguousarray(Xs), metric))


def _draw(n, d, m, md, B, seed):
    """B resamples with different rows and different (sorted) columns each."""
    rs = np.random.RandomState(seed)
    idx = np.stack([rs.permutation(n)[:m] for _ in range(B)]).astype(np.int32)
    cols = np.stack([np.sort(rs.permutation(d)[:md]) for _ in range(B)]).astype(np.int32)
    return idx, cols


# ---------------------------------------------------------------- distances

SHAPES = ([(70, 40, 64, 16, np.float32), (70, 40, 65, 17, np.float64), (140, 9, 129, 1, np.float32),
           (40, 12, 2, 2, np.float64)]
          + [(90, 300, 63, md, np.float64) for md in (7, 8, 9)]
          + [(90, 300, 33, md, np.float32) for md in (128, 129, 136, 257)]
          + [(12, 8300, 9, 8195, np.float64)])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,d,m,md,dtype", SHAPES)
def test_pdist_batched_equals_scipy_bit_for_bit(n, d, m, md, dtype, metric):
    """One tile and one slab; a tile edge plus an odd last column after one slab; md = 1 (the
    correlation is NaN off the diagonal, and equal NaNs compare equal); the smallest tree; the
    block (8, 128) and recursion (129, 136, 257) edges of numpy's sum; a row longer than numpy's
    buffer of 8192, which its mean sums in pieces."""
    B = 3
    X = np.random.RandomState(n + d + md).randn(n, d).astype(dtype)
    idx, cols = _draw(n, d, m, md, B, seed=md)
    got = engine.pdist_batched(_dev(X), _dev(idx), _dev(cols), metric).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (B, m, m)
    for b in range(B):
        np.testing.assert_array_equal(got[b], _scipy(X[idx[b]][:, cols[b]], metric), err_msg=f"tree {b}")
        np.testing.assert_array_equal(got[b], got[b].T)
        np.testing.assert_array_equal(np.diag(got[b]), 0.0)


@pytest.mark.parametrize("metric", METRICS)
def test_every_column_equals_the_full_matrix(metric):
    n, d, m = 50, 12, 40
    X = np.random.RandomState(8).randn(n, d).astype(np.float32)
    idx, _ = _draw(n, d, m, d, 3, seed=1)
    cols = np.tile(np.arange(d, dtype=np.int32), (3, 1))
    got = engine.pdist_batched(_dev(X), _dev(idx), _dev(cols), metric).cpu().numpy()
    for b in range(3):
        np.testing.assert_array_equal(got[b], _scipy(X[idx[b]], metric))
    if metric != "correlation":  # engine.pdist centres correlation on the host
        full = engine.pdist(_dev(X), metric).cpu().numpy()
        for b in range(3):
            np.testing.assert_array_equal(got[b], full[idx[b]][:, idx[b]])


def test_out_of_range_indices_are_refused_before_the_launch():
    X = _dev(np.random.RandomState(0).randn(20, 6).astype(np.float32))
    idx, cols = _draw(20, 6, 10, 3, 2, seed=0)
    out = torch.full((2, 10, 10), -7.0, dtype=torch.float64, device="cuda")
    for bad_idx, bad_cols, what in [(20, None, "idx"), (-1, None, "idx"), (None, 6, "cols"), (None, -1, "cols")]:
        i, c = idx.copy(), cols.copy()
        if bad_idx is not None:
            i[1, 3] = bad_idx
        if bad_cols is not None:
            c[1, 2] = bad_cols
        with pytest.raises(ValueError, match=f"{what} entries must lie in"):
            engine.pdist_batched(X, _dev(i), _dev(c), "euclidean", out=out)
    assert bool((out == -7.0).all())  # nothing ran
    with pytest.raises(ValueError, match="metric must be one of"):
        engine.pdist_batched(X, _dev(idx), _dev(cols), "chebyshev")


def test_c_entry_point_refusals():
    X = _dev(np.zeros((4, 3), np.float32))
    idx = _dev(np.zeros((1, 4), np.int32))
    cols = _dev(np.zeros((1, 2), np.int32))
    D = torch.empty((1, 4, 4), dtype=torch.float64, device="cuda")
    lib = _lib.load()
    need = int(lib.cc_pdist_batched_workspace_bytes(1, 4, 2, 3))
    assert need == 8 * (4 * 2 + 4)
    assert int(lib.cc_pdist_batched_workspace_bytes(1, 4, 2, 7)) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(metric=3, m=4, md=2, nbytes=need, n=4, d=3, x=X.data_ptr()):
        _lib.call("cc_pdist_batched", x, 0, n, d, idx.data_ptr(), cols.data_ptr(), 1, m, md, metric,
                  D.data_ptr(), ws.data_ptr(), nbytes, engine.stream_ptr())

    call()
    with pytest.raises(_lib.CCMIError, match="unknown metric 7"):
        call(metric=7)
    with pytest.raises(_lib.CCMIError, match=f"workspace of {need - 1} bytes, {need} needed"):
        call(nbytes=need - 1)
    for kw in (dict(md=4), dict(m=5), dict(m=0), dict(x=None)):  # md > d, m > n, a size below 1, null
        with pytest.raises(_lib.CCMIError, match="bad arguments"):
            call(**kw)
    # cc_pdist keeps refusing the new code
    with pytest.raises(_lib.CCMIError, match="unknown metric 3"):
        _lib.call("cc_pdist", X.data_ptr(), 0, 4, 3, 3, D.data_ptr(), None, engine.stream_ptr())


# ---------------------------------------------------------------- trees

TREE_CASES = [(link, metric) for link in ("average", "complete") for metric in METRICS] + [("ward", "euclidean")]


@pytest.mark.parametrize("link,metric", TREE_CASES)
@pytest.mark.parametrize("m", [2, 3, 33])
def test_trees_equal_scipy(m, link, metric):
    n, d, md, B = m + 7, 9, 5, 3
    X = np.random.RandomState(m).randn(n, d).astype(np.float32)
    idx, cols = _draw(n, d, m, md, B, seed=m + 1)
    Db = engine.pdist_batched(_dev(X), _dev(idx), _dev(cols), metric)
    Z = engine.hc_nnchain_batched(Db, link).cpu().numpy()
    for b in range(B):
        Xs = np.ascontiguousarray(X[idx[b]][:, cols[b]])
        np.testing.assert_array_equal(post.linkage_finish(Z[b], m), linkage(Xs, link, metric), err_msg=f"tree {b}")


# ---------------------------------------------------------------- sharding and routes

def _route_labels(ranges, route):
    n, d, m, md, H, Ks = 60, 10, 48, 6, 7, [2, 3, 4]
    X = np.random.RandomState(2).randn(n, d).astype(np.float32)
    idx, _ = _draw(n, d, m, md, H, seed=4)
    cols = post.feature_indices(9, d, md, H)
    labels = engine.new_label_matrix(len(Ks), n, engine.pad_h(H), "cuda")
    for h0, h1 in ranges:
        stats = engine.hc_labels(None, _dev(idx), h0, h1, Ks, "average", labels, route=route, X=_dev(X),
                                 cols_d=_dev(cols), metric="correlation")
        assert stats["route"] == route and stats["feature_subsampling"] == md
    got = labels.cpu().numpy()
    for h in range(H):  # sklearn's partition of every (h, K) (the device names the clusters its own way)
        Xs = np.ascontiguousarray(X[idx[h]][:, cols[h]])
        for k, K in enumerate(Ks):
            want = AgglomerativeClustering(n_clusters=K, linkage="average", metric="correlation").fit_predict(Xs)
            mine = got[k, idx[h], h]
            assert sorted(set(mine.tolist())) == list(range(K)), (h, K)
            np.testing.assert_array_equal(mine[:, None] == mine[None, :], want[:, None] == want[None, :],
                                          err_msg=f"h={h} K={K}")
        unsampled = np.setdiff1d(np.arange(n), idx[h])
        assert (got[:, unsampled, h] == 0xFF).all()
    return got


def test_feature_route_in_one_call_in_two_and_sequentially():
    """cols is indexed by the global h like idx: [0, 7) at once and as [0, 3) then [3, 7) fill the
    same labels, one tree at a time (cc_linkage_nnchain) as well, and they are sklearn's
    partitions."""
    whole = _route_labels([(0, 7)], "batched")
    np.testing.assert_array_equal(_route_labels([(0, 3), (3, 7)], "batched"), whole)
    np.testing.assert_array_equal(_route_labels([(0, 7)], "sequential"), whole)


def test_feature_route_budget():
    n, d, m, md, H, Ks = 60, 10, 48, 6, 7, [2, 3]
    X = _dev(np.random.RandomState(2).randn(n, d).astype(np.float32))
    idx, _ = _draw(n, d, m, md, H, seed=4)
    cols = _dev(post.feature_indices(9, d, md, H))
    labels = engine.new_label_matrix(len(Ks), n, engine.pad_h(H), "cuda")
    per = engine.hc_tree_bytes(m, len(Ks)) + engine.hc_feature_bytes(m, md)
    args = (None, _dev(idx), 0, H, Ks, "average", labels)
    kw = dict(X=X, cols_d=cols, metric="euclidean")
    assert engine.hc_labels(*args, budget=3 * per, **kw) == dict(route="batched", batch=3, launches=3,
                                                                 feature_subsampling=md)
    with pytest.raises(ValueError, match="workspace_budget"):
        engine.hc_labels(*args, budget=per - 1, **kw)


def test_feature_route_refuses_distances_that_overflow():
    """A finite row whose squared differences overflow float64: the first resample that holds it
    is named (scipy's linkage refuses such distances in the host loop too)."""
    n, d, m, md, H, Ks = 30, 8, 12, 4, 6, [2]
    X = np.random.RandomState(5).randn(n, d)
    X[7] = 1e200
    idx, _ = _draw(n, d, m, md, H, seed=3)
    first = min(h for h in range(H) if 7 in idx[h])
    assert 0 < first  # an earlier resample is clean
    labels = engine.new_label_matrix(1, n, engine.pad_h(H), "cuda")
    with pytest.raises(engine.DegenerateResample, match=f"not all finite \\(resample {first},") as e:
        engine.hc_labels(None, _dev(idx), 0, H, Ks, "average", labels, X=_dev(X),
                         cols_d=_dev(post.feature_indices(1, d, md, H)), metric="euclidean")
    assert e.value.code == 4 * first + engine.DEGENERATE_NOT_FINITE
    with pytest.raises(ValueError):
        linkage(np.ascontiguousarray(X[idx[first]][:, :md]), "average", "euclidean")


# ---------------------------------------------------------------- whole fits

E2E = dict(K_range=list(range(2, 8)), n_iterations=24, subsampling=0.8, random_state=3)
FRACTION, MD = 0.75, 6
CASES = [("average", "correlation"), ("complete", "cosine"), ("average", "manhattan"), ("ward", "euclidean")]


@functools.lru_cache(maxsize=None)
def _e2e_X(dtype):
    return np.ascontiguousarray(load_fixture("blobs_n400_d8_k4")["X"], dtype=dtype)


def _formula_cols(seed, d, md, H):
    return np.stack([np.sort(np.random.RandomState((seed + h, 1)).choice(d, md, replace=False))
                     for h in range(H)])


@functools.lru_cache(maxsize=None)
def _e2e_fit(link, metric, dtype, hierarchical="auto"):
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage=link, metric=metric), clusterer_options={},
                             plot_cdf=False, hierarchical=hierarchical, feature_subsampling=FRACTION, **E2E)
    return cc.fit(_e2e_X(dtype))


@functools.lru_cache(maxsize=None)
def _e2e_reference(link, metric, dtype):
    """The fit from the oracle's pieces, with sklearn on every resample's contiguous subset."""
    X = _e2e_X(dtype)
    n, d = X.shape
    H, Ks, seed = E2E["n_iterations"], E2E["K_range"], E2E["random_state"]
    idx = O.subsampling_indices(n, H, E2E["subsampling"], seed)
    cols = _formula_cols(seed, d, MD, H)
    I = O.cosample_matrix(idx, n)
    out = {}
    for K in Ks:
        labs = np.stack([AgglomerativeClustering(n_clusters=K, linkage=link, metric=metric).fit_predict(
            np.ascontiguousarray(X[idx[h]][:, cols[h]])) for h in range(H)])
        out[K] = O.analyse(O.coassoc_matrix(idx, labs, K, n), I, dtype=O.reference_dtype(H))
    return out


def _assert_same_results(a, b):
    for K in E2E["K_range"]:
        for key in ("mij", "iij", "cij", "hist", "cdf", "bin_edges"):
            np.testing.assert_array_equal(a.cdf_at_K_data[K][key], b.cdf_at_K_data[K][key], err_msg=f"{key} K={K}")
        assert a.cdf_at_K_data[K]["pac_area"] == b.cdf_at_K_data[K]["pac_area"]
        np.testing.assert_array_equal(a.pair_counts_[K], b.pair_counts_[K])
    assert a.best_k_ == b.best_k_


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("link,metric", CASES)
def test_fit_equals_reference_and_host(link, metric, dtype):
    X = _e2e_X(dtype)
    n, d = X.shape
    cc = _e2e_fit(link, metric, dtype)
    assert cc.backend_ == "gpu-hc" and cc.hc_stats_["feature_subsampling"] == MD
    assert cc.feature_indices_.dtype == np.int32
    np.testing.assert_array_equal(cc.feature_indices_, _formula_cols(E2E["random_state"], d, MD, E2E["n_iterations"]))
    assert len({tuple(c) for c in cc.feature_indices_}) > 1
    ref = _e2e_reference(link, metric, dtype)
    for K in E2E["K_range"]:
        g, r = cc.cdf_at_K_data[K], ref[K]
        np.testing.assert_array_equal(g["mij"], r["mij"], err_msg=f"K={K}")
        np.testing.assert_array_equal(g["iij"], r["iij"])
        np.testing.assert_array_equal(post.pair_counts_to_hist_counts(cc.pair_counts_[K], n),
                                      O.bin_counts(r["cij"]), err_msg=f"K={K}")
        np.testing.assert_array_equal(g["hist"], r["hist"], err_msg=f"K={K}")
        np.testing.assert_array_equal(g["cdf"], r["cdf"], err_msg=f"K={K}")
        assert g["pac_area"] == r["pac_area"], K
        assert np.max(np.abs(g["cij"] - r["cij"])) <= 1e-6
    host = _e2e_fit(link, metric, dtype, "host")
    assert host.backend_ == "host-clusterer" and host.hc_stats_ is None
    np.testing.assert_array_equal(host.feature_indices_, cc.feature_indices_)
    _assert_same_results(cc, host)


@pytest.mark.parametrize("link,metric", [("average", "correlation"), ("ward", "euclidean")])
def test_fit_on_a_device_tensor(link, metric):
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage=link, metric=metric), clusterer_options={},
                             plot_cdf=False, feature_subsampling=FRACTION, **E2E)
    cc.fit(torch.from_numpy(_e2e_X(np.float32)).cuda())
    assert cc.backend_ == "gpu-hc"
    _assert_same_results(cc, _e2e_fit(link, metric, np.float32))


def test_default_fraction_changes_nothing():
    X = _e2e_X(np.float32)
    kw = dict(clusterer_options={}, plot_cdf=False, **E2E)
    a = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="average", metric="correlation"), **kw).fit(X)
    b = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="average", metric="correlation"),
                            feature_subsampling=1.0, **kw).fit(X)
    _assert_same_results(a, b)
    assert a.feature_indices_ is None and b.feature_indices_ is None
    assert a.backend_ == b.backend_ == "gpu-hc"
    assert a.hc_stats_ == b.hc_stats_ and b.hc_stats_["route"] == "batched"
    assert "feature_subsampling" not in b.hc_stats_


@pytest.mark.parametrize("value", [0, 1.5, True, 0.1])
def test_fraction_refusals(value):
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(), clusterer_options={}, plot_cdf=False,
                             feature_subsampling=value, **E2E)
    with pytest.raises(ValueError, match="feature_subsampling.*d = 8"):
        cc.fit(_e2e_X(np.float32))


def _fit_raises(X, link, metric, hierarchical, match):
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage=link, metric=metric), clusterer_options={},
                             plot_cdf=False, hierarchical=hierarchical, feature_subsampling=FRACTION, **E2E)
    with pytest.raises(ValueError, match=match) as e:
        cc.fit(X)
    return cc, e.value


def test_a_zero_row_under_cosine_is_refused_per_resample():
    X = _e2e_X(np.float32).copy()
    X[0] = 0.0
    idx = O.subsampling_indices(len(X), E2E["n_iterations"], E2E["subsampling"], E2E["random_state"])
    first = min(h for h in range(len(idx)) if 0 in idx[h])
    sentence = "Cosine affinity cannot be used when X contains zero vectors"
    for hierarchical in ("device", "auto"):
        cc, err = _fit_raises(X, "average", "cosine", hierarchical, sentence)
        assert cc.backend_ == "gpu-hc"
        assert f"resample {first}," in str(err) and "'cosine'" in str(err)
    cc, _ = _fit_raises(X, "average", "cosine", "host", sentence)
    assert cc.backend_ == "host-clusterer"


def test_a_constant_row_under_correlation_is_refused_per_resample():
    """1.5 sums and divides exactly, so the centred row is exactly zero."""
    X = _e2e_X(np.float32).copy()
    X[3] = 1.5
    idx = O.subsampling_indices(len(X), E2E["n_iterations"], E2E["subsampling"], E2E["random_state"])
    first = min(h for h in range(len(idx)) if 3 in idx[h])
    for hierarchical in ("device", "auto"):
        cc, err = _fit_raises(X, "average", "correlation", hierarchical, f"resample {first},")
        assert cc.backend_ == "gpu-hc" and "'correlation'" in str(err)
    _fit_raises(X, "average", "correlation", "host", None)


def test_kmeans_falls_back_to_the_host_loop():
    X = np.ascontiguousarray(load_fixture("blobs_n150_d5_k3_h300")["X"])
    n, d = X.shape
    Ks, H, seed, md = [2, 3], 6, 0, 2
    cc = ConsensusClustering(K_range=Ks, n_iterations=H, subsampling=0.8, random_state=seed, plot_cdf=False,
                             feature_subsampling=0.5)
    with pytest.warns(UserWarning, match="k-means engines do not subsample features"):
        cc.fit(X)
    assert cc.backend_ == "host-clusterer" and cc.precision_ is None and cc.feature_indices_.shape == (H, md)
    idx = O.subsampling_indices(n, H, 0.8, seed)
    cols = _formula_cols(seed, d, md, H)
    I = O.cosample_matrix(idx, n)
    for K in Ks:
        labs = np.stack([KMeans(n_clusters=K, random_state=0, n_init=3).fit_predict(
            np.ascontiguousarray(X[idx[h]][:, cols[h]])) for h in range(H)])
        r = O.analyse(O.coassoc_matrix(idx, labs, K, n), I, dtype=O.reference_dtype(H))
        np.testing.assert_array_equal(cc.cdf_at_K_data[K]["mij"], r["mij"])
        np.testing.assert_array_equal(cc.cdf_at_K_data[K]["iij"], r["iij"])
    with warnings.catch_warnings():  # the default fraction keeps the device k-means, silently
        warnings.filterwarnings("error", message=".*k-means engines.*")
        cc = ConsensusClustering(K_range=Ks, n_iterations=H, subsampling=0.8, random_state=seed,
                                 plot_cdf=False).fit(X)
    assert cc.backend_ == "gpu-kmeans"
