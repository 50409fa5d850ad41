"""Host side of feature subsampling (no GPU): the column draws, the recipes the device row pass
restates (numpy's mean of a compact row; scipy's correlation as cosine on the rows so centred)
against the installed numpy and scipy, the host loop on column subsets, the planner without the
n x n matrix, and the ranks' agreement on a failing resample (gloo, world 2)."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp
from scipy.spatial.distance import pdist
from sklearn.cluster import AgglomerativeClustering

from consensus_clustering_amd import ConsensusClustering, api, engine, post
from tests.conftest import ROOT


# ---------------------------------------------------------------- column draws

def test_feature_indices_follow_the_formula():
    seed, d, md, H = 11, 40, 13, 9
    cols = post.feature_indices(seed, d, md, H)
    assert cols.dtype == np.int32 and cols.shape == (H, md)
    for h in range(H):
        want = np.sort(np.random.RandomState((seed + h, 1)).choice(d, md, replace=False))
        np.testing.assert_array_equal(cols[h], want)
        assert (np.diff(cols[h]) > 0).all()  # sorted and distinct
        assert cols[h].min() >= 0 and cols[h].max() < d
    np.testing.assert_array_equal(cols, post.feature_indices(seed, d, md, H))
    assert len({tuple(c) for c in cols}) > 1


def test_column_stream_is_apart_from_the_item_stream():
    """The same seed, the same population and the same count: the item draw RandomState(seed + h)
    and the column draw RandomState((seed + h, 1)) choose different sets."""
    seed, d, md, H = 3, 50, 20, 6
    cols = post.feature_indices(seed, d, md, H)
    for h in range(H):
        items = np.sort(np.random.RandomState(seed + h).choice(d, md, replace=False))
        assert not np.array_equal(cols[h], items)


def test_largest_seed_is_accepted():
    post.feature_indices(2**32 - 3, 5, 2, 3)  # both seed elements lie in [0, 2**32)


# ---------------------------------------------------------------- the row pass's recipes

BLOCK, BUFSIZE = 128, 8192  # numpy's PW_BLOCKSIZE and default buffer size


def _pw(a):
    n = len(a)
    if n < 8:
        s = 0.0
        for x in a:
            s = s + x
        return s
    if n <= BLOCK:
        r = [a[j] for j in range(8)]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = r[j] + a[i + j]
            i += 8
        s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            s = s + a[i]
            i += 1
        return s
    n2 = n // 2
    n2 -= n2 % 8
    return _pw(a[:n2]) + _pw(a[n2:])


def recipe_mean(row):
    """numpy's mean of a float64 row as csrc/pdist.hip restates it: from 0.0, the pairwise
    sum of each piece of numpy's buffer size added in turn; divided by the length."""
    row = [np.float64(x) for x in row]
    s = np.float64(0.0)
    for o in range(0, len(row), BUFSIZE):
        s = s + _pw(row[o:o + BUFSIZE])
    return s / np.float64(len(row))


MDS = list(range(1, 10)) + [15, 16, 17] + list(range(127, 138)) + [255, 256, 257, 300]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("md", MDS)
def test_mean_recipe_equals_numpy(md, dtype):
    """A numpy that sums differently fails here first."""
    X = (np.random.RandomState(md).randn(3, md) * 100).astype(dtype).astype(np.float64)
    got = np.array([recipe_mean(X[r]) for r in range(3)])
    np.testing.assert_array_equal(got, X.mean(axis=1))


@pytest.mark.parametrize("md", [8192, 8193, 16385, 20001])
def test_mean_recipe_past_numpys_buffer(md):
    """Rows longer than numpy's buffer reach the add loop in pieces of 8192."""
    X = np.random.RandomState(md).randn(2, md)
    np.testing.assert_array_equal(np.array([recipe_mean(X[0]), recipe_mean(X[1])]), X.mean(axis=1))


def test_mean_recipe_keeps_the_sign_of_zero():
    X = np.full((1, 9), -0.0)
    got, want = recipe_mean(X[0]), X.mean(axis=1)[0]
    assert got == want and np.signbit(got) == np.signbit(want)


def _dot2(u, v):
    """scipy's dot product: two accumulators by parity of k, the odd last column after a0 + a1."""
    a0 = a1 = np.float64(0.0)
    de = len(u) & ~1
    for k in range(0, de, 2):
        a0 = a0 + u[k] * v[k]
        a1 = a1 + u[k + 1] * v[k + 1]
    t = a0 + a1
    if len(u) & 1:
        t = t + u[-1] * v[-1]
    return t


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("md", [2, 7, 8, 9, 17, 129, 136])
def test_correlation_recipe_equals_scipy(md, dtype):
    rs = np.random.RandomState(md)
    X = rs.randn(30, 300).astype(dtype)
    idx = rs.permutation(30)[:12]
    cols = np.sort(rs.choice(300, md, replace=False))
    Xs = np.ascontiguousarray(X[idx][:, cols])
    C = Xs.astype(np.float64)
    C = np.stack([C[r] - recipe_mean(C[r]) for r in range(len(C))])
    norms = np.array([np.sqrt(_dot2(u, u)) for u in C])
    got = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(len(C)):
            for j in range(i + 1, len(C)):
                c = _dot2(C[i], C[j]) / (norms[i] * norms[j])
                if abs(c) > 1.0:
                    c = np.copysign(1.0, c)
                got.append(1.0 - c)
        want = pdist(Xs, "correlation")
    np.testing.assert_array_equal(np.array(got), want)


# ---------------------------------------------------------------- the host loop

@pytest.mark.parametrize("n_jobs", [1, 2])
def test_host_loop_fits_the_contiguous_subset(n_jobs):
    rs = np.random.RandomState(0)
    X = rs.randn(40, 10).astype(np.float32)
    idx = np.stack([rs.permutation(40)[:30] for _ in range(5)]).astype(np.int32)
    cols = post.feature_indices(4, 10, 6, 5)
    est = AgglomerativeClustering(n_clusters=3, linkage="average", metric="correlation")
    got = api.host_fit_predict(est, X, idx, n_jobs, "multithreading", cols=cols)
    assert got.dtype == np.int32 and got.shape == (5, 30)
    for h in range(5):
        Xs = np.ascontiguousarray(X[idx[h]][:, cols[h]])
        assert Xs.flags.c_contiguous and not X[idx[h]][:, cols[h]].flags.c_contiguous
        np.testing.assert_array_equal(got[h], AgglomerativeClustering(
            n_clusters=3, linkage="average", metric="correlation").fit_predict(Xs))
    # without cols nothing changes
    np.testing.assert_array_equal(api.host_fit_predict(est, X, idx, n_jobs),
                                  np.stack([est.fit_predict(X[i]) for i in idx]))


# ---------------------------------------------------------------- refusals from host values

@pytest.mark.parametrize("value", [0, 1.5, True, 0.1, -0.5, "0.5", None])
def test_fraction_is_validated(value):
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(), clusterer_options={}, K_range=[2],
                             random_state=0, plot_cdf=False, feature_subsampling=value)
    with pytest.raises(ValueError, match=r"feature_subsampling .*d = 8.*got"):
        cc._feature_count(8)
    with pytest.raises(ValueError, match="feature_subsampling"):  # before the GPU is asked for
        cc.fit(np.zeros((10, 8), np.float32))


def test_fraction_truncates_like_the_item_count():
    cc = ConsensusClustering(K_range=[2], random_state=0, plot_cdf=False, feature_subsampling=0.75)
    assert cc._feature_count(8) == 6 and cc._feature_count(9) == 6 and cc._feature_count(2) == 1
    cc.feature_subsampling = 1
    assert cc._feature_count(8) == 8


# ---------------------------------------------------------------- planner

def test_planner_without_the_full_matrix():
    n, m, nh, nK, md = 3000, 2400, 60, 11, 25
    extra = engine.hc_feature_bytes(m, md)
    assert extra == 8 * m * md + 8 * m + 4 * md
    per = engine.hc_tree_bytes(m, nK) + extra
    # no 8 n^2 term: a budget below the n x n matrix alone holds a tree
    assert per < 8 * n * n
    assert engine.hc_plan(n, m, nh, nK, 1000 * per, md=md) == (60, "batched")
    assert engine.hc_plan(n, m, nh, nK, 20 * per + per // 2, md=md) == (20, "batched")
    assert engine.hc_plan(n, m, nh, nK, (engine.HC_BATCH_CROSSOVER - 1) * per, md=md) == (
        engine.HC_BATCH_CROSSOVER - 1, "sequential")
    assert engine.hc_plan(n, m, nh, nK, 2 * per - 1, md=md) == (1, "sequential")
    assert engine.hc_plan(n, m, nh, nK, engine.HC_BATCH_CROSSOVER * per, md=md) == (
        engine.HC_BATCH_CROSSOVER, "batched")
    assert engine.hc_plan(n, m, 1, nK, per, md=md) == (1, "batched")
    with pytest.raises(ValueError, match=f"workspace_budget = {per - 1} bytes"):
        engine.hc_plan(n, m, nh, nK, per - 1, md=md)


def test_planner_with_the_full_matrix_is_unchanged():
    n, m, nh, nK = 3000, 2400, 60, 11
    per = 8 * m * m + (32 + 8 + 8 + 4) * (m - 1) + 8 * m + 4 * nK * m + 512
    assert engine.hc_tree_bytes(m, nK) == per
    full = 8 * n * n
    assert engine.hc_plan(n, m, nh, nK, full + 20 * per + per // 2) == (20, "batched")
    assert engine.hc_plan(n, m, nh, nK, full + per) == (1, "sequential")
    with pytest.raises(ValueError, match=f"workspace_budget = {full + per - 1} bytes"):
        engine.hc_plan(n, m, nh, nK, full + per - 1)


# ---------------------------------------------------------------- rank agreement

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out):
    import sys

    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from consensus_clustering_amd import dist as cdist

        one = cdist.first_failure(5 if rank == 1 else None)
        none = cdist.first_failure(None)
        both = cdist.first_failure(7 if rank == 0 else 6)
        np.save(f"{out}.{rank}.npy", np.array([-1 if v is None else v for v in (one, none, both)]))
    finally:
        dist.destroy_process_group()


def test_ranks_agree_on_the_first_failing_resample(tmp_path):
    out = str(tmp_path / "agree")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    for rank in range(2):
        np.testing.assert_array_equal(np.load(f"{out}.{rank}.npy"), [5, -1, 6])


def test_agreement_without_a_process_group_does_nothing():
    from consensus_clustering_amd import dist as cdist

    assert cdist.first_failure(None) is None and cdist.first_failure(9) == 9


def test_degenerate_resample_messages():
    e = engine.DegenerateResample(4 * 5 + engine.DEGENERATE_ZERO_NORM, "cosine")
    assert isinstance(e, ValueError) and e.code == 20
    assert "Cosine affinity cannot be used when X contains zero vectors" in str(e) and "resample 5" in str(e)
    e = engine.DegenerateResample(4 * 2 + engine.DEGENERATE_ZERO_NORM, "correlation")
    assert "resample 2" in str(e) and "correlation" in str(e)
    e = engine.DegenerateResample(4 * 3 + engine.DEGENERATE_NOT_FINITE, "euclidean")
    assert "resample 3" in str(e) and "euclidean" in str(e) and "not all finite" in str(e)
