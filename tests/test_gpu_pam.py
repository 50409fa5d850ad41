"""The PAM base clusterer on the device (csrc/pam.hip): cc_pam_build, cc_pam_swap_step and
cc_pam_labels against the host PAM on gathered resamples, and whole fits against the oracle with
the host PAM as its clusterer and against the host loop.  tests/test_pam_host.py holds the host
PAM to the brute-force reference of tests/pam_ref.py on the CPU.

The device adds in another order than the host, so the two agree wherever a decision's margin is
well above m * 2^-52.  Every continuous case below therefore first asserts that
pam_ref, whose sums are exactly rounded, reports a relative margin >= 1e-9 over its decisions: a
precondition of the comparison, with the seeds chosen on the CPU so that it holds.  The margin
leaves out the decisions pam_ref counts as ties: candidates whose sums are the same terms in
another order (the two equal row sums at m = 2; the two closest medoids at K = m - 1, either of
which may leave for the same total deviation), which every implementation that rounds each term
alike must also see as ties, and which the tie rule settles.  The lattice case has exact sums
throughout and is compared with no precondition."""
import functools

import numpy as np
import pytest
import torch
from scipy.spatial.distance import pdist, squareform

from consensus_clustering_amd import PAM, ConsensusClustering, engine, post
from consensus_clustering_amd import pam as P
from oracle import cc_oracle as O
from tests.conftest import load_fixture
from tests.pam_ref import pam_ref

pytestmark = pytest.mark.gpu

H_BEGIN = 2  # the column of the first tree: the kernels add it to every output index


class SubPAM(PAM):
    """A subclass: never routed to the device, so a fit with it is the host loop."""


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# (name, m, Ks, metric, seed): one past a wave (65), one past a 256-thread tile (257), K across a
# wave boundary and at KMAX (130), K = m (33), the smallest problems (2, 3)
CASES = [("m2", 2, [1, 2], "euclidean", 0), ("m3", 3, [1, 2, 3], "cityblock", 0),
         ("m33", 33, [1, 4, 32, 33], "correlation", 0), ("m65", 65, [1, 2, 7, 64], "cosine", 0),
         ("m130", 130, [1, 2, 64, 65, 127], "euclidean", 0), ("m257", 257, [1, 2, 5], "cityblock", 0)]
B = 3


@functools.lru_cache(maxsize=None)
def _case(name):
    """X, idx [B, m] and per tree the host distances, for a continuous case or the lattice."""
    rs = np.random.RandomState(1)
    if name == "lattice":
        half = rs.randint(0, 3, size=(32, 2)).astype(np.float64)
        X, m, Ks, metric = np.concatenate([half, half]), 64, [1, 2, 3, 8, 31, 63, 64], "cityblock"
        idx = np.stack([rs.permutation(64) for _ in range(B)]).astype(np.int32)
    else:
        _, m, Ks, metric, seed = next(c for c in CASES if c[0] == name)
        rs = np.random.RandomState(1000 * seed + m)
        n = m + 7
        X = rs.randn(n, 6)
        idx = np.stack([rs.permutation(n)[:m] for _ in range(B)]).astype(np.int32)
    D = [squareform(pdist(X[idx[b]], metric)) for b in range(B)]
    return X, idx, Ks, metric, D


@functools.lru_cache(maxsize=None)
def _host(name, max_iter=300):
    """[b][k] -> (medoids, labels, inertia, n_iter) of the host PAM: computed once, never changed."""
    _, _, Ks, _, D = _case(name)
    return [[P.pam(D[b], K, max_iter) for K in Ks] for b in range(B)]


def margins(name):
    """The smallest pam_ref margin over the trees and K of a case, and whether the host PAM took
    pam_ref's decisions throughout."""
    _, _, Ks, _, D = _case(name)
    worst, same = np.inf, True
    for b in range(B):
        for k, K in enumerate(Ks):
            ref = pam_ref(D[b], K)
            got = _host(name)[b][k]
            worst = min(worst, ref.margin)
            same &= np.array_equal(ref.medoids, got[0]) and np.array_equal(ref.labels, got[1]) and ref.n_iter == got[3]
    return worst, same


def _device(name, max_iter=300):
    X, idx, Ks, metric, _ = _case(name)
    n, m, nK, Kmax = X.shape[0], idx.shape[1], len(Ks), max(Ks)
    Xd = _dev(X)
    Dfull = engine.euclidean(Xd) if metric == "euclidean" else engine.pdist(Xd, metric)
    idx_d = _dev(idx)
    Db = engine.hc_gather(Dfull, idx_d)
    Hpad = engine.pad_h(H_BEGIN + B)
    labels = engine.new_label_matrix(nK, n, Hpad, "cuda")
    inertia = torch.full((nK, H_BEGIN + B), -1.0, dtype=torch.float64, device="cuda")
    n_iter = torch.full((nK, H_BEGIN + B), -1, dtype=torch.int32, device="cuda")
    medoids = torch.full((B, nK, Kmax), -7, dtype=torch.int32, device="cuda")
    its = engine.pam_batch(Db, idx_d, _dev(np.array(Ks, dtype=np.int32)), Kmax, H_BEGIN, labels, max_iter, inertia,
                           n_iter, medoids)
    torch.cuda.synchronize()
    return medoids.cpu().numpy(), labels.cpu().numpy(), inertia.cpu().numpy(), n_iter.cpu().numpy(), its


def _assert_device_equals_host(name, max_iter=300):
    X, idx, Ks, _, _ = _case(name)
    m = idx.shape[1]
    host = _host(name, max_iter)
    medoids, labels, inertia, n_iter, its = _device(name, max_iter)
    assert its <= max_iter
    assert (labels[:, :, :H_BEGIN] == 0xFF).all() and (labels[:, :, H_BEGIN + B:] == 0xFF).all()
    assert (inertia[:, :H_BEGIN] == -1.0).all() and (n_iter[:, :H_BEGIN] == -1).all()
    for b in range(B):
        out = np.setdiff1d(np.arange(X.shape[0]), idx[b])
        for k, K in enumerate(Ks):
            h_med, h_lab, h_inertia, h_iter = host[b][k]
            np.testing.assert_array_equal(medoids[b, k, :K], h_med, err_msg=f"tree {b} K={K}")
            assert (medoids[b, k, K:] == -1).all()
            np.testing.assert_array_equal(labels[k, idx[b], H_BEGIN + b], h_lab, err_msg=f"tree {b} K={K}")
            assert (labels[k, out, H_BEGIN + b] == 0xFF).all()
            assert n_iter[k, H_BEGIN + b] == h_iter, (b, K)
            assert abs(inertia[k, H_BEGIN + b] - h_inertia) <= m * 2.0 ** -52 * h_inertia, (b, K)
    return host, n_iter


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_device_equals_host_pam(name):
    worst, same = margins(name)
    print(f"{name}: smallest pam_ref margin {worst:.3e}")
    assert worst >= 1e-9 and same  # the precondition (module docstring), not a tolerance
    _assert_device_equals_host(name)


def test_lattice_is_exact():
    host, _ = _assert_device_equals_host("lattice")
    _, _, Ks, _, D = _case("lattice")
    ref = pam_ref(D[0], 8)
    assert ref.ties > 0
    np.testing.assert_array_equal(host[0][Ks.index(8)][0], ref.medoids)
    got = _device("lattice")[2]
    for b in range(B):
        for k in range(len(Ks)):
            assert got[k, H_BEGIN + b] == host[b][k][2]  # integer sums: the same bits


@pytest.mark.parametrize("name", ["m130", "m257"])
def test_two_runs_are_bitwise_equal(name):
    a, b = _device(name), _device(name)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    assert a[4] == b[4]


@pytest.mark.parametrize("name", ["m65", "m257"])
def test_max_iter_one(name):
    full = _host(name)
    host, n_iter = _assert_device_equals_host(name, max_iter=1)
    _, _, Ks, _, _ = _case(name)
    seen = 0
    for b in range(B):
        for k in range(len(Ks)):
            if full[b][k][3] >= 1:
                assert n_iter[k, H_BEGIN + b] == 1
                seen += 1
    assert seen > 0
    medoids, _, _, n0, its = _device(name, max_iter=0)
    assert its == 0 and (n0[:, H_BEGIN:] == 0).all()
    for b in range(B):
        for k, K in enumerate(Ks):
            np.testing.assert_array_equal(medoids[b, k, :K], sorted(P.build(_case(name)[4][b], K)))


def test_abi_refusals():
    from consensus_clustering_amd import _lib

    lib = _lib.load()
    assert lib.cc_pam_workspace_bytes(10, 1, 1, 11) == 0 and lib.cc_pam_workspace_bytes(200, 1, 1, 128) == 0
    assert lib.cc_pam_workspace_bytes(65536, 1, 1, 2) == 0 and lib.cc_pam_workspace_bytes(10, 1, 1, 10) > 0
    D = torch.zeros((1, 4, 4), dtype=torch.float64, device="cuda")
    Ks = _dev(np.array([2], dtype=np.int32))
    ws = engine.pam_workspace(4, 1, 1, 2, "cuda")
    with pytest.raises(_lib.CCMIError, match="cc_pam_build: bad arguments"):
        _lib.call("cc_pam_build", D.data_ptr(), 1, 4, Ks.data_ptr(), 1, 2, ws.data_ptr(), ws.numel() - 1,
                  engine.stream_ptr())
    with pytest.raises(_lib.CCMIError, match="cc_pam_swap_step: bad arguments"):
        _lib.call("cc_pam_swap_step", D.data_ptr(), 1, 4, Ks.data_ptr(), 1, 5, 3, ws.data_ptr(), ws.numel(),
                  engine.stream_ptr())
    with pytest.raises(ValueError, match="needs 1 <= K <= min"):
        engine.pam_workspace(4, 1, 1, 5, "cuda")


# ---------------------------------------------------------------- end to end

E2E = dict(K_range=list(range(2, 8)), n_iterations=24, subsampling=0.8, random_state=3)
FITS = [("euclidean", np.float32), ("correlation", np.float64), ("manhattan", np.float32)]


@functools.lru_cache(maxsize=None)
def _e2e_X(dtype):
    return np.ascontiguousarray(load_fixture("blobs_n400_d8_k4")["X"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def _e2e_fit(metric, dtype, sub=False, **kw):
    cc = ConsensusClustering(clusterer=(SubPAM if sub else PAM)(metric=metric), clusterer_options={}, plot_cdf=False,
                             **dict(E2E, **kw))
    return cc.fit(_e2e_X(dtype))


def _assert_same_results(a, b):
    for K in E2E["K_range"]:
        for key in ("mij", "iij", "cij", "hist", "cdf", "bin_edges"):
            np.testing.assert_array_equal(a.cdf_at_K_data[K][key], b.cdf_at_K_data[K][key], err_msg=f"{key} K={K}")
        assert a.cdf_at_K_data[K]["pac_area"] == b.cdf_at_K_data[K]["pac_area"]
        np.testing.assert_array_equal(a.pair_counts_[K], b.pair_counts_[K])
    assert a.best_k_ == b.best_k_


@pytest.mark.parametrize("metric,dtype", FITS, ids=[f[0] for f in FITS])
def test_fit_equals_oracle_and_host(metric, dtype):
    X = _e2e_X(dtype)
    n = X.shape[0]
    cc = _e2e_fit(metric, dtype)
    assert cc.backend_ == "gpu-pam" and cc.pam_metric_ == P.METRICS[metric]
    assert cc.pam_stats_["route"] == "batched" and cc.pam_stats_["batch"] == E2E["n_iterations"]
    assert cc.pam_stats_["launches"] == 1 and cc.pam_stats_["swap_iterations"] >= 1
    ref, ref_labels = O.fit(X, E2E["K_range"], E2E["n_iterations"], E2E["subsampling"], E2E["random_state"],
                            clusterer=lambda Xs, K: PAM(n_clusters=K, metric=metric).fit_predict(Xs))
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
    # the labels themselves, not only the counts they add up to
    idx = cc.resampling_indices_
    L = cc.labels_.cpu().numpy()
    for k, K in enumerate(E2E["K_range"]):
        for h in range(E2E["n_iterations"]):
            np.testing.assert_array_equal(L[k, idx[h], h], ref_labels[K][h], err_msg=f"K={K} h={h}")
    inertia, n_iter = cc.pam_inertia_.cpu().numpy(), cc.pam_n_iter_.cpu().numpy()
    assert inertia.shape == n_iter.shape == (6, 24) and inertia.dtype == np.float64 and n_iter.dtype == np.int32
    assert (inertia > 0).all() and (n_iter >= 0).all()
    host = _e2e_fit(metric, dtype, sub=True)
    assert host.backend_ == "host-clusterer" and host.pam_stats_ is None and host.pam_metric_ is None
    assert host.pam_inertia_ is None and host.pam_n_iter_ is None
    _assert_same_results(cc, host)


def test_fit_with_feature_subsampling_under_cosine():
    cc = _e2e_fit("cosine", np.float32, feature_subsampling=0.75)
    assert cc.backend_ == "gpu-pam" and cc.pam_stats_["feature_subsampling"] == 6
    host = _e2e_fit("cosine", np.float32, sub=True, feature_subsampling=0.75)
    assert host.backend_ == "host-clusterer"
    np.testing.assert_array_equal(cc.feature_indices_, host.feature_indices_)
    _assert_same_results(cc, host)


def test_fit_on_a_device_tensor():
    cc = ConsensusClustering(clusterer=PAM(metric="correlation"), clusterer_options={}, plot_cdf=False, **E2E)
    cc.fit(torch.from_numpy(_e2e_X(np.float64)).cuda())
    assert cc.backend_ == "gpu-pam" and cc.pam_metric_ == "correlation"
    _assert_same_results(cc, _e2e_fit("correlation", np.float64))


def test_fit_in_batches_of_two_trees():
    n, m = 400, 320
    budget = 8 * n * n + 2 * engine.pam_tree_bytes(m, 6, 7) + 100
    cc = _e2e_fit("euclidean", np.float32, workspace_budget=budget)
    assert cc.backend_ == "gpu-pam" and cc.pam_stats_["batch"] == 2 and cc.pam_stats_["launches"] == 12
    whole = _e2e_fit("euclidean", np.float32)
    _assert_same_results(cc, whole)
    assert torch.equal(cc.pam_inertia_, whole.pam_inertia_) and torch.equal(cc.pam_n_iter_, whole.pam_n_iter_)
    small = ConsensusClustering(clusterer=PAM(), clusterer_options={}, plot_cdf=False,
                                workspace_budget=8 * n * n + 1000, **E2E)
    with pytest.raises(ValueError, match="cannot hold the PAM clusterer"):
        small.fit(_e2e_X(np.float32))


def test_refusals():
    X = _e2e_X(np.float32)
    Xz = X.copy()
    Xz[0] = 0.0
    # a degenerate row keeps the fit in the host loop, where PAM refuses the first resample that
    # holds row 0 (24 resamples of 80 %: one of them does) in the tree path's sentence
    cc = ConsensusClustering(clusterer=PAM(metric="cosine"), clusterer_options={}, plot_cdf=False, **E2E)
    with pytest.raises(ValueError, match="Cosine affinity cannot be used when X contains zero vectors"):
        cc.fit(Xz)
    assert cc.backend_ == "host-clusterer" and cc.pam_metric_ is None
    cc = ConsensusClustering(clusterer=PAM(metric="cosine"), clusterer_options={}, plot_cdf=False,
                             **dict(E2E, feature_subsampling=0.75))
    with pytest.raises(engine.DegenerateResample, match="Cosine affinity cannot be used when X contains zero vectors"):
        cc.fit(Xz)
    assert cc.backend_ == "gpu-pam"
    cc = ConsensusClustering(clusterer=PAM(), clusterer_options={}, plot_cdf=False,
                             **dict(E2E, K_range=[2, 17]))
    with pytest.raises(ValueError, match="Cannot extract more clusters than samples: 17 clusters were given for 16 "
                                         "samples"):
        cc.fit(X[:20])
    assert cc.backend_ == "gpu-pam"
    Xn = X.copy()
    Xn[5, 2] = np.nan
    with pytest.raises(ValueError, match=r"Input X contains NaN\."):
        ConsensusClustering(clusterer=PAM(), clusterer_options={}, plot_cdf=False, **E2E).fit(Xn)
