"""The full-covariance GMM base clusterer on the device (csrc/gmm_full.hip, engine.gmm_labels with
covariance='full', backend 'gpu-gmm') against the sklearn fixtures of
tests/golden/make_gmm_full_fixtures.py, which keep a case only where sklearn, the host form and
the host form on reordered rows and columns decide every problem alike, so the comparisons here
are exact on the decisions; the lower bound is held to the fixture's lb_rtol."""
import warnings

import numpy as np
import pytest
import torch

from consensus_clustering_amd import GMM, ConsensusClustering, FullGMM, engine, post
from tests.test_gmm_full_host import SubFullGMM, load_case

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _run(X, idx, Ks, ranges, cols=None, n_init=1, seed=3, budget=None, **kw):
    """engine.gmm_labels(covariance='full') over each [h0, h1) of ranges into one set of outputs:
    the labels in the rows' order [nK, H, m], lower bound, n_iter and converged [nK, H], the stats
    of the last range."""
    n = X.shape[0]
    H, m = idx.shape
    Xd, idx_d = _dev(np.asarray(X, dtype=np.float64)), _dev(idx.astype(np.int32))
    cols_d = None if cols is None else _dev(cols.astype(np.int32))
    nK = len(Ks)
    labels = engine.new_label_matrix(nK, n, engine.pad_h(H), "cuda")
    lb = torch.zeros((nK, H), dtype=torch.float64, device="cuda")
    nit = torch.zeros((nK, H), dtype=torch.int32, device="cuda")
    conv = torch.zeros((nK, H), dtype=torch.uint8, device="cuda")
    stats = None
    for h0, h1 in ranges:
        stats = engine.gmm_labels(Xd, idx_d, h0, h1, Ks, labels, budget=budget, n_init=n_init, seed=seed,
                                  cols_d=cols_d, lower_bound=lb, n_iter=nit, converged=conv, covariance='full', **kw)
    torch.cuda.synchronize()
    L = labels.cpu().numpy()
    rows = np.stack([L[:, idx[h], h] for h in range(H)], axis=1)  # [nK, H, m]
    return rows, lb.cpu().numpy(), nit.cpu().numpy(), conv.cpu().numpy().astype(bool), stats


def _check_case(case, alone=False):
    fx, meta, X = load_case(case)
    idx, Ks, H = fx["idx"], meta["Ks"], meta["H"]
    cols = None if meta["md"] == meta["d"] else fx["cols"]
    rtol = float(fx["lb_rtol"])
    first = None
    for n_init in sorted(meta["n_inits"]):
        lab, lb, nit, conv, stats = _run(X, idx, Ks, [(0, H)], cols, n_init, meta["seed"])
        assert stats["route"] == "batched" and stats["inits"] == n_init
        ref = fx[f"lower_bound_{n_init}"]
        err = np.abs(lb - ref) / np.abs(ref)
        print(f"{case} n_init={n_init}: n_iter {nit.min()}..{nit.max()}, lower bound within {err.max():.3e} "
              f"(lb_rtol {rtol:.3e})")
        np.testing.assert_array_equal(nit, fx[f"n_iter_{n_init}"])
        np.testing.assert_array_equal(conv, fx[f"converged_{n_init}"])
        np.testing.assert_array_equal(lab, fx[f"labels_{n_init}"])
        assert (err <= rtol).all(), err.max()
        if n_init == 1:
            first = lb
        else:
            # the winning init: a later init wins with a strictly larger bound than the first's,
            # which is the n_init = 1 run's, bit for bit (the same stream, the same sums)
            np.testing.assert_array_equal(lb != first, fx[f"win_{n_init}"] != 0)
        if alone:
            for h in range(H):
                one = _run(X, idx, Ks, [(h, h + 1)], cols, n_init, meta["seed"])
                np.testing.assert_array_equal(one[1][:, h], lb[:, h])  # bitwise
                np.testing.assert_array_equal(one[0][:, h], lab[:, h])
                np.testing.assert_array_equal(one[2][:, h], nit[:, h])


@pytest.mark.parametrize("md", [1, 3, 4, 5, 15, 16, 17])
def test_kernels_equal_the_fixtures(md):
    _check_case(f"n200_md{md}", alone=True)


def test_three_tile_rows():
    _check_case("n400_md33")


def test_second_component_tile():
    _check_case("n400_k20", alone=True)  # md = 3: each resample alone equals the batch, as for the n200 cases


def test_partial_row_tile_and_partial_step_of_rows():
    """m = 77 is no multiple of 16 (the last row tile of the E-step holds 13 rows) nor of 4 (the last
    step of the chains over the rows in the means and covariance kernels holds 1): the device
    against the host FullGMM on the same rows.  The case was screened like the fixtures: on the
    CPU the host form and the host form on permuted rows with reversed columns agree on every
    label and n_iter (2, and 12 at h = 0, K = 4) and on the bound to 3.9e-16, so the comparison is
    exact on the decisions and holds the bound to the fixtures' floor of 1e-13."""
    n, m, seed, Ks = 96, 77, 3, [1, 2, 3, 4]
    X = _blobs64(n, 5, 3)
    idx = np.stack([np.random.RandomState(seed + h).choice(n, size=m, replace=False) for h in range(2)])
    lab, lb, nit, conv, _ = _run(X, idx, Ks, [(0, 2)], None, 1, seed)
    for h in range(2):
        for k, K in enumerate(Ks):
            ref = FullGMM(n_components=K, random_state=seed).fit(X[idx[h]])
            tag = f"h={h} K={K}"
            print(f"{tag}: n_iter {nit[k, h]} / {ref.n_iter_}, bound {lb[k, h]!r} / {ref.lower_bound_!r}")
            np.testing.assert_array_equal(lab[k, h], ref.labels_, err_msg=tag)
            assert nit[k, h] == ref.n_iter_ and conv[k, h] == ref.converged_, tag
            assert abs(lb[k, h] - ref.lower_bound_) <= 1e-13 * abs(ref.lower_bound_), tag
    assert nit.max() >= 10  # one problem iterates well past the two of the separated ones


def test_md_limit_and_the_largest_lds_stage():
    _check_case("n700_md128")


def test_invariant_under_batching_and_repeatable():
    fx, meta, X = load_case("n200_md5")
    H, m, Ks = 7, meta["m"], [2, 3, 5, 17]
    idx = np.stack([np.random.RandomState(3 + h).choice(meta["n"], size=m, replace=False) for h in range(H)])
    cols = post.feature_indices(3, meta["d"], 5, H)
    whole = _run(X, idx, Ks, [(0, H)], cols, 3)
    assert whole[4]["batch"] == H
    split = _run(X, idx, Ks, [(0, 3), (3, H)], cols, 3)
    per = engine.gmm_full_bytes(m, 5, Ks) + len(Ks) * meta["n"]
    single = _run(X, idx, Ks, [(0, H)], cols, 3, budget=1024 + 127 * len(Ks) * meta["n"] + per + per // 2)
    assert single[4]["batch"] == 1 and single[4]["launches"] == H
    again = _run(X, idx, Ks, [(0, H)], cols, 3)
    for other in (split, single, again):
        for a, b in zip(whole[:4], other[:4]):
            np.testing.assert_array_equal(a, b)  # the lower bound bitwise


def _blobs64(n, d, k):
    from sklearn.datasets import make_blobs

    X, _ = make_blobs(n_samples=n, n_features=d, centers=k, cluster_std=1.0, center_box=(-10, 10), shuffle=True,
                      random_state=n + d)
    X = X.astype(np.float32).astype(np.float64)
    return X + np.random.default_rng(0).normal(scale=0.5, size=X.shape)


def _fit(est, X, **kw):
    cc = ConsensusClustering(clusterer=est, K_range=range(2, 7), n_iterations=24, random_state=5, plot_cdf=False,
                             **kw)
    return cc.fit(X)


def _same_consensus(a, b):
    assert a.best_k_ == b.best_k_
    for K in a.cdf_at_K_data:
        ra, rb = a.cdf_at_K_data[K], b.cdf_at_K_data[K]
        for key in ("mij", "iij", "hist", "cdf"):
            np.testing.assert_array_equal(ra[key], rb[key], err_msg=f"K={K} {key}")
        assert ra["pac_area"] == rb["pac_area"]
        assert np.abs(ra["cij"] - rb["cij"]).max() <= 1e-6


@pytest.fixture(scope="module")
def end_to_end():
    X = _blobs64(600, 12, 4)
    return X, _fit(FullGMM(), X), _fit(SubFullGMM(), X)


def test_end_to_end_equals_the_host_loop(end_to_end):
    X, dev, host = end_to_end
    assert dev.backend_ == "gpu-gmm" and host.backend_ == "host-clusterer"
    assert dev.gmm_covariance_type_ == "full" and host.gmm_covariance_type_ is None
    nK, H = 5, 24
    for t, dt in ((dev.gmm_lower_bound_, torch.float64), (dev.gmm_n_iter_, torch.int32),
                  (dev.gmm_converged_, torch.uint8)):
        assert t.is_cuda and t.dtype == dt and tuple(t.shape) == (nK, H)
    assert int(dev.gmm_n_iter_.min()) >= 1 and int(dev.gmm_n_iter_.max()) <= 100
    assert bool(torch.isfinite(dev.gmm_lower_bound_).all())
    s = dev.gmm_stats_
    assert s["route"] == "batched" and s["inits"] == 3 and s["em_iterations"] >= 3 and "feature_subsampling" not in s
    assert host.gmm_stats_ is None and host.gmm_lower_bound_ is None and host.gmm_n_iter_ is None
    assert host.gmm_converged_ is None and dev.pam_stats_ is None and dev.kmeans_stats_ is None
    _same_consensus(dev, host)


def test_end_to_end_feature_subsampling(end_to_end):
    X = end_to_end[0]
    dev, host = _fit(FullGMM(), X, feature_subsampling=0.75), _fit(SubFullGMM(), X, feature_subsampling=0.75)
    assert dev.backend_ == "gpu-gmm" and host.backend_ == "host-clusterer"
    assert dev.gmm_covariance_type_ == "full" and dev.gmm_stats_["feature_subsampling"] == 9
    np.testing.assert_array_equal(dev.feature_indices_, host.feature_indices_)
    _same_consensus(dev, host)


def test_the_diagonal_model_is_unchanged_and_tells_its_type(end_to_end):
    X, full, _ = end_to_end
    diag = _fit(GMM(), X)
    assert diag.backend_ == "gpu-gmm" and diag.gmm_covariance_type_ == "diag"
    assert diag.gmm_stats_["route"] == "batched" and diag.gmm_stats_["inits"] == 3
    # the diagonal kernels through the engine's default and through the covariance argument
    n, H, m = X.shape[0], 4, 480
    idx = np.stack([np.random.RandomState(h).choice(n, size=m, replace=False) for h in range(H)]).astype(np.int32)
    out = []
    for kw in ({}, dict(covariance='diag')):
        labels = engine.new_label_matrix(2, n, engine.pad_h(H), "cuda")
        lb = torch.zeros((2, H), dtype=torch.float64, device="cuda")
        engine.gmm_labels(_dev(X), _dev(idx), 0, H, [2, 4], labels, n_init=1, seed=5, lower_bound=lb, **kw)
        out.append((labels.cpu().numpy(), lb.cpu().numpy()))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert not torch.equal(diag.gmm_lower_bound_, full.gmm_lower_bound_)  # another model
    with pytest.raises(ValueError, match="covariance must be 'diag' or 'full'"):
        engine.gmm_labels(_dev(X), _dev(idx), 0, H, [2], labels, covariance='tied')


def test_float32_input_warns_once_and_is_cast(end_to_end):
    X, dev64, _ = end_to_end
    X32 = X.astype(np.float32)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        dev = _fit(FullGMM(), X32)
    assert len([x for x in w if "GMM computes in float64" in str(x.message)]) == 1
    assert dev.backend_ == "gpu-gmm" and dev.gmm_covariance_type_ == "full"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ref = _fit(FullGMM(), X32.astype(np.float64))
    assert not [x for x in w if "float64" in str(x.message)]  # float64 input: nothing warns
    assert torch.equal(dev.gmm_lower_bound_, ref.gmm_lower_bound_) and torch.equal(dev.labels_, ref.labels_)
    assert torch.equal(dev.gmm_n_iter_, ref.gmm_n_iter_)


def test_more_than_128_features_fit_on_the_host_with_a_warning():
    X = _blobs64(170, 129, 2)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        cc = ConsensusClustering(clusterer=FullGMM(), clusterer_options={}, K_range=[2], n_iterations=2,
                                 random_state=0, plot_cdf=False).fit(X)
    assert cc.backend_ == "host-clusterer" and cc.gmm_stats_ is None and cc.gmm_covariance_type_ is None
    assert len([x for x in w if "at most 128 features" in str(x.message) and "129" in str(x.message)]) == 1
    # 128 of the 129 columns stay on the device
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cc = ConsensusClustering(clusterer=FullGMM(), clusterer_options={}, K_range=[2], n_iterations=2,
                                 random_state=0, plot_cdf=False, feature_subsampling=0.995).fit(X)
    assert cc.backend_ == "gpu-gmm" and cc.gmm_stats_["feature_subsampling"] == 128


def test_subclass_and_sklearn_stay_on_the_host():
    from sklearn.mixture import GaussianMixture

    X = _blobs64(60, 3, 2)
    for est in (GaussianMixture(), SubFullGMM()):
        cc = ConsensusClustering(clusterer=est, clusterer_options={}, K_range=[2], n_iterations=3, random_state=0,
                                 plot_cdf=False).fit(X)
        assert cc.backend_ == "host-clusterer" and cc.gmm_stats_ is None and cc.gmm_covariance_type_ is None


def test_ill_defined_covariance_raises_from_the_device():
    X = np.repeat(np.array([[0.0, 1.0], [4.0, 2.0], [9.0, -3.0]]), 8, axis=0)  # duplicated points
    cc = ConsensusClustering(clusterer=FullGMM(reg_covar=0.0), clusterer_options={}, K_range=[2, 3], n_iterations=3,
                             random_state=0, plot_cdf=False)
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        cc.fit(X)
    assert cc.backend_ == "gpu-gmm" and cc.gmm_covariance_type_ == "full"
    idx = np.stack([np.arange(24, dtype=np.int32)])
    with pytest.raises(engine.IllDefinedMixture):
        _run(X, idx, [3], [(0, 1)], reg_covar=0.0)
    lab, lb, nit, conv, _ = _run(X, idx, [3], [(0, 1)])  # reg_covar carries the covariances
    assert np.isfinite(lb).all() and len(np.unique(lab)) == 3


def test_refusals_before_any_launch():
    X = _blobs64(60, 3, 2)

    def fit(X, **kw):
        return ConsensusClustering(clusterer=FullGMM(), K_range=kw.pop("Ks", [2, 3]), n_iterations=4, random_state=0,
                                   plot_cdf=False, **kw).fit(X)

    with pytest.raises(ValueError, match="Expected n_samples >= n_components but got n_components = 49, n_samples = 48"):
        fit(X, Ks=[2, 49])
    with pytest.raises(ValueError, match="workspace_budget = 1000 bytes cannot hold the GMM clusterer"):
        fit(X, workspace_budget=1000)
    bad = X.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match="Input X contains NaN."):
        fit(bad)
    bad[7, 1] = np.inf
    with pytest.raises(ValueError, match="Input X contains infinity"):
        fit(torch.from_numpy(bad).cuda())
    with pytest.raises(ValueError, match="GMM on the device needs .* at most 128 features"):
        engine.gmm_workspace(200, 129, 1, np.asarray([2], dtype=np.int32), "cuda", 'full')
