"""Feature subsampling on the float64 k-means (cc_kmeans_f64_cols): the gather in the per-resample
setup against the materialised column subset bit for bit, the column row under shifted h_begin and
chunked launches, sklearn's float64 fits on every resample's own rows and columns (committed
fixtures, tests/golden/make_sk_feature_fixtures.py), whole fits against the oracle's pieces, and
the refusals.  tests/test_kmeans_features_host.py holds what needs no GPU."""
import functools
import warnings

import numpy as np
import pytest
import torch

from consensus_clustering_amd import ConsensusClustering, _lib, engine, kmeans, post
from consensus_clustering_amd.kmeans import BatchedKMeans
from oracle import cc_oracle as O
from tests.conftest import digest
from tests.sk_parity import load_sk_fixture

pytestmark = pytest.mark.gpu

SEED = 3


@functools.lru_cache(maxsize=None)
def _f64_noisy_once(n, d, k):
    from sklearn.datasets import make_blobs

    X, _ = make_blobs(n_samples=n, n_features=d, centers=k, cluster_std=1.0, center_box=(-10, 10), shuffle=True,
                      random_state=n + d)
    X = X.astype(np.float32).astype(np.float64)
    X += np.random.default_rng(0).normal(scale=0.5, size=X.shape)
    return X


def _f64_noisy(n, d, k):
    """tests/golden/make_sk_fixtures.py::_f64_noisy (the rows of test_f64_labels_match_sklearn_float64)."""
    return _f64_noisy_once(n, d, k).copy()


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _run(X, idx, Ks, ranges, cols=None, grid=None):
    """run_f64 over each [h0, h1) of ranges into one set of outputs: the labels in the rows' order
    [nK, H, m] (0xFF where a resample did not run), inertia and n_iter [nK, H], the last plan."""
    n, _ = X.shape
    H, m = idx.shape
    Xd, idx_d = _dev(X), _dev(idx)
    cols_d = None if cols is None else _dev(cols)
    L = engine.new_label_matrix(len(Ks), n, engine.pad_h(H), "cuda")
    inert = torch.zeros((len(Ks), H), dtype=torch.float64, device="cuda")
    nit = torch.zeros((len(Ks), H), dtype=torch.int32, device="cuda")
    bk = BatchedKMeans(Ks, n_init=3, random_state=SEED)
    for h0, h1 in ranges:
        bk.run_f64(Xd, idx_d, n, H, m, h0, h1, L, inertia=inert, n_iter=nit, grid=grid, cols_d=cols_d)
    torch.cuda.synchronize()
    Lh = L.cpu().numpy()
    labs = np.stack([np.stack([Lh[k][idx[h], h] for h in range(H)]) for k in range(len(Ks))])
    return labs, inert.cpu().numpy(), nit.cpu().numpy(), bk.calls


def _assert_same(a, b, what):
    for x, y, name in zip(a[:3], b[:3], ("labels", "inertia", "n_iter")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}")


# ---------------------------------------------------------------- the gather

def _gather_equals_subset(X, idx, Ks, cols):
    H = idx.shape[0]
    for h in range(H):
        got = _run(X, idx, Ks, [(h, h + 1)], cols=cols)
        want = _run(np.ascontiguousarray(X[:, cols[h]]), idx, Ks, [(h, h + 1)])
        assert (want[0][:, h] != 0xFF).all() and (want[2][:, h] >= 1).all() and (want[1][:, h] > 0).all()
        others = [g for g in range(H) if g != h]
        assert (got[0][:, others] == 0xFF).all() and (got[2][:, others] == 0).all()
        _assert_same(got, want, f"resample {h}")
        assert got[3] == want[3]  # planned at the subset's width, like the plain fit of that matrix


@pytest.mark.parametrize("md", [1, 3, 4, 5, 9, 12])
def test_gather_equals_the_materialised_subset(md):
    """m = 76: four full 16-row tiles plus 12 rows, two setup row blocks; the widths cover one
    column, a partial and a full k-step of 4, one einsum block of 8 plus a tail, d - 1."""
    X = _f64_noisy(96, 13, 3)
    H, Ks = 5, [2, 3, 7]
    idx = engine.resample_indices(SEED, 96, 76, 0, H)
    cols = post.feature_indices(SEED, 13, md, H)
    assert len({tuple(c) for c in cols}) > 1  # slot 0 serves every call: another resample's row would show
    _gather_equals_subset(X, idx, Ks, cols)


def test_every_column_equals_the_plain_call():
    X = _f64_noisy(96, 13, 3)
    H, Ks = 5, [2, 3, 7]
    idx = engine.resample_indices(SEED, 96, 76, 0, H)
    cols = np.tile(np.arange(13, dtype=np.int32), (H, 1))
    got = _run(X, idx, Ks, [(0, H)], cols=cols)
    want = _run(X, idx, Ks, [(0, H)])
    assert (want[0] != 0xFF).all()
    _assert_same(got, want, "identity columns")
    assert got[3] == want[3]


def test_gather_on_wide_rows():
    """md = 257 of d = 300: the row copy's strided loop (k += 256) takes a second step."""
    X = _f64_noisy(64, 300, 3)
    idx = engine.resample_indices(SEED, 64, 51, 0, 2)
    _gather_equals_subset(X, idx, [2, 3], post.feature_indices(SEED, 300, 257, 2))


# ---------------------------------------------------------------- offsets

def test_column_row_follows_the_resample_not_the_slot(monkeypatch):
    """[0, 7) in one call, as [0, 3) then [3, 7) (h_begin = 3 on slot 0) and on a grid of 2
    workgroups (several launches, each with a shifted h_begin), for one-K and two-K units: the
    same labels, inertia and n_iter bit for bit."""
    X = _f64_noisy(96, 13, 3)
    H, Ks = 7, [2, 3, 7]
    idx = engine.resample_indices(SEED, 96, 76, 0, H)
    cols = post.feature_indices(SEED, 13, 5, H)
    assert len({tuple(c) for c in cols}) == H  # a row taken from another resample would show
    first = None
    for kpack in ("1", "2"):
        monkeypatch.setenv("CCMI_F64_KPACK", kpack)
        whole = _run(X, idx, Ks, [(0, H)], cols=cols)
        assert (whole[0] != 0xFF).all() and (whole[2] >= 1).all()
        _assert_same(_run(X, idx, Ks, [(0, 3), (3, H)], cols=cols), whole, f"kpack {kpack}: two calls")
        _assert_same(_run(X, idx, Ks, [(0, H)], cols=cols, grid=2), whole, f"kpack {kpack}: grid 2")
        first = first or whole
        _assert_same(whole, first, "kpack 2 against 1")


# ---------------------------------------------------------------- sklearn

# case: n, d, k_true, md, Ks, H
SK_CASES = [("n600_d12", 600, 12, 4, 9, [2, 3, 4, 6, 9], 4),
            ("n29_d29", 29, 29, 3, 23, [2, 3, 4, 5, 6, 7, 8, 9, 10], 6),
            ("n300_d150", 300, 150, 3, 120, [2, 3, 5], 3),
            ("n200_d4", 200, 4, 3, 3, [2, 3, 5], 4)]


@pytest.mark.parametrize("case,n,d,k_true,md,Ks,H", SK_CASES)
def test_labels_match_sklearn_float64_on_the_subset(case, n, d, k_true, md, Ks, H):
    """sklearn's float64 KMeans on ascontiguousarray(X[idx[h]][:, cols[h]]): every (K, h)
    identical in labels and n_iter, inertia within 1e-12 relative (the plain engine's bound,
    test_f64_labels_match_sklearn_float64)."""
    f = load_sk_fixture("f64_feat_" + case)
    meta = f["meta"]
    X = _f64_noisy(n, d, k_true)
    assert digest(X) == meta["x_sha256"]
    assert (meta["n"], meta["d"], meta["md"], meta["Ks"], meta["H"], meta["seed"]) == (n, d, md, Ks, H, SEED)
    m = int(0.8 * n)
    idx = engine.resample_indices(SEED, n, m, 0, H)
    labs, inert, nit, _ = _run(X, idx, Ks, [(0, H)], cols=f["cols"])
    bad, rel = [], 0.0
    for k, K in enumerate(Ks):
        for h in range(H):
            if digest(labs[k, h].astype(np.int8)) != f["digest64"][k, h] or nit[k, h] != f["n_iter"][k, h]:
                bad.append((K, h, int(nit[k, h]), int(f["n_iter"][k, h])))
            rel = max(rel, abs(inert[k, h] - f["inertia"][k, h]) / f["inertia"][k, h])
    print(f"f64 features [{case}, md = {md}]: {len(Ks) * H - len(bad)}/{len(Ks) * H} identical to sklearn float64 "
          f"(labels, n_iter); max relative inertia difference {rel:.2e}; differing {bad}")
    assert not bad, bad
    assert rel <= 1e-12, rel


# ---------------------------------------------------------------- whole fits

FIT = dict(n_iterations=4, subsampling=0.8, random_state=SEED, feature_subsampling=0.8, plot_cdf=False)


def _fit_quiet(X, **kw):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        cc = ConsensusClustering(**{**FIT, **kw}).fit(X)
    user = [str(w.message) for w in rec if issubclass(w.category, UserWarning)]
    assert not user, user
    return cc


@pytest.mark.parametrize("where", ["numpy", "device"])
def test_fit_equals_the_oracle_on_sklearn_labels(where):
    f = load_sk_fixture("f64_feat_n600_d12")
    X = _f64_noisy(600, 12, 4)
    assert digest(X) == f["meta"]["x_sha256"]
    n, Ks, H = 600, f["meta"]["Ks"], 4
    cc = _fit_quiet(_dev(X) if where == "device" else X, K_range=Ks)
    assert cc.backend_ == "gpu-kmeans" and cc.precision_ == "f64"
    assert cc.feature_indices_.dtype == np.int32
    np.testing.assert_array_equal(cc.feature_indices_, f["cols"])
    np.testing.assert_array_equal(cc.kmeans_n_iter_.cpu().numpy(), f["n_iter"])
    inert = cc.kmeans_inertia_.cpu().numpy()
    assert inert.dtype == np.float64 and (np.abs(inert - f["inertia"]) <= 1e-12 * f["inertia"]).all()
    assert cc.kmeans_stats_ is not None
    idx = O.subsampling_indices(n, H, 0.8, SEED)
    I = O.cosample_matrix(idx, n)
    for k, K in enumerate(Ks):
        g = cc.cdf_at_K_data[K]
        r = O.analyse(O.coassoc_matrix(idx, f["labels"][k].astype(np.int64), K, n), I, dtype=O.reference_dtype(H))
        for key in ("mij", "iij", "hist", "cdf"):
            np.testing.assert_array_equal(g[key], r[key], err_msg=f"{key} K={K}")
        assert g["pac_area"] == r["pac_area"], K


def test_float32_input_keeps_the_host_loop_unless_f64_is_asked():
    f = load_sk_fixture("f64_feat_n600_d12")
    X32 = _f64_noisy(600, 12, 4).astype(np.float32)
    Ks = [2, 3]
    with pytest.warns(UserWarning, match="^the k-means engines do not subsample features: with "
                                         "feature_subsampling < 1 the KMeans fits run on the host"):
        host = ConsensusClustering(K_range=Ks, **FIT).fit(X32)
    assert host.backend_ == "host-clusterer" and host.precision_ is None and host.kmeans_n_iter_ is None
    with pytest.warns(UserWarning, match="k-means engines do not subsample features"):
        fast = ConsensusClustering(K_range=Ks, precision="fast", **FIT).fit(_f64_noisy(600, 12, 4))
    assert fast.backend_ == "host-clusterer" and fast.precision_ is None
    cc = _fit_quiet(X32, K_range=Ks, precision="f64")
    assert cc.backend_ == "gpu-kmeans" and cc.precision_ == "f64"
    np.testing.assert_array_equal(cc.feature_indices_, f["cols"])
    np.testing.assert_array_equal(cc.feature_indices_, host.feature_indices_)
    assert (cc.kmeans_n_iter_.cpu().numpy() >= 1).all()
    with pytest.raises(ValueError, match="precision must be"):
        ConsensusClustering(K_range=Ks, precision="double", **FIT).fit(X32)


# ---------------------------------------------------------------- refusals

def test_run_f64_refuses_bad_columns_before_the_launch():
    X = _f64_noisy(96, 13, 3)
    H, m, Ks = 3, 76, [2, 3]
    idx = engine.resample_indices(SEED, 96, m, 0, H)
    good = post.feature_indices(SEED, 13, 5, H)
    Xd, idx_d = _dev(X), _dev(idx)
    L = engine.new_label_matrix(len(Ks), 96, engine.pad_h(H), "cuda")
    nit = torch.zeros((len(Ks), H), dtype=torch.int32, device="cuda")

    def run(cols_d):
        BatchedKMeans(Ks, n_init=3, random_state=SEED).run_f64(Xd, idx_d, 96, H, m, 0, H, L, n_iter=nit, cols_d=cols_d)

    for value in (13, -1, 2**31 - 1):
        c = good.copy()
        c[2, 4] = value
        with pytest.raises(ValueError, match=r"cols entries must lie in \[0, 13\)"):
            run(_dev(c))
    with pytest.raises(ValueError, match=r"cols_d must be \[H, md\]"):
        run(_dev(np.zeros((H, 14), dtype=np.int32)))  # md > d
    with pytest.raises(ValueError, match=r"cols_d must be \[H, md\]"):
        run(_dev(good[:2]))  # a row per resample
    with pytest.raises(ValueError, match=r"cols_d must be \[H, md\]"):
        run(_dev(good[0]))
    with pytest.raises(ValueError, match="int32 tensor on X's device"):
        run(_dev(good.astype(np.int64)))
    with pytest.raises(ValueError, match="int32 tensor on X's device"):
        run(torch.from_numpy(good.copy()))
    torch.cuda.synchronize()
    assert bool((L == 0xFF).all()) and bool((nit == 0).all())  # nothing ran


def test_c_entry_point_refusals():
    n, d, md, H, m, Ks = 20, 6, 3, 2, 16, np.array([2, 3], dtype=np.int32)
    X = _dev(np.random.RandomState(0).randn(n, d))
    idx = _dev(engine.resample_indices(SEED, n, m, 0, H))
    cols = _dev(post.feature_indices(SEED, d, md, H))
    u, pos, stride = kmeans.kpp_tables(Ks, 3, SEED, m, np.float64)
    u_d, pos_d = _dev(u), _dev(pos)
    L = engine.new_label_matrix(len(Ks), n, engine.pad_h(H), "cuda")
    grid = 4
    need = int(_lib.load().cc_kmeans_f64_workspace_bytes(m, md, Ks.ctypes.data, len(Ks), grid, H))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(cols_ptr=cols.data_ptr(), md=md, nbytes=need):
        _lib.call("cc_kmeans_f64_cols", X.data_ptr(), n, d, cols_ptr, md, idx.data_ptr(), H, m, 0, H,
                  Ks.ctypes.data, len(Ks), 3, 300, 1e-4, u_d.data_ptr(), stride, pos_d.data_ptr(), L.data_ptr(),
                  L.stride(1), None, None, ws.data_ptr(), nbytes, grid, engine.stream_ptr())

    with pytest.raises(_lib.CCMIError, match="cc_kmeans_f64_cols: cols is null"):
        call(cols_ptr=None)
    for bad in (d + 1, 0, -2):
        with pytest.raises(_lib.CCMIError, match=f"cc_kmeans_f64_cols: need 1 <= md <= d, got md = {bad}, d = {d}"):
            call(md=bad)
    with pytest.raises(_lib.CCMIError, match="cc_kmeans_f64_cols: cols must be 4-B aligned"):
        call(cols_ptr=cols.data_ptr() + 2)
    with pytest.raises(_lib.CCMIError, match="cc_kmeans_f64_cols: workspace too small"):
        call(nbytes=need - 1)
    torch.cuda.synchronize()
    assert bool((L == 0xFF).all())  # nothing ran
    call()  # the arguments above are otherwise good
    torch.cuda.synchronize()
    got = L.cpu().numpy()
    idx_h = idx.cpu().numpy()
    for h in range(H):
        for k, K in enumerate(Ks):
            assert sorted(set(got[k, idx_h[h], h].tolist())) == list(range(K))
