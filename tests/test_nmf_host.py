"""The host form of the NMF base clusterer (consensus_clustering_amd/nmf.py) against sklearn's NMF and
the fixtures of tests/golden/make_nmf_fixtures.py, the estimator's protocol and refusals, the device
route's decision (_nmf_spec), the declared entry points and the batch planner.  No GPU."""
import glob
import hashlib
import json
import os
import pickle
import re

import numpy as np
import pytest
from sklearn.base import clone

import consensus_clustering_amd
from consensus_clustering_amd import NMF, _lib, api, engine
from consensus_clustering_amd import nmf as N

HERE = os.path.dirname(os.path.abspath(__file__))
SK = os.path.join(HERE, "golden", "sk")
CASES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(SK, "nmf_*.npz")))
ENTRY_POINTS = ("cc_nmf_workspace_bytes", "cc_nmf_start", "cc_nmf_steps", "cc_nmf_finish")


class SubNMF(NMF):
    """A subclass: never routed to the device."""


def nonneg_rows(n, d, k, noise=0):
    """abs(centres ~ U(0, 10) + N(0, 1)) through float32: the fixture generator's blobs."""
    rng = np.random.default_rng([n, d, noise])
    centres = rng.uniform(0.0, 10.0, size=(k, d))
    member = rng.integers(0, k, size=n)
    return np.abs(centres[member] + rng.standard_normal((n, d))).astype(np.float32).astype(np.float64)


def load_case(case):
    """(fixture arrays, meta, X): the rows are rebuilt from the recorded recipe and checked
    against the recorded digest."""
    fx = np.load(os.path.join(SK, f"nmf_{case}.npz"))
    meta = json.loads(str(fx["meta"]))
    n, d = meta["n"], meta["d"]
    X = nonneg_rows(n, d, meta["k_true"], meta["noise"])
    X[fx["idx"][0, 0]] = 0.0
    X[:, 1 % d] = 0.0
    a = np.ascontiguousarray(X)
    sha = hashlib.sha256(a.view(np.uint8).tobytes() + str(a.dtype).encode() + str(a.shape).encode()).hexdigest()
    assert sha == meta["x_sha256"], "the fixture's rows are not reproduced here"
    return fx, meta, X


def test_the_fixture_cases_are_all_there():
    assert CASES == sorted([f"n96_md{md}" for md in (1, 3, 4, 5, 12, 13)] + ["n300_md120", "n160_k127",
                                                                            "n96_md5_default"])


def test_the_fixtures_reach_both_exits_and_the_edge_rows():
    stopped, ran_out = 0, 0
    for case in CASES:
        fx, meta, X = load_case(case)
        assert (X >= 0).all() and not X[fx["idx"][0, 0]].any() and not X[:, 1 % meta["d"]].any()
        assert 1e-13 <= float(fx["err_tol"]) < 1e-9
        np.testing.assert_array_equal(fx["has3"], [K >= 2 and meta["md"] >= 3 for K in meta["Ks"]])
        stopped += int(fx["converged_1"].sum())
        ran_out += int((~fx["converged_1"]).sum())
        assert (fx["n_iter_1"][fx["converged_1"]] % 10 == 0).all()
        assert (fx["n_iter_1"][~fx["converged_1"]] == meta["max_iter"]).all()
    assert stopped > 50 and ran_out > 10


@pytest.mark.parametrize("case", CASES)
def test_host_form_equals_sklearn_and_the_fixture(case):
    from sklearn.decomposition import NMF as SkNMF
    from sklearn.exceptions import ConvergenceWarning
    import warnings

    fx, meta, X = load_case(case)
    tol, max_iter, err_tol = meta["tol"], meta["max_iter"], float(fx["err_tol"])
    for h in range(meta["H"]):
        rows = np.ascontiguousarray(X[fx["idx"][h]][:, fx["cols"][h]])
        for k, K in enumerate(meta["Ks"]):
            tag = f"h={h} K={K}"
            est = NMF(n_components=K, random_state=meta["seed"], tol=tol, max_iter=max_iter)
            W = est.fit_transform(rows)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", ConvergenceWarning)
                sk = SkNMF(K, init='random', solver='mu', random_state=meta["seed"], tol=tol, max_iter=max_iter)
                Wsk = sk.fit_transform(rows)
            np.testing.assert_array_equal(W, Wsk, err_msg=tag)  # bitwise
            np.testing.assert_array_equal(est.components_, sk.components_, err_msg=tag)
            assert est.n_iter_ == sk.n_iter_ and est.reconstruction_err_ == sk.reconstruction_err_, tag
            assert W is est.W_ and W.shape == (rows.shape[0], K) and est.components_.shape == (K, rows.shape[1])
            for n_init in meta["n_inits"]:
                if n_init > 1:
                    if not fx["has3"][k]:
                        continue
                    est = NMF(n_components=K, n_init=n_init, random_state=meta["seed"], tol=tol,
                              max_iter=max_iter).fit(rows)
                np.testing.assert_array_equal(est.labels_, fx[f"labels_{n_init}"][k, h], err_msg=tag)
                assert est.n_iter_ == fx[f"n_iter_{n_init}"][k, h], tag
                assert est.converged_ == fx[f"converged_{n_init}"][k, h], tag
                assert est.best_init_ == fx[f"win_{n_init}"][k, h], tag
                ref, err0 = fx[f"err_{n_init}"][k, h], fx[f"err0_{n_init}"][k, h]
                assert abs(est.reconstruction_err_ - ref) <= err_tol * (err0 if err0 > 0 else 1.0), tag


def test_the_label_rule_is_scale_free_and_takes_the_first_index():
    W = np.array([[1.0, 3.0], [2.0, 1.0], [0.0, 0.0], [2.0, 1.0]])
    H = np.array([[4.0, 3.0], [1.0, 0.0]])  # row norms 5 and 1
    np.testing.assert_array_equal(N.labels_of(W, H), [0, 0, 0, 0])
    np.testing.assert_array_equal(W.argmax(1), [1, 0, 0, 0])
    s = np.array([0.25, 8.0])
    np.testing.assert_array_equal(N.labels_of(W * s, H / s[:, None]), N.labels_of(W, H))
    np.testing.assert_array_equal(N.labels_of(np.array([[1.0, 5.0], [3.0, 15.0]]), H), [0, 0])  # ties: the first


def test_n_init_continues_the_stream():
    X = nonneg_rows(60, 6, 3)
    rs = np.random.RandomState(7)
    normals = [N.init_normals(rs, 60, 6, 3) for _ in range(3)]
    best, win, lab, runs = N.fit_from_normals(X, normals, 3, 1e-4, 200)
    est = NMF(3, n_init=3, random_state=7).fit(X)
    errs = [r["reconstruction_err"] for r in runs]
    assert est.best_init_ == win == int(np.argmin(errs)) and est.reconstruction_err_ == min(errs)
    np.testing.assert_array_equal(est.labels_, lab)
    one = NMF(3, n_init=1, random_state=7).fit(X)
    assert one.reconstruction_err_ == errs[0] and one.best_init_ == 0
    # the second init is the fit from the stream's next draws, not a reseeded one
    rs = np.random.RandomState(7)
    N.init_normals(rs, 60, 6, 3)
    W2, H2 = N.init_normals(rs, 60, 6, 3)
    np.testing.assert_array_equal(W2, normals[1][0])
    assert len({round(e, 12) for e in errs}) > 1


def test_zero_input_and_float32_and_integer_input():
    Z = np.zeros((12, 4))
    est = NMF(2, random_state=0, max_iter=30).fit(Z)
    assert est.n_iter_ == 30 and not est.converged_ and est.reconstruction_err_ == 0.0 and not est.labels_.any()
    X = nonneg_rows(40, 3, 2)
    a = NMF(2, random_state=0).fit(X.astype(np.float32))
    b = NMF(2, random_state=0).fit(X)
    assert a.W_.dtype == np.float64 and a.reconstruction_err_ == b.reconstruction_err_
    np.testing.assert_array_equal(a.labels_, b.labels_)
    c = NMF(2, random_state=0).fit(np.arange(12).reshape(4, 3))
    assert c.W_.dtype == np.float64 and c.labels_.shape == (4,)


def test_params_clone_pickle_repr():
    est = NMF(n_components=3, tol=1e-3, n_init=2, random_state=7)
    p = est.get_params()
    assert p == dict(n_components=3, tol=1e-3, max_iter=200, n_init=2, random_state=7)
    assert NMF().get_params() == dict(n_components=1, tol=1e-4, max_iter=200, n_init=1, random_state=None)
    assert NMF().set_params(**p).get_params() == p
    assert NMF().set_params(n_init=3, random_state=5).get_params() == dict(n_components=1, tol=1e-4, max_iter=200,
                                                                           n_init=3, random_state=5)
    assert clone(est).get_params() == p and type(clone(SubNMF(2))) is SubNMF
    fitted = pickle.loads(pickle.dumps(est.fit(nonneg_rows(20, 3, 2))))
    assert fitted.get_params() == p
    np.testing.assert_array_equal(fitted.labels_, est.labels_)
    assert repr(est) == "NMF(n_components=3, tol=0.001, max_iter=200, n_init=2, random_state=7)"
    assert repr(SubNMF()).startswith("SubNMF(")
    with pytest.raises(ValueError, match=r"Invalid parameter 'n_clusters' for estimator NMF\(\)"):
        est.set_params(n_clusters=2)
    assert consensus_clustering_amd.NMF is NMF
    assert "sqrt(sum_j H[k, j]**2)" in NMF.__doc__ and "W.argmax(1)" in NMF.__doc__


def test_the_module_needs_neither_torch_nor_the_engine():
    import subprocess
    import sys

    code = ("import sys; import consensus_clustering_amd.nmf; "
            "assert 'torch' not in sys.modules and 'consensus_clustering_amd.engine' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(HERE))


def test_set_clusterer_K_with_the_default_options():
    cc = consensus_clustering_amd.ConsensusClustering(clusterer=NMF(), K_range=[4], random_state=11, plot_cdf=False)
    cc._K = 4
    cc._set_clusterer_K()
    p = cc.clusterer.get_params()
    assert (p["n_components"], p["random_state"], p["n_init"]) == (4, 11, 3)


@pytest.mark.parametrize("params, match", [
    (dict(n_components=0), "'n_components' parameter of NMF must be an int in the range \\[1, inf\\)"),
    (dict(n_components=2.0), "'n_components' parameter"),
    (dict(n_components=True), "'n_components' parameter"),
    (dict(max_iter=0), "'max_iter' parameter of NMF must be an int in the range \\[1, inf\\)"),
    (dict(n_init=0), "'n_init' parameter of NMF must be an int"),
    (dict(n_init=1.5), "'n_init' parameter"),
    (dict(tol=-1e-3), "'tol' parameter of NMF must be a float in the range \\[0.0, inf\\)"),
    (dict(tol=float('nan')), "'tol' parameter"),
])
def test_parameter_refusals(params, match):
    X = nonneg_rows(20, 2, 2)
    with pytest.raises(ValueError, match=match):
        NMF(**{**dict(n_components=2), **params}).fit(X)


def test_data_refusals():
    X = nonneg_rows(20, 2, 2)
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="Input X contains NaN."):
        NMF(2).fit(bad)
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="Input X contains infinity"):
        NMF(2).fit(bad)
    bad[3, 1] = -1e-9
    with pytest.raises(ValueError, match=r"Negative values in data passed to NMF \(input X\)\."):
        NMF(2).fit(bad)
    with pytest.raises(ValueError, match="Expected 2D array"):
        NMF(2).fit(X[:, 0])


def test_nmf_spec_table():
    from sklearn.decomposition import NMF as SkNMF

    assert api._nmf_spec(NMF()) == dict(n_init=1, max_iter=200, tol=1e-4)
    assert api._nmf_spec(NMF(n_init=np.int64(3), tol=0, max_iter=7)) == dict(n_init=3, max_iter=7, tol=0.0)
    for est in (SubNMF(), NMF(max_iter=0), NMF(n_init=True), NMF(n_init=0), NMF(tol=-1.0), NMF(tol=float('inf')),
                NMF(tol=float('nan')), NMF(tol='x'), NMF(max_iter=2.0), SkNMF(2, init='random', solver='mu'),
                object()):
        assert api._nmf_spec(est) is None, est


def test_entry_points_declared_and_exported():
    with open(os.path.join(os.path.dirname(HERE), "include", "ccmi.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"^(int|size_t) " + name + r"\(", header, re.M), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def test_workspace_bytes_and_plan():
    lib = _lib.load()

    def ws(m, md, B, Ks):
        a = np.asarray(Ks, dtype=np.int32)
        return int(lib.cc_nmf_workspace_bytes(m, md, B, a.ctypes.data, len(a)))

    for m, md, Ks in ((76, 5, [1, 2, 3, 7, 16, 17]), (240, 120, [2, 3, 5]), (130, 3, [127]), (8000, 64, range(2, 16))):
        Ks = list(Ks)
        per = engine.nmf_bytes(m, md, Ks)
        for B in (1, 3, 64):
            got = ws(m, md, B, Ks)
            # the rows [m, md] and the indices are the engine's own; the rest is the workspace
            assert 0 < got <= 512 + B * (per - 8 * m * md), (m, md, B)
            assert got > B * 8 * m * sum((K + 15) // 16 * 16 for K in Ks)
    assert ws(76, 5, 1, [77]) > 0 and ws(3, 2, 1, [127]) > 0  # K may exceed m and md
    assert ws(76, 5, 1, [128]) == 0 and ws(76, 5, 1, [0]) == 0 and ws(0, 5, 1, [2]) == 0
    assert ws(76, 0, 1, [2]) == 0 and ws(76, 5, 0, [2]) == 0 and ws(200, 5, 600, list(range(1, 128))) == 0
    assert ws(76, 5, 1, [2] * 128) == 0

    n, m, md, Ks = 96, 76, 5, [2, 3, 17]
    per = engine.nmf_bytes(m, md, Ks)
    fixed = 1024 + 8 * (m + md) * sum(Ks)
    assert engine.nmf_plan(n, m, 7, Ks, md, fixed + per) == 1
    assert engine.nmf_plan(n, m, 7, Ks, md, fixed + 3 * per + per - 1) == 3
    assert engine.nmf_plan(n, m, 7, Ks, md, 1 << 40) == 7
    assert engine.nmf_plan(n, m, 7, Ks, md, 3 * fixed + per, n_init=3) == 1
    assert engine.nmf_plan(n, m, 60000, [2] * 100, md, 1 << 50) == 655
    with pytest.raises(ValueError, match=r"workspace_budget = \d+ bytes cannot hold the NMF clusterer: one resample of "
                                         r"m = 76 over 5 features \(\d+ bytes\) is needed"):
        engine.nmf_plan(n, m, 7, Ks, md, fixed + per - 1)
