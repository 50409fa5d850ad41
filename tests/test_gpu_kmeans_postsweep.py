"""The post-sweep phase of the d <= 128 k-means engine (the change-list apply, the f64 running
sums, the centre update) against the engine's own output at the commit named in
tests/golden/engine/postsweep_parent.npz, before the phase's element-wise passes were
restructured.  A restructuring of this phase may change which thread does what, never the
arithmetic per element nor the order of the f32 additions per (cluster, dim), so everything is
compared exactly: labels (sha256), inertia bits and n_iter.

The fixture lives under tests/golden/engine/ (not tests/golden/): every .npz directly under
tests/golden/ is taken for a consensus fixture by tests/conftest.py.  It is written by
tests/golden/make_postsweep.py, on the GPU, with the library of that commit.

d = 128 cases (the only sparse instantiation): blobs with k_true = 8 (cluster_std 12: the blobs
touch, so that every K, K = 8 too, runs Lloyd iterations past the first two dense ones; with
well separated blobs K = 8 converges in two and never enters the sparse path), 80 % resamples,
H = 2, n_init 3; n = 2503 (m = 2002, no multiple of 16, 64 or 1024) and n = 4000; K in 2, 7, 8, 9, 20,
24, 25, 40: fewer clusters than waves, one, two and three clusters per wave, and more than 24 (the
sizes at which an apply that splits a list by cluster over the eight waves changes path).  Every
K runs alone (so that "sparse item-sweeps ran" is known per
K) and all together in one unit (many items per sweep); the two must agree, since nothing
depends on the packing.  The same with CCMI_KM_LSEG=16, a change-list capacity of 16 entries per
segment, so that lists overflow and the sums are rebuilt from every label.
"""
import hashlib
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN, digest
from tests.test_gpu_kmeans import blobs, run_gpu

pytestmark = pytest.mark.gpu

POSTSWEEP_GOLDEN = "engine/postsweep_parent.npz"  # under tests/golden/
KS_SPARSE = [2, 7, 8, 9, 20, 24, 25, 40]
NS_SPARSE = [2503, 4000]
LSEGS = [0, 16]  # 0: the default capacity
NARROW = [(64, 3000), (32, 3000)]  # (d, n): the centre-update passes shared with d = 128
KS_NARROW = list(range(2, 11))
K_TRUE, FRAC, H, SEED = 8, 0.8, 2, 5
STD = {128: 12.0, 64: 3.0, 32: 3.0}  # cluster_std of the blobs by d


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _pack(labs, inert, nit, stats):
    """What the fixture stores of one run: per K the labels' digest, the inertia bits, n_iter."""
    return dict(labels_sha256=np.array([_sha(labs[k].astype(np.uint8)) for k in range(labs.shape[0])]),
                inertia_bits=np.ascontiguousarray(inert).view(np.uint32).copy(),
                n_iter=nit.astype(np.int32), sparse_item_sweeps=np.int64(stats[6]))


_data = {}


def case_data(n, d):
    if (n, d) not in _data:
        _data[n, d] = blobs(n, d, K_TRUE, seed=n + d, std=STD[d])
    return _data[n, d]


def sparse_runs(n, lseg, env=os.environ):
    """The d = 128 runs of one (n, capacity): {"all": every K in one unit, K: that K alone}, each
    with the labels kept beside what the fixture stores."""
    X = case_data(n, 128)
    old = env.get("CCMI_KM_LSEG")
    if lseg:
        env["CCMI_KM_LSEG"] = str(lseg)
    else:
        env.pop("CCMI_KM_LSEG", None)
    try:
        out = {}
        for key, Ks in [("all", KS_SPARSE)] + [(K, [K]) for K in KS_SPARSE]:
            _, labs, inert, nit, stats = run_gpu(X, Ks, H, FRAC, SEED)
            out[key] = (_pack(labs, inert, nit, stats), labs)
    finally:
        if old is None:
            env.pop("CCMI_KM_LSEG", None)
        else:
            env["CCMI_KM_LSEG"] = old
    return out


def narrow_run(d, n):
    _, labs, inert, nit, stats = run_gpu(case_data(n, d), KS_NARROW, H, FRAC, SEED)
    return _pack(labs, inert, nit, stats)


def fixture_key(n, d, lseg, run):
    return f"d{d}_n{n}_l{lseg}_{run}_"


_default_runs = {}


def default_runs(n):
    """The runs at the default capacity, computed once (two tests read them)."""
    if n not in _default_runs:
        _default_runs[n] = sparse_runs(n, 0)
    return _default_runs[n]


def _check(z, key, got):
    for name in ("labels_sha256", "inertia_bits", "n_iter"):
        np.testing.assert_array_equal(got[name], z[key + name], err_msg=key + name)


@pytest.mark.parametrize("n", NS_SPARSE)
@pytest.mark.parametrize("lseg", LSEGS)
def test_sparse_apply_is_pinned(n, lseg):
    z = np.load(os.path.join(GOLDEN, POSTSWEEP_GOLDEN), allow_pickle=False)
    assert digest(case_data(n, 128)) == str(z[f"d128_n{n}_x_sha256"])
    runs = default_runs(n) if lseg == 0 else sparse_runs(n, lseg)
    for run, (got, _) in runs.items():
        print(f"n={n} lseg={lseg} run={run}: sparse item-sweeps {int(got['sparse_item_sweeps'])}, "
              f"n_iter {got['n_iter'].tolist()}")
        assert got["sparse_item_sweeps"] > 0, (n, lseg, run)  # the change-list path ran
        _check(z, fixture_key(n, 128, lseg, run), got)
    # nothing depends on how the problems were packed into sweeps
    for k, K in enumerate(KS_SPARSE):
        for name in ("labels_sha256", "inertia_bits", "n_iter"):
            np.testing.assert_array_equal(runs["all"][0][name][k], runs[K][0][name][0], err_msg=f"K={K} {name}")
    if lseg:
        # a rebuild recomputes the sums the lists would have reached, up to rounding: where
        # k-means is well posed (K <= the number of blobs) the capacity changes no label
        ref = default_runs(n)
        for k, K in enumerate(KS_SPARSE):
            if K <= K_TRUE:
                np.testing.assert_array_equal(runs["all"][1][k], ref["all"][1][k], err_msg=f"K={K}")
                np.testing.assert_array_equal(runs[K][1][0], ref[K][1][0], err_msg=f"K={K} alone")


@pytest.mark.parametrize("d,n", NARROW)
def test_narrow_centre_update_is_pinned(d, n):
    z = np.load(os.path.join(GOLDEN, POSTSWEEP_GOLDEN), allow_pickle=False)
    assert digest(case_data(n, d)) == str(z[f"d{d}_n{n}_x_sha256"])
    _check(z, fixture_key(n, d, 0, "all"), narrow_run(d, n))
