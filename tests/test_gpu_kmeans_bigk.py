"""k-means above K = 20 on all three engines against sklearn, label for label.

The paths that only run there (DESIGN.md "K thresholds"): the multi-pass argmin of the narrow
engine's E-step (K >= 25, two passes and a partly filled last pass from K = 33), the trial
classes 2 + floor(ln K) = 5 (K = 21..54) and 6 (K >= 55) of the seeding, the 128-slot Lloyd
items of K = 125..127 that can never share a 256-slot sweep, units and wide calls of more than
21 K values, the wide engine's call splitting by centroid capacity, and the float64 engine's
eighth 16-centre tile.  BIGK has one K on each side of every threshold.

The rows are 128 tight blobs (std 0.3 in a (-10, 10) box), where sklearn's own fit shows no
rounding sensitivity at any of these K (tests/golden/make_sk_fixtures.py: its float64 fit, eight
2^-22 nudges, threads, alignments, the engine's operand precision and the near-tie count all leave
resample 0's labels alone; tests/test_sk_parity_host.py asserts reasons == 0 for every problem of
these fixtures, with one exception).  So every (K, h) must be IDENTICAL to sklearn's labels,
nothing left out.  The data seed of each case is n + d + 1000 j with the first j for which that
holds (DATA_SEED).  The exception is K = 2..30 on wide rows: no j in 0..59 is free of near ties
there, so j = 0 stays, whose K = 16 and K = 24 pass one near tie each on resample 0; identity is
demanded of them all the same.

The f16 engines' n_iter must equal sklearn's and their inertia must lie within the rounding bound
of check_sklearn of the float64 sum of squares about sklearn's centres (fixtures fit_<case>.npz);
the largest error in units of sigma is printed per case."""
import numpy as np
import pytest
import torch

from consensus_clustering_amd import engine, kmeans
from consensus_clustering_amd.kmeans import BatchedKMeans
from tests.conftest import digest
from tests.sk_parity import load_sk_fixture, partition_ss, sklearn_identical, sklearn_parity
from tests.test_gpu_kmeans import blobs, run_gpu

pytestmark = pytest.mark.gpu

BIGK = [21, 24, 25, 32, 33, 54, 55, 64, 65, 96, 97, 125, 127]
RANGE = list(range(2, 31))   # 29 K values x 3 inits = 87 problems: more than one unit / wide call
SEED, FRAC = 7, 0.8
# case -> make_blobs random_state (make_sk_fixtures.py CASES holds the same numbers)
DATA_SEED = {
    "bigk_n1536_d16": 4552,
    "bigk_n1536_d40": 1576,
    "bigk_n1536_d100": 5636,
    "range_n1536_d16": 29552,
    "bigk_n1024_d300": 4324,
    "bigk5_n1024_d300": 4324,
    "range_n1024_d300": 1324,
}

_X, _RUN = {}, {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for name in ("CCMI_NSUB", "CCMI_SEEDMAX", "CCMI_KM_SHARE_SEED", "CCMI_KM_DENSE", "CCMI_WIDE_RELOC_FULL"):
        monkeypatch.delenv(name, raising=False)


def rows(case):
    if case not in _X:
        n, d = (int(t[1:]) for t in case.split("_")[1:])
        _X[case] = blobs(n, d, 128, seed=DATA_SEED[case], std=0.3)
    return _X[case]


def fit(case, Ks, H, tag="default"):
    """run_gpu on the case's rows, once per (case, Ks, tag): several tests read the same run."""
    key = (case, tuple(Ks), H, tag)
    if key not in _RUN:
        _RUN[key] = run_gpu(rows(case), Ks, H, FRAC, SEED)
    return _RUN[key]


def check_sklearn(case, run, Ks, H):
    """Every (K, h) identical to sklearn's float32 labels; resample 0 also through the full
    classification (which reads the fixture's variants and must find none needed).  n_iter equals
    sklearn's for every (K, h) on which sklearn's own float32 and float64 fits agree about it, and
    the inertia lies within 8 sigma + 2^-19 relative of the float64 sum of squares about sklearn's
    float32 centres (tests/golden/sk/fit_<case>.npz, make_sk_fit_fixtures.py: sigma is one float32
    rounding per row at the magnitude of the cancelling terms, in quadrature)."""
    X = rows(case)
    idx, labs, inert, nit, stats = run
    assert sklearn_identical(case, X, labs, idx) == len(Ks) * H
    same, _, total = sklearn_parity(case, X, labs, idx, max_unexplained=0, Ks=Ks)
    assert same == total == len(Ks)
    assert np.all(nit >= 1) and np.all(nit <= 300)
    assert np.all(np.isfinite(inert)) and np.all(inert > 0)
    assert stats[0] > 0 and stats[2] > 0
    rel = 0.0
    for k, K in enumerate(Ks):
        assert labs[k].min() == 0 and labs[k].max() == K - 1
        for h in range(H):
            ss = partition_ss(X[idx[h]], labs[k, h], K)
            rel = max(rel, abs(float(inert[k, h]) - ss) / ss)
    f = load_sk_fixture("fit_" + case)
    meta = f["meta"]
    assert (meta["Ks"], meta["H"], meta["seed"], meta["frac"]) == (list(Ks), H, SEED, FRAC)
    assert meta["x_sha256"] == digest(X)
    err = np.abs(inert.astype(np.float64) - f["inertia64"]) / f["inertia64"]
    bound = 8.0 * f["sigma"] + 2.0 ** -19
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"f16 inertia [{case}, {len(Ks)} K x {H}]: max |inertia - SS64(own labels)| / SS64 = {rel:.3e}; against "
          f"sklearn's centres max |err| / sigma = {(err / f['sigma']).max():.2f}, max |err| / inertia64 = {err.max():.3e}, "
          f"max |err| / bound = {(err / bound).max():.3f} at K = {Ks[worst[0]]}, h = {worst[1]}; n_iter "
          f"{int(nit.min())}..{int(nit.max())}, {int((nit != f['n_iter']).sum())} differ from sklearn's, "
          f"{int(f['exempt'].sum())} exempt")
    differ = [(Ks[k], h, int(nit[k, h]), int(f["n_iter"][k, h])) for k, h in np.argwhere((nit != f["n_iter"]) & ~f["exempt"])]
    assert not differ, f"n_iter (K, h, engine, sklearn): {differ}"
    over = [(Ks[k], h, float(err[k, h]), float(bound[k, h])) for k, h in np.argwhere(err > bound)]
    assert not over, f"inertia (K, h, relative error, bound): {over}"


def triple(run, k=None):
    """(labels, inertia bits, n_iter) of a run, or of its k-th K only."""
    labs, inert, nit = run[1:4]
    out = (labs, inert.view(np.uint32), nit)
    return out if k is None else tuple(v[k:k + 1] for v in out)


def same_bits(a, b, what):
    for x, y, name in zip(a, b, ("labels", "inertia", "n_iter")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}")


# ---- narrow engine (kmeans.hip): d = 16, 40, 100 run the kernels padded to 32, 64, 128 ----

@pytest.mark.parametrize("d", [16, 40, 100])
def test_narrow_bigk_identical_to_sklearn(d):
    case = f"bigk_n1536_d{d}"
    run = fit(case, BIGK, 3)
    check_sklearn(case, run, BIGK, 3)
    if d == 100:
        assert run[4][6] > 0  # the sparse M-step ran at these K


def test_narrow_bigk_dense_mstep_identical_to_sklearn(monkeypatch):
    """d = 100 with the sparse M-step switched off (CCMI_KM_DENSE=1): the same checks, so that
    neither form of the M-step hides behind the other.  (The sparse form once left the counts of
    clusters 64 and up of a change-list sweep uncleared: K = 65, h = 0 converged on a centre
    scaled by a stale count, with sklearn's labels and n_iter and an inertia 6.2e-3 too high.)"""
    case = "bigk_n1536_d100"
    monkeypatch.setenv("CCMI_KM_DENSE", "1")
    run = fit(case, BIGK, 3, tag="dense")
    assert run[4][6] == 0
    check_sklearn(case, run, BIGK, 3)


def test_narrow_unit_split_changes_nothing(monkeypatch):
    """CCMI_NSUB=1: all 39 problems in one unit, ~2500 slots against the sweep's 256, so the
    round-robin over problems (first_skip) carries the whole run; CCMI_NSUB=13: one K per unit;
    and the default split.  Labels, inertia bits and n_iter are the same in all three."""
    case = "bigk_n1536_d16"
    assert [len(kmeans.plan(BIGK, 3, s)) for s in (1, 13)] == [1, 13]
    default = fit(case, BIGK, 3)
    for nsub in ("1", "13"):
        monkeypatch.setenv("CCMI_NSUB", nsub)
        same_bits(triple(default), triple(fit(case, BIGK, 3, tag="nsub" + nsub)), f"CCMI_NSUB={nsub}")


@pytest.mark.parametrize("d", [16, 40, 100])
def test_narrow_k127_alone(d):
    """K = 127 on its own: three 128-slot items, one per sweep (at d <= 64 a 128-slot sweep is
    exactly the width at which pair mode switches on).  Bit-identical to its rows in the long
    list's run."""
    case = f"bigk_n1536_d{d}"
    full = fit(case, BIGK, 3)
    one = fit(case, [127], 3)
    same_bits(triple(full, BIGK.index(127)), triple(one), f"d={d} K=127 alone")


@pytest.mark.parametrize("nsub", ["1", None])
def test_narrow_more_than_21_k_values(monkeypatch, nsub):
    """K = 2..30 at d = 16 (a fixture of its own, range_n1536_d16): 87 problems, which
    cc_kmeans_plan cannot put in fewer than 2 units; with CCMI_NSUB=1 the first unit is full (64
    problems)."""
    case = "range_n1536_d16"
    g = kmeans.plan(RANGE, 3, 1)
    assert len(g) >= 2 and g[:, 0].max() <= 64 and g[:, 0].sum() == 87
    if nsub:
        monkeypatch.setenv("CCMI_NSUB", nsub)
    check_sklearn(case, fit(case, RANGE, 3, tag=f"nsub{nsub}"), RANGE, 3)


# ---- wide engine (kmeans_wide.hip): d = 300, dpad 320, m = 819 ----

def wide_calls(Ks, n_init=3, m=819, dpad=320):
    """The K values of each cc_kmeans_wide call for Ks (cc_kmeans_wide_chunk, which
    BatchedKMeans._run_wide and cc_kmeans_fit both follow)."""
    from consensus_clustering_amd import _lib

    a = np.ascontiguousarray(np.asarray(Ks, dtype=np.int32))
    out, k0 = [], 0
    while k0 < len(Ks):
        nk = _lib.load().cc_kmeans_wide_chunk(m, dpad, a[k0:].ctypes.data, len(Ks) - k0, n_init)
        _lib.check(min(nk, 0), "cc_kmeans_wide_chunk")
        out.append(list(Ks[k0:k0 + nk]))
        k0 += nk
    return out


def test_wide_short_list_identical_to_sklearn():
    """Five K values across the trial classes and argmin forms, few enough for one call."""
    Ks = [21, 25, 33, 55, 127]
    check_sklearn("bigk5_n1024_d300", fit("bigk5_n1024_d300", Ks, 2), Ks, 2)


def test_wide_bigk_identical_to_sklearn():
    """All of BIGK: about 2800 centroid slots, more than one call holds (8 column tiles of 256),
    so the host splits the list by capacity."""
    case = "bigk_n1024_d300"
    check_sklearn(case, fit(case, BIGK, 2), BIGK, 2)
    calls = wide_calls(BIGK)
    assert len(calls) >= 2 and [K for c in calls for K in c] == BIGK


def test_wide_more_than_21_k_values():
    """K = 2..30 on wide rows: 21 K values (64 // n_init) in the first call and 8 in the second,
    whose labels, inertia, n_iter and k-means++ tables are offset by k0.  Identical to sklearn, and
    bit-identical to each K run in a call of its own."""
    case = "range_n1024_d300"
    run = fit(case, RANGE, 2)
    check_sklearn(case, run, RANGE, 2)
    assert wide_calls(RANGE) == [RANGE[:21], RANGE[21:]]
    for k, K in enumerate(RANGE):
        one = fit(case, [K], 2)
        same_bits(triple(run, k), triple(one), f"K={K} alone")


def test_wide_single_k_beyond_capacity_names_k_and_n_init():
    """K = 127 with n_init = 16 (2048 slots) fits no call alone: an error that names K and n_init,
    raised before anything is launched."""
    from consensus_clustering_amd import _lib

    with pytest.raises(_lib.CCMIError, match=r"K = 127 with n_init = 16"):
        run_gpu(rows("bigk_n1024_d300"), [127, 21], 1, FRAC, SEED, n_init=16)


# ---- float64 engine (kmeans_f64.hip) ----

def f64_rows(n, d):
    X = blobs(n, d, 128, seed=n + d).astype(np.float64)
    X += np.random.default_rng(0).normal(scale=0.5, size=X.shape)
    return X


@pytest.mark.parametrize("d", [24, 150])
def test_f64_bigk_identical_to_sklearn_float64(d):
    """n = 400 (m = 320), 128 blobs plus noise as in test_f64_labels_match_sklearn_float64, K up to
    127 (7 full 16-centre tiles and one of 15; at d = 150 K d is far past what sits in LDS): label
    digest and n_iter identical for every (K, h), inertia within 1e-12 relative (that test's own
    bound).  sklearn's side was generated under the engine's lowest-index order among tied
    farthest rows (fixture meta); its relocation count is printed."""
    from tests.conftest import digest

    case, n, Ks, H, seed = f"f64_n400_d{d}", 400, [21, 33, 55, 100, 127], 2, 3
    f = load_sk_fixture(case)
    meta = f["meta"]
    assert (meta["n"], meta["d"], meta["Ks"], meta["H"], meta["seed"]) == (n, d, Ks, H, seed)
    X = f64_rows(n, d)
    assert digest(X) == meta["x_sha256"]
    dev = engine.require_gpu()
    m = int(0.8 * n)
    idx = engine.resample_indices(seed, n, m, 0, H)
    L = engine.new_label_matrix(len(Ks), n, engine.pad_h(H), dev)
    inert = torch.zeros((len(Ks), H), dtype=torch.float64, device=dev)
    nit = torch.zeros((len(Ks), H), dtype=torch.int32, device=dev)
    BatchedKMeans(Ks, n_init=3, random_state=seed).run_f64(
        torch.from_numpy(X).to(dev), torch.from_numpy(idx).to(dev), n, H, m, 0, H, L, inertia=inert, n_iter=nit)
    torch.cuda.synchronize()
    Lh, nit, inert = L.cpu().numpy(), nit.cpu().numpy(), inert.cpu().numpy()
    bad, rel = [], 0.0
    for k, K in enumerate(Ks):
        for h in range(H):
            got = Lh[k][idx[h], h].astype(np.int8)
            if digest(got) != f["digest64"][k, h] or nit[k, h] != f["n_iter"][k, h]:
                bad.append((K, h, int(nit[k, h]), int(f["n_iter"][k, h])))
            rel = max(rel, abs(inert[k, h] - f["inertia"][k, h]) / f["inertia"][k, h])
    print(f"f64 [{case}]: {len(Ks) * H - len(bad)}/{len(Ks) * H} identical to sklearn float64 (labels, n_iter); "
          f"max relative inertia difference {rel:.2e}; differing {bad}; sklearn relocated "
          f"{meta['relocated_rows']} rows (numpy's tie order differs in "
          f"{meta['problems_where_numpy_order_differs']} problems)")
    assert not bad, bad
    assert rel <= 1e-12, rel
