"""Pairwise agreement of label columns on the GPU (cc_agreement_sums, engine.agreement_sums,
ConsensusClustering.agreement_sums / resample_agreement / partition_agreement / stability): the
four exact int64 sums of every pair against the numpy reference (tests/agreement_ref.py), across
channel widths, tile ranges, strides, streams and two ranks, and the indices against sklearn's
adjusted_rand_score on the fitted labels."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from sklearn.metrics import adjusted_rand_score

from consensus_clustering_amd import ConsensusClustering, _lib, engine, post
from tests.agreement_ref import group_sums
from tests.conftest import ROOT, load_fixture

pytestmark = pytest.mark.gpu

ABSENT = 0xFF


def _random_case(n, H, frac, K, seed, p0=None):
    """Resample indices [H, m] and labels [H, m]: a noisy copy of one truth partition per resample
    (p0: instead, label 0 with probability p0, else uniform)."""
    rng = np.random.default_rng(seed)
    m = max(int(frac * n), 1)
    idx = np.stack([rng.permutation(n)[:m] for _ in range(H)]).astype(np.int32)
    truth = rng.integers(0, K, size=n)
    lab = np.empty((H, m), dtype=np.int32)
    for h in range(H):
        if p0 is None:
            lab[h] = (truth[idx[h]] + (rng.random(m) < 0.25) * rng.integers(0, K, size=m)) % K
        else:
            lab[h] = np.where(rng.random(m) < p0, 0, rng.integers(0, K, size=m))
    return idx, lab


def _host_matrix(idx, lab, n):
    """uint8 [n, H], 0xFF = not sampled: what scatter_labels builds on the device."""
    A = np.full((n, idx.shape[0]), ABSENT, dtype=np.uint8)
    for h in range(idx.shape[0]):
        A[idx[h], h] = lab[h]
    return A


def _device_labels(idx, lab, n, dev):
    Hpad = engine.pad_h(idx.shape[0])
    L = engine.new_label_matrix(1, n, Hpad, dev)
    engine.scatter_labels(torch.from_numpy(np.array(idx, dtype=np.int32)).to(dev),
                          torch.from_numpy(np.array(lab, dtype=np.int32)).to(dev), n, L[0])
    return L[0]


@functools.lru_cache(maxsize=None)
def _case(n, H, frac, K, p0=None):
    """One random case and its reference sums, computed once and shared (read only)."""
    idx, lab = _random_case(n, H, frac, K, seed=1000 * K + n + H, p0=p0)
    A = _host_matrix(idx, lab, n)
    S = group_sums(A, K)
    for a in (idx, lab, A, S):
        a.setflags(write=False)
    return idx, lab, A, S


def _kp(K):
    """The smallest power of two that holds K cluster channels and the membership channel (the
    library pads to at least 4, which only adds virtual columns)."""
    kp = 2
    while kp < K + 1:
        kp *= 2
    return kp


CASES = [
    (300, 37, 0.6, 3),    # one tile; n no multiple of 32 or 16
    (257, 70, 0.6, 3),    # 280 virtual columns: a diagonal tile, an off-diagonal tile and the mirror
    (513, 40, 0.9, 8),    # KP = 16, 640 columns: 6 tiles
    (257, 5, 0.6, 127),   # KP = 128: two resamples per block
    (129, 37, 1.0, 2),    # nothing absent
    (260, 5, 0.3, 4),     # items never sampled
    (1, 5, 1.0, 2), (2, 5, 1.0, 2), (15, 5, 1.0, 2), (33, 5, 1.0, 2),  # short and ragged item chunks
] + [
    # the membership channel is the last of its group at K = KP - 1; empty channels follow it at
    # K = KP / 2; H so that H * KP > 256 (more than one tile side)
    (257, 256 // _kp(K) + 3, 0.6, K) for K in (1, 7, 15, 16, 31, 32, 63, 64)
]


@pytest.mark.parametrize("n,H,frac,K", CASES)
def test_sums_equal_the_reference(n, H, frac, K):
    dev = engine.require_gpu()
    idx, lab, A, S_ref = _case(n, H, frac, K)
    if (n, H) == (260, 5):
        assert len(np.setdiff1d(np.arange(n), idx.ravel())) > 0
        s0 = S_ref[..., 0][np.triu_indices(H, 1)]
        assert s0.min() < s0.max(), "some pair of resamples shares fewer items than the others"
    if frac == 1.0:
        assert not (A == ABSENT).any()
    L = _device_labels(idx, lab, n, dev)
    S = engine.agreement_sums(L, H, K, n)
    assert S.dtype == torch.int64 and tuple(S.shape) == (H, H, 4) and S.device.type == "cuda"
    np.testing.assert_array_equal(S.cpu().numpy(), S_ref)


def test_squares_beyond_31_bits():
    """n = 70 000 with 90 % of the labels 0: an entry of N exceeds 46 341, so its square does not
    fit 31 bits (the squares are taken in 64 bits)."""
    dev = engine.require_gpu()
    n, H, K = 70_000, 3, 2
    idx, lab, A, S_ref = _case(n, H, 1.0, K, p0=0.9)
    n00 = int(((A[:, 0] == 0) & (A[:, 1] == 0)).sum())
    assert n00 > 46_341 and n00 * n00 >= 2**31
    L = _device_labels(idx, lab, n, dev)
    np.testing.assert_array_equal(engine.agreement_sums(L, H, K, n).cpu().numpy(), S_ref)


def test_a_partition_column_of_another_k():
    """B = one column [n] (ldB = 1) of Kc = 3 != K = 5 with ids outside [0, Kc): those items are
    absent from that column."""
    dev = engine.require_gpu()
    n, H, K, Kc = 300, 37, 5, 3
    idx, lab, A, _ = _case(n, H, 0.6, K)
    rng = np.random.default_rng(4)
    col = rng.integers(0, Kc, size=n).astype(np.uint8)
    col[::7] = 7
    col[1::11] = 200
    col[3] = ABSENT
    S_ref = group_sums(A, K, col[:, None], Kc)
    assert (S_ref[..., 0] < (A != ABSENT).sum(axis=0)[:, None]).all(), "the ids outside [0, Kc) count nowhere"
    L = _device_labels(idx, lab, n, dev)
    S = engine.agreement_sums(L, H, K, n, torch.from_numpy(col).to(dev), 1, Kc)
    assert tuple(S.shape) == (H, 1, 4)
    np.testing.assert_array_equal(S.cpu().numpy(), S_ref)
    # the same pair the other way round: r2 and c2 exchanged
    T = engine.agreement_sums(torch.from_numpy(col).to(dev), 1, Kc, n, L, H, K)
    np.testing.assert_array_equal(T.cpu().numpy()[0], S_ref[:, 0][:, [0, 1, 3, 2]])


def test_two_label_matrices_of_different_k():
    dev = engine.require_gpu()
    n = 300
    idxA, labA, A, _ = _case(n, 37, 0.6, 3)
    idxB, labB, B, _ = _case(n, 70, 0.6, 9)   # KP = 16 for both sides: 2 x 5 tiles
    S_ref = group_sums(A, 3, B, 9)
    LA, LB = _device_labels(idxA, labA, n, dev), _device_labels(idxB, labB, n, dev)
    assert engine.agreement_num_tiles(37, 3, 70, 9) == 3 * 5
    S = engine.agreement_sums(LA, 37, 3, n, LB, 70, 9)
    np.testing.assert_array_equal(S.cpu().numpy(), S_ref)


def test_tile_ranges():
    dev = engine.require_gpu()
    n, H, frac, K = 513, 40, 0.9, 8
    idx, lab, A, S_ref = _case(n, H, frac, K)
    L = _device_labels(idx, lab, n, dev)
    nt = engine.agreement_num_tiles(H, K)
    assert nt == 6
    S = torch.zeros((H, H, 4), dtype=torch.int64, device=dev)
    engine.agreement_sums(L, H, K, n, tile_begin=3, tile_end=3, out=S)
    assert not bool(S.any()), "an empty range writes nothing"
    filled = []
    for tb, te in [(0, 1), (1, 4), (4, nt)]:
        part = engine.agreement_sums(L, H, K, n, tile_begin=tb, tile_end=te)
        filled.append(part.cpu().numpy().any(axis=2))
        out = engine.agreement_sums(L, H, K, n, tile_begin=tb, tile_end=te, out=S)
        assert out is S
    assert (sum(f.astype(int) for f in filled) == 1).all(), "disjoint ranges fill disjoint pairs"
    np.testing.assert_array_equal(S.cpu().numpy(), S_ref)


def test_strided_labels_side_stream_and_reproducibility():
    dev = engine.require_gpu()
    n, H, frac, K = 300, 37, 0.6, 3
    idx, lab, A, S_ref = _case(n, H, frac, K)
    L = _device_labels(idx, lab, n, dev)
    Hpad = L.shape[1]
    wide = torch.full((n, Hpad + 128), 0x01, dtype=torch.uint8, device=dev)  # junk past Hpad
    view = wide[:, :Hpad]
    view.copy_(L)
    assert view.stride(0) == Hpad + 128
    S = engine.agreement_sums(view, H, K, n)
    np.testing.assert_array_equal(S.cpu().numpy(), S_ref)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        S2 = engine.agreement_sums(L, H, K, n)
    side.synchronize()
    assert torch.equal(S, S2), "two runs are bitwise equal"
    np.testing.assert_array_equal(S2.cpu().numpy(), S_ref)


def test_abi_errors_launch_nothing():
    dev = engine.require_gpu()
    n, H, frac, K = 300, 37, 0.6, 3
    idx, lab, A, S_ref = _case(n, H, frac, K)
    L = _device_labels(idx, lab, n, dev)
    lib = _lib.load()
    nt = engine.agreement_num_tiles(H, K)
    nbytes = int(lib.cc_agreement_workspace_bytes(n, H, H))
    assert nbytes >= 2 * 128 * 384
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    S = torch.zeros((H, H, 4), dtype=torch.int64, device=dev)
    good = dict(A=L.data_ptr(), ldA=L.stride(0), HA=H, KA=K, B=None, ldB=0, HB=0, KB=0, n=n, tb=0, te=nt,
                S=S.data_ptr(), ws=ws.data_ptr(), nbytes=nbytes)

    def call(**kw):
        a = dict(good, **kw)
        _lib.call("cc_agreement_sums", a["A"], a["ldA"], a["HA"], a["KA"], a["B"], a["ldB"], a["HB"], a["KB"],
                  a["n"], a["tb"], a["te"], a["S"], a["ws"], a["nbytes"], engine.stream_ptr())

    two = dict(B=L.data_ptr(), ldB=L.stride(0), HB=H, KB=K, te=engine.agreement_num_tiles(H, K, H, K))
    for bad in (dict(A=None), dict(S=None), dict(ws=None), dict(KA=0), dict(KA=128), dict(HA=0), dict(n=0),
                dict(S=S.data_ptr() + 4), dict(te=nt + 1), dict(tb=-1), dict(tb=2, te=1), dict(nbytes=nbytes // 4),
                dict(two, KB=0), dict(two, KB=128), dict(two, HB=0), dict(two, te=two["te"] + 1),
                dict(two, nbytes=nbytes - 1)):
        with pytest.raises(_lib.CCMIError, match="cc_agreement_sums"):
            call(**bad)
    torch.cuda.synchronize()
    assert not bool(S.any()), "a rejected call must not launch"
    with pytest.raises(_lib.CCMIError):  # the engine reaches the same checks
        engine.agreement_sums(L, H, 0, n)
    with pytest.raises(_lib.CCMIError):
        engine.agreement_sums(L, H, K, n, tile_end=nt + 1)
    call(tb=nt, te=nt)  # an empty range is fine
    torch.cuda.synchronize()
    assert not bool(S.any())
    call(**two)       # and so is the accepted form of the two-group call
    torch.cuda.synchronize()
    np.testing.assert_array_equal(S.cpu().numpy(), S_ref)


# ---------------------------------------------------------------- the public API

FIXTURE = "blobs_n400_d8_k4"


@pytest.fixture(scope="module")
def fitted():
    f = load_fixture(FIXTURE)
    meta = f["meta"]
    cc = ConsensusClustering(K_range=[int(k) for k in f["K_range"]], n_iterations=meta["H"],
                             subsampling=meta["subsampling"], random_state=meta["random_state"],
                             plot_cdf=False, keep_matrices=False)
    return cc.fit(f["X"])


def _resample_labels(cc, K):
    """{h: (sorted item ids, their labels)} read back from labels_ and resampling_indices_."""
    k = list(cc.cdf_at_K_data).index(K)
    L = cc.labels_[k].cpu().numpy()
    out = {}
    for h, idx in enumerate(cc.resampling_indices_):
        items = np.sort(idx)
        lab = L[items, h]
        assert (lab < K).all()
        out[h] = (items, lab)
    assert (L[:, :len(out)] != ABSENT).sum() == sum(len(v[0]) for v in out.values())
    return out


def test_api_resample_agreement_is_sklearns_ari(fitted):
    cc = fitted
    H = int(cc.n_iterations)
    Ks = list(cc.cdf_at_K_data)
    for K in sorted({Ks[0], cc.best_k_, Ks[-1]}):
        R = cc.resample_agreement(K, 'ari')
        assert R.shape == (H, H) and R.dtype == np.float64
        np.testing.assert_array_equal(R, R.T)
        np.testing.assert_array_equal(np.diag(R), 1.0)
        cols = _resample_labels(cc, K)
        worst = 0.0
        for h1 in range(H):
            for h2 in range(h1 + 1, H):
                _, i1, i2 = np.intersect1d(cols[h1][0], cols[h2][0], assume_unique=True, return_indices=True)
                want = adjusted_rand_score(cols[h1][1][i1], cols[h2][1][i2])
                worst = max(worst, abs(R[h1, h2] - want))
        print(f"K={K}: largest |resample_agreement - adjusted_rand_score| = {worst:.3g}")
        assert worst <= 1e-12
        J = cc.resample_agreement(K, 'jaccard')
        ok = ~np.isnan(J)
        assert ok.all() and (J >= 0).all() and (J <= 1).all()
    np.testing.assert_array_equal(cc.resample_agreement(), cc.resample_agreement(cc.best_k_))


def test_api_partition_agreement(fitted):
    cc = fitted
    H, n = int(cc.n_iterations), cc._N
    for K in cc.cdf_at_K_data:
        consensus = cc.predict(K)
        cols = _resample_labels(cc, K)
        P = cc.partition_agreement(K)
        assert P.shape == (H,) and P.dtype == np.float64
        want = np.array([adjusted_rand_score(consensus[cols[h][0]], cols[h][1]) for h in range(H)])
        print(f"K={K}: largest |partition_agreement - adjusted_rand_score| = {np.abs(P - want).max():.3g}")
        assert np.abs(P - want).max() <= 1e-12
    K = list(cc.cdf_at_K_data)[1]
    given = (np.arange(n) * 7 % 5).astype(np.int16)
    S = cc.agreement_sums(K, given)
    assert S.shape == (H, 4) and S.dtype == np.int64
    k = list(cc.cdf_at_K_data).index(K)
    A = cc.labels_[k].cpu().numpy()[:, :H]
    np.testing.assert_array_equal(S, group_sums(A, K, given[:, None], 5)[:, 0])
    np.testing.assert_array_equal(cc.partition_agreement(K, given, 'jaccard'), post.agreement_from_sums(S, 'jaccard'))
    full = cc.agreement_sums(K)
    assert full.shape == (H, H, 4) and full.dtype == np.int64
    np.testing.assert_array_equal(full, group_sums(A, K))


def test_api_stability_and_untouched_results(fitted):
    cc = fitted
    before = {K: {name: (None if v is None else np.array(v, copy=True)) for name, v in res.items()}
              for K, res in cc.cdf_at_K_data.items()}
    best, pairs = cc.best_k_, {K: np.array(v, copy=True) for K, v in cc.pair_counts_.items()}
    st = cc.stability()
    assert list(st) == list(cc.cdf_at_K_data)
    iu = np.triu_indices(int(cc.n_iterations), 1)
    for K, v in st.items():
        assert v == cc.resample_agreement(K)[iu].mean()
    K = list(cc.cdf_at_K_data)[-1]
    assert list(cc.stability([K], 'jaccard')) == [K]
    assert cc.stability([K], 'jaccard')[K] == cc.resample_agreement(K, 'jaccard')[iu].mean()
    assert cc.best_k_ == best and list(cc.pair_counts_) == list(pairs)
    for K, v in pairs.items():
        np.testing.assert_array_equal(np.asarray(cc.pair_counts_[K]), v)
    for K, res in cc.cdf_at_K_data.items():
        assert list(res) == list(before[K])
        for name, v in res.items():
            if before[K][name] is None:
                assert v is None
            else:
                np.testing.assert_array_equal(np.asarray(v), before[K][name])


def test_api_errors(fitted):
    cc = fitted
    n = cc._N
    fresh = ConsensusClustering(K_range=[2, 3], plot_cdf=False, random_state=0)
    for method in (fresh.agreement_sums, fresh.resample_agreement, fresh.partition_agreement, fresh.stability):
        with pytest.raises(ValueError):
            method()
    for method in (cc.agreement_sums, cc.resample_agreement, cc.partition_agreement):
        with pytest.raises(KeyError):
            method(99)
    with pytest.raises(KeyError):
        cc.stability([99])
    K = list(cc.cdf_at_K_data)[0]
    for bad in (np.zeros(n - 1, dtype=np.int64), np.full(n, -1), np.full(n, 127), np.zeros(n, dtype=np.float64)):
        with pytest.raises(ValueError):
            cc.agreement_sums(K, bad)
        with pytest.raises(ValueError):
            cc.partition_agreement(K, bad)
    for method in (cc.resample_agreement, cc.stability):
        with pytest.raises(ValueError):
            method(index='rand')
    with pytest.raises(ValueError):
        cc.partition_agreement(K, index='rand')


def test_two_ranks_equal_one_rank(tmp_path, fitted):
    """Two gloo ranks on cuda:0 (tests/agreement_dist_worker.py): each rank fills the pairs of its
    share of the tiles in a zeroed buffer, the int64 SUM all-reduce merges them; equal to the
    one-rank sums exactly."""
    cc = fitted
    K = list(cc.cdf_at_K_data)[-1]
    out = str(tmp_path / "r0.npz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "agreement_dist_worker.py"), FIXTURE, "2",
                    str(K), out], check=True, timeout=300, env=env)
    from tests.agreement_dist_worker import given_labels

    got = np.load(out)
    np.testing.assert_array_equal(got["pairs"], cc.agreement_sums(K))
    np.testing.assert_array_equal(got["given"], cc.agreement_sums(K, given_labels(cc._N)))
