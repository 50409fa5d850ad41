"""Item and cluster consensus from the label matrix (cc_item_consensus, engine.item_consensus_sums,
ConsensusClustering.consensus_sums / item_consensus / cluster_consensus / icl): the exact int64
sums S[i, c] = sum_{j != i, cl[j] == c} C_ij * 2^40 against the CPU oracle's C, against the
materialised GPU route, across tile ranges, chunks, strides, streams and two ranks."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from consensus_clustering_amd import ConsensusClustering, _lib, engine, post
from oracle import cc_oracle as O
from tests.conftest import ROOT, load_fixture

pytestmark = pytest.mark.gpu

TWO40 = float(1 << 40)


def _device_labels(idx, labels_list, n, H, dev):
    Hpad = engine.pad_h(H)
    idx_d = torch.from_numpy(np.array(idx, dtype=np.int32)).to(dev)  # (copies: the shared cases are read-only)
    L = engine.new_label_matrix(len(labels_list), n, Hpad, dev)
    for j, lab in enumerate(labels_list):
        lab_d = torch.from_numpy(np.array(lab, dtype=np.int32)).to(dev)
        engine.scatter_labels(idx_d, lab_d, n, L[j])
    return L, Hpad


def _random_case(n, H, frac, Ks, seed):
    rng = np.random.default_rng(seed)
    m = int(frac * n)
    idx = np.stack([rng.permutation(n)[:m] for _ in range(H)]).astype(np.int32)
    truth = rng.integers(0, 7, size=n)
    labs = []
    for K in Ks:
        lab = np.empty((H, m), dtype=np.int32)
        for h in range(H):
            noisy = (truth[idx[h]] + (rng.random(m) < 0.15) * rng.integers(0, K, size=m)) % K
            lab[h] = noisy
        labs.append(lab)
    return idx, labs


def _random_clusters(n, Kc, rng):
    """Cluster ids in [0, Kc) with (where Kc allows) an id that has one member and an id that has
    none: id Kc - 1 stays empty (Kc >= 3), id Kc - 2 (Kc == 2: id 1) gets exactly one item."""
    if Kc == 1:
        return np.zeros(n, dtype=np.int32)
    single = 1 if Kc == 2 else Kc - 2
    cl = rng.integers(0, single, size=n).astype(np.int32)
    cl[rng.integers(0, n)] = single
    return cl


def _sums_from_C(C, cl, Kc):
    x = C.astype(np.float64) * TWO40
    Q = x.astype(np.int64)
    assert (Q.astype(np.float64) == x).all()
    np.fill_diagonal(Q, 0)
    onehot = np.zeros((len(cl), Kc), dtype=np.int64)
    ok = (cl >= 0) & (cl < Kc)
    onehot[np.flatnonzero(ok), cl[ok]] = 1
    return Q @ onehot


@functools.lru_cache(maxsize=None)
def _case(n, H, frac, K, Kc):
    """One random case and its oracle sums, computed once and shared (read only)."""
    idx, labs = _random_case(n, H, frac, [K], seed=n + H + K)
    rng = np.random.default_rng(1000 + n + Kc)
    cl = _random_clusters(n, Kc, rng)
    I = O.cosample_matrix(idx.astype(np.int64), n)
    M = O.coassoc_matrix(idx.astype(np.int64), labs[0].astype(np.int64), K, n)
    C = O.consensus_matrix(M.astype(np.uint16), I.astype(np.uint16))
    S = _sums_from_C(C, cl, Kc)
    for a in (idx, labs[0], cl, C, S):
        a.setflags(write=False)
    return idx, labs[0], cl, C, S


CASES = [
    (300, 37, 0.6, 3, 4),      # two row blocks, ragged
    (513, 300, 0.9, 8, 17),    # a one-row last block, counts > 255, two cluster passes
    (257, 131, 0.6, 127, 127),
    (700, 200, 0.8, 5, 1),
    (129, 37, 1.0, 2, 2),
    (260, 5, 0.3, 4, 3),       # pairs never co-sampled and items never sampled
    (1, 5, 1.0, 2, 2),
    (2, 5, 1.0, 2, 2),
    # the channel widths the cases above do not reach (KP = 16, 32, 64) and K = 1 (runs as KP = 2),
    # at the smallest n with a diagonal tile, an off-diagonal tile and a one-row ragged block
    (257, 37, 0.6, 9, 3),
    (257, 37, 0.6, 17, 3),
    (257, 37, 0.6, 33, 3),
    (257, 5, 1.0, 1, 2),
]


@pytest.mark.parametrize("n,H,frac,K,Kc", CASES)
def test_sums_equal_the_oracle(n, H, frac, K, Kc):
    dev = engine.require_gpu()
    idx, lab, cl, C, S_ref = _case(n, H, frac, K, Kc)
    if Kc >= 3:
        sizes = np.bincount(cl, minlength=Kc)
        assert sizes[Kc - 1] == 0 and sizes[Kc - 2] == 1
    if (n, H) == (260, 5):
        never = np.setdiff1d(np.arange(n), idx.ravel())
        assert len(never) > 0 and (C[np.triu_indices(n, 1)] == 0).any()
    L, Hpad = _device_labels(idx, [lab], n, H, dev)
    S = engine.item_consensus_sums(L[0], n, Hpad, K, cl, Kc)
    assert S.dtype == torch.int64 and tuple(S.shape) == (n, Kc) and S.device.type == "cuda"
    np.testing.assert_array_equal(S.cpu().numpy(), S_ref)


def test_masked_items_add_to_no_column_and_keep_their_row():
    dev = engine.require_gpu()
    n, H, frac, K, Kc = 513, 300, 0.9, 8, 17
    idx, lab, cl, C, S_full = _case(n, H, frac, K, Kc)
    masked = cl.copy()
    masked[::3] = -1
    masked[1] = Kc + 5  # any id outside [0, Kc) is "no cluster"
    S_ref = _sums_from_C(C, masked, Kc)
    assert (S_ref[::3] != 0).any(), "the masked items' own rows stay filled"
    L, Hpad = _device_labels(idx, [lab], n, H, dev)
    S = engine.item_consensus_sums(L[0], n, Hpad, K, masked, Kc).cpu().numpy()
    np.testing.assert_array_equal(S, S_ref)
    assert (S <= S_full).all() and (S != S_full).any()


def test_accumulation_sharding_and_chunks():
    dev = engine.require_gpu()
    n, H, frac, K, Kc = 700, 200, 0.8, 5, 1
    idx, lab, cl, C, S_ref = _case(n, H, frac, K, Kc)
    L, Hpad = _device_labels(idx, [lab], n, H, dev)
    nt = engine.num_tiles(n)
    assert nt == 6
    # three disjoint tile ranges into one S
    S = torch.zeros((n, Kc), dtype=torch.int64, device=dev)
    for tb, te in [(0, 1), (1, 4), (4, nt)]:
        out = engine.item_consensus_sums(L[0], n, Hpad, K, cl, Kc, tb, te, S=S)
        assert out is S
    np.testing.assert_array_equal(S.cpu().numpy(), S_ref)
    # an empty range adds nothing; a second call into a non-zero S adds
    engine.item_consensus_sums(L[0], n, Hpad, K, cl, Kc, 3, 3, S=S)
    np.testing.assert_array_equal(S.cpu().numpy(), S_ref)
    engine.item_consensus_sums(L[0], n, Hpad, K, cl, Kc, S=S)
    np.testing.assert_array_equal(S.cpu().numpy(), 2 * S_ref)


def test_tile_chunks_and_memory_bound():
    """tile_chunk = 4 at n = 1500 (21 tiles, 6 chunks) equals one chunk, and the call holds four
    co-sampling tiles, S and cl: nothing of n^2 = 2.25 MB."""
    dev = engine.require_gpu()
    n, H, K, Kc = 1500, 8, 4, 5
    idx, labs = _random_case(n, H, 0.8, [K], seed=77)
    cl = torch.from_numpy(_random_clusters(n, Kc, np.random.default_rng(7))).to(dev)
    L, Hpad = _device_labels(idx, labs, n, H, dev)
    assert engine.num_tiles(n) == 21
    whole = engine.item_consensus_sums(L[0], n, Hpad, K, cl, Kc).cpu().numpy()
    assert whole.any()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    S = engine.item_consensus_sums(L[0], n, Hpad, K, cl, Kc, tile_chunk=4)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes")
    assert rise < 4 * 131072 + 8 * n * Kc + 4 * n + 2**20
    np.testing.assert_array_equal(S.cpu().numpy(), whole)


def test_equals_the_materialised_gpu_route():
    """n = 2052 (45 tiles): the existing cosample(want_full) -> coassoc(M_full) -> consensus route,
    then (C * 2^40) summed by cluster with torch, and the symmetry of the block totals."""
    dev = engine.require_gpu()
    n, H, K, Kc = 2052, 64, 6, 6
    idx, labs = _random_case(n, H, 0.8, [K], seed=5)
    cl_h = np.random.default_rng(9).integers(0, Kc, size=n).astype(np.int32)
    cl = torch.from_numpy(cl_h).to(dev)
    L, Hpad = _device_labels(idx, labs, n, H, dev)
    nt = engine.num_tiles(n)
    I_tiles, I_full = engine.cosample(L[0], n, Hpad, 0, nt, want_full=True)
    M = torch.zeros((n, n), dtype=torch.int32, device=dev)
    counts = torch.zeros(20, dtype=torch.int64, device=dev)
    engine.coassoc(L[0], n, Hpad, K, 0, nt, I_tiles, engine.edges_device(dev), counts, M)
    C = engine.consensus(M, I_full)
    Q = (C.double() * TWO40).long()
    assert bool((Q.double() == C.double() * TWO40).all())
    Q.fill_diagonal_(0)
    S_ref = torch.zeros((n, Kc), dtype=torch.int64, device=dev).index_add_(1, cl.long(), Q)
    S = engine.item_consensus_sums(L[0], n, Hpad, K, cl, Kc)
    np.testing.assert_array_equal(S.cpu().numpy(), S_ref.cpu().numpy())
    onehot = np.eye(Kc, dtype=np.int64)[cl_h]
    B = onehot.T @ S.cpu().numpy()  # B[a, b] = sum_{i in a} S[i, b]
    np.testing.assert_array_equal(B, B.T)


def test_strided_labels_and_side_stream():
    dev = engine.require_gpu()
    n, H, frac, K, Kc = 300, 37, 0.6, 3, 4
    idx, lab, cl, C, S_ref = _case(n, H, frac, K, Kc)
    L, Hpad = _device_labels(idx, [lab], n, H, dev)
    wide = torch.full((n, Hpad + 128), 0x07, dtype=torch.uint8, device=dev)  # junk past Hpad
    view = wide[:, :Hpad]
    view.copy_(L[0])
    assert view.stride(0) == Hpad + 128
    S = engine.item_consensus_sums(view, n, Hpad, K, cl, Kc)
    np.testing.assert_array_equal(S.cpu().numpy(), S_ref)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        S2 = engine.item_consensus_sums(L[0], n, Hpad, K, cl, Kc)
    side.synchronize()
    np.testing.assert_array_equal(S2.cpu().numpy(), S_ref)


def test_abi_errors_launch_nothing():
    dev = engine.require_gpu()
    n, H, frac, K, Kc = 300, 37, 0.6, 3, 4
    idx, lab, cl, C, S_ref = _case(n, H, frac, K, Kc)
    L, Hpad = _device_labels(idx, [lab], n, H, dev)
    nt = engine.num_tiles(n)
    I_tiles, _ = engine.cosample(L[0], n, Hpad, 0, nt)
    cl_d = torch.from_numpy(cl.copy()).to(dev)
    S = torch.zeros((n, 128), dtype=torch.int64, device=dev)  # room for any Kc tried here

    def call(K=K, Kc=Kc, S_ptr=S.data_ptr(), te=nt, cl_ptr=cl_d.data_ptr(), I_ptr=I_tiles.data_ptr()):
        _lib.call("cc_item_consensus", L[0].data_ptr(), n, L[0].stride(0), Hpad, K, 0, te, I_ptr,
                  cl_ptr, Kc, S_ptr, engine.stream_ptr())

    for bad in (dict(Kc=0), dict(Kc=128), dict(K=0), dict(K=128), dict(S_ptr=None),
                dict(S_ptr=S.data_ptr() + 4), dict(te=nt + 1), dict(cl_ptr=None), dict(I_ptr=None)):
        with pytest.raises(_lib.CCMIError, match="cc_item_consensus"):
            call(**bad)
    torch.cuda.synchronize()
    assert not bool(S.any()), "a rejected call must not launch"
    with pytest.raises(_lib.CCMIError):  # the engine reaches the same checks
        engine.item_consensus_sums(L[0], n, Hpad, K, cl, 0)
    with pytest.raises(_lib.CCMIError):
        engine.item_consensus_sums(L[0], n, Hpad, K, cl, Kc, 0, nt + 1)
    _lib.call("cc_item_consensus", L[0].data_ptr(), n, L[0].stride(0), Hpad, K, 2, 2, None,
              cl_d.data_ptr(), Kc, S.data_ptr(), engine.stream_ptr())  # an empty range is fine


# ---------------------------------------------------------------- the public API

FIXTURE = "blobs_n400_d8_k4"


def _fit(keep):
    f = load_fixture(FIXTURE)
    meta = f["meta"]
    cc = ConsensusClustering(K_range=[int(k) for k in f["K_range"]], n_iterations=meta["H"],
                             subsampling=meta["subsampling"], random_state=meta["random_state"],
                             plot_cdf=False, keep_matrices=keep)
    return cc.fit(f["X"])


@pytest.fixture(scope="module")
def fitted():
    return _fit(True), _fit(False)


def test_api_sums_do_not_depend_on_keep_matrices(fitted):
    kept, lean = fitted
    assert kept.cdf_at_K_data[kept.best_k_]["cij"] is not None
    assert lean.cdf_at_K_data[lean.best_k_]["cij"] is None
    before = {K: dict(v) for K, v in lean.cdf_at_K_data.items()}
    for K in kept.cdf_at_K_data:
        a, b = kept.consensus_sums(K), lean.consensus_sums(K)
        assert isinstance(a, np.ndarray) and a.dtype == np.int64
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(kept.consensus_sums(), kept.consensus_sums(kept.best_k_))
    for K, v in lean.cdf_at_K_data.items():  # the reference's result dict is untouched
        assert list(v) == list(before[K]) and v["consensus_labels"] == [] and v["cij"] is None


def test_api_equals_the_kept_matrix(fitted):
    kept, _ = fitted
    n = kept._N
    for K in kept.cdf_at_K_data:
        labels = kept.predict(K)
        Kc = int(labels.max()) + 1
        S_ref = _sums_from_C(kept.cdf_at_K_data[K]["cij"], labels, Kc)
        np.testing.assert_array_equal(kept.consensus_sums(K), S_ref)
        item = kept.item_consensus(K)
        np.testing.assert_array_equal(item, post.item_consensus_from_sums(S_ref, labels, Kc))
        np.testing.assert_array_equal(kept.cluster_consensus(K),
                                      post.cluster_consensus_from_sums(S_ref, labels, Kc))
        assert item.shape == (n, Kc)
        ok = ~np.isnan(item)
        assert ok.any() and (item[ok] >= 0).all() and (item[ok] <= 1).all()
    # a partition from elsewhere
    given = (np.arange(n) % 3).astype(np.int16)
    K = list(kept.cdf_at_K_data)[0]
    np.testing.assert_array_equal(kept.consensus_sums(K, given),
                                  _sums_from_C(kept.cdf_at_K_data[K]["cij"], given.astype(np.int64), 3))


def test_api_icl_covers_k_range(fitted):
    _, lean = fitted
    out = lean.icl()
    assert list(out) == list(lean.cdf_at_K_data)
    for K, v in out.items():
        assert set(v) == {"consensus_labels", "item_consensus", "cluster_consensus"}
        np.testing.assert_array_equal(v["consensus_labels"], lean.predict(K))
        np.testing.assert_array_equal(v["item_consensus"], lean.item_consensus(K))
        np.testing.assert_array_equal(v["cluster_consensus"], lean.cluster_consensus(K))
    K = list(lean.cdf_at_K_data)[-1]
    assert list(lean.icl([K])) == [K]


def test_api_errors(fitted):
    _, lean = fitted
    n = lean._N
    fresh = ConsensusClustering(K_range=[2, 3], plot_cdf=False, random_state=0)
    for method in (fresh.consensus_sums, fresh.item_consensus, fresh.cluster_consensus, fresh.icl):
        with pytest.raises(ValueError):
            method()
    with pytest.raises(KeyError):
        lean.consensus_sums(99)
    with pytest.raises(KeyError):
        lean.icl([99])
    K = list(lean.cdf_at_K_data)[0]
    with pytest.raises(ValueError):
        lean.consensus_sums(K, np.zeros(n - 1, dtype=np.int64))
    with pytest.raises(ValueError):
        lean.item_consensus(K, np.full(n, -1))
    with pytest.raises(ValueError):
        lean.cluster_consensus(K, np.full(n, 127))
    with pytest.raises(ValueError):
        lean.consensus_sums(K, np.zeros(n, dtype=np.float64))


def test_two_ranks_equal_one_rank(tmp_path, fitted):
    """Two gloo ranks on cuda:0 (tests/icl_dist_worker.py): each rank sums its share of the
    triangle tiles, the int64 SUM all-reduce merges them; equal to the one-rank sums exactly."""
    _, lean = fitted
    K = list(lean.cdf_at_K_data)[1]
    out = str(tmp_path / "r0.npz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "icl_dist_worker.py"), FIXTURE, "2",
                    str(K), out], check=True, timeout=300, env=env)
    from tests.icl_dist_worker import given_labels

    got = np.load(out)
    np.testing.assert_array_equal(got["predicted"], lean.consensus_sums(K))
    np.testing.assert_array_equal(got["given"], lean.consensus_sums(K, given_labels(lean._N)))
