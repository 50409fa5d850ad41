"""cc_cosample / cc_coassoc (tiles_kernel, csrc/coassoc.hip) at the edges of their contract in
include/ccmi.h: sharded tile ranges over interior tiles for every binning form, a row stride
beyond Hpad with live bytes behind the window, counts above 32 767, every channel of the 64-
and 128-channel paddings, tile-aligned and tiny n; and cc_consensus at small n and full-range
counts.  Every expected value is an exact integer (or float32) from the numpy references of
tests/consensus_edges_ref.py; nothing is compared with a tolerance."""
import functools

import numpy as np
import pytest
import torch

from consensus_clustering_amd import _lib, engine
from oracle import cc_oracle as O
from tests import consensus_edges_ref as R
from tests.test_gpu_coassoc import _random_case

pytestmark = pytest.mark.gpu

CC_ERR_ARG = -1


def _upload(W, Hpad, dev, ldl=None, K=None, seed=0):
    """The label bytes W [n, H] as a device window [n, Hpad] of an [n, ldl] allocation (ldl =
    Hpad: contiguous).  Columns [H, Hpad) are 0xFF; columns >= Hpad hold live labels in [0, K) on
    nine rows in ten, so that any read the kernel does not mask by Hpad changes a count."""
    n, H = W.shape
    ldl = Hpad if ldl is None else ldl
    buf = np.full((n, ldl), 0xFF, dtype=np.uint8)
    buf[:, :H] = W
    if ldl > Hpad:
        rng = np.random.default_rng(seed)
        live = rng.integers(0, K, size=(n, ldl - Hpad)).astype(np.uint8)
        live[rng.random(n) < 0.1] = 0xFF
        buf[:, Hpad:] = live
    return torch.from_numpy(buf).to(dev)[:, :Hpad]


def _run(Lv, n, Hpad, K, ranges=None, want_full=False, use_table=True):
    """(I, M, counts) of one K over the tile ranges, accumulated as the sharded fit does."""
    dev = Lv.device
    ranges = ranges or [(0, engine.num_tiles(n))]
    edges = engine.edges_device(dev)
    counts = torch.zeros(20, dtype=torch.int64, device=dev)
    I = torch.zeros((n, n), dtype=torch.int32, device=dev) if want_full else None
    M = torch.zeros((n, n), dtype=torch.int32, device=dev) if want_full else None
    for tb, te in ranges:
        I_tiles, I_part = engine.cosample(Lv, n, Hpad, tb, te, want_full=want_full)
        Mp = torch.zeros((n, n), dtype=torch.int32, device=dev) if want_full else None
        engine.coassoc(Lv, n, Hpad, K, tb, te, I_tiles, edges, counts, Mp, use_table=use_table)
        if want_full:
            I += I_part
            M += Mp
    torch.cuda.synchronize()
    return (I.cpu().numpy() if want_full else None, M.cpu().numpy() if want_full else None,
            counts.cpu().numpy())


@pytest.fixture
def coassoc_calls(monkeypatch):
    """The (bin_table pointer, table_rows) of every cc_coassoc call made through the engine."""
    seen = []
    real = _lib.call

    def spy(name, *args):
        if name == "cc_coassoc":
            seen.append((args[11], args[12]))
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    return seen


def _table_form(rows):
    """The staged form of a table of `rows` rows (bt_form, coassoc.hip:83): 2 = triangle,
    1 = threshold pairs, 0 = uint16 thresholds, None = no table (division path)."""
    lib = _lib.load()
    for form in (2, 1, 0):
        if rows <= lib.cc_bin_table_form_rows(form):
            return form
    return None


# ---------------------------------------------------------------- A1: sharded interior tiles

A1_N, A1_KS, A1_CUTS = 1100, [2, 5, 17], [(0, 3), (3, 12), (12, 15)]
A1_FORMS = [("triangle", 256, 2), ("pairs", 1024, 1), ("uint16", 1920, 0), ("none", 2048, None)]


@functools.lru_cache(maxsize=None)
def _a1_case(Hpad):
    """(label bytes per K, numpy's 20 counts per K) for n = 1100 and H = Hpad - 5."""
    n, H = A1_N, Hpad - 5
    idx, labs = _random_case(n, H, 0.8, A1_KS, seed=Hpad)
    Ws = [R.label_matrix(idx, lab, n) for lab in labs]
    hists = []
    for W, K in zip(Ws, A1_KS):
        I, M = R.counts_ref(W, K)
        hists.append(R.pair_hist(M, I))
    return Ws, hists


@pytest.mark.parametrize("name,Hpad,form", A1_FORMS, ids=[f[0] for f in A1_FORMS])
def test_sharded_ranges_over_interior_tiles(name, Hpad, form, coassoc_calls):
    """Multi-GPU mode B's launches: tile_begin > 0, no n x n matrix, interior tiles.  n = 1100 is
    5 x 5 blocks = 15 tiles, (0,1)..(2,3) interior (coassoc.hip:843: btab && !diag &&
    (bj + 1) * 256 <= n && !full_out), column block 4 masked.  The ranges (0, 3), (3, 12), (12, 15)
    put interior tiles behind tile_begin = 3; the 9-workgroup middle launch deals its tiles with
    xq = 1, xr = 1 (coassoc.hip:602-603), and each tile must read its own I tile at
    tl = t - tile_begin (coassoc.hip:765, :839).  Per form -- triangle (coassoc.hip:844), pairs
    (:870), uint16 (:909), no table (the division path, :954-979) -- the summed counters equal the
    single-range run, the use_table=False run and numpy's histogram."""
    assert _table_form(Hpad + 1) == form
    dev = engine.require_gpu()
    n = A1_N
    assert engine.num_tiles(n) == 15
    Ws, hists = _a1_case(Hpad)
    for W, K, want in zip(Ws, A1_KS, hists):
        Lv = _upload(W, Hpad, dev)
        del coassoc_calls[:]
        _, _, sharded = _run(Lv, n, Hpad, K, ranges=A1_CUTS)
        _, _, single = _run(Lv, n, Hpad, K)
        # every launch so far was handed the table of this form (or none past the largest)
        assert len(coassoc_calls) == 4
        for tab, rows in coassoc_calls:
            assert (tab is not None, rows) == (form is not None, Hpad + 1 if form is not None else 0)
        _, _, division = _run(Lv, n, Hpad, K, use_table=False)
        assert coassoc_calls[-1] == (None, 0)
        print(f"{name} K={K} counts {sharded.tolist()}")
        assert int(want.sum()) == n * (n - 1) // 2
        np.testing.assert_array_equal(sharded, want, err_msg=f"{name} K={K} sharded")
        np.testing.assert_array_equal(single, want, err_msg=f"{name} K={K} single range")
        np.testing.assert_array_equal(division, want, err_msg=f"{name} K={K} division")


def test_sharded_ranges_through_coassoc_all():
    """The same sharded launches as the fit issues them: engine.coassoc_all over three side
    streams, per tile range, with the threshold-pair table (Hpad = 1024)."""
    dev = engine.require_gpu()
    n, Hpad = A1_N, 1024
    assert _table_form(Hpad + 1) == 1
    Ws, hists = _a1_case(Hpad)
    L = torch.stack([_upload(W, Hpad, dev) for W in Ws])
    counts = torch.zeros((len(A1_KS), 20), dtype=torch.int64, device=dev)
    for tb, te in A1_CUTS:
        I_tiles, _ = engine.cosample(L[0], n, Hpad, tb, te, want_full=False)
        engine.coassoc_all(L, n, Hpad, A1_KS, tb, te, I_tiles, counts, None, streams=3)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(counts.cpu().numpy(), np.stack(hists))


# ---------------------------------------------------------------- A2: ldl > Hpad

A2_N = 300
A2_K_PACK = [(2, "default"), (3, "default"), (8, "default"), (9, "default"), (17, "exact"), (17, "pow2"),
             (18, "exact"), (18, "pow2"), (33, "default"), (100, "default")]


@functools.lru_cache(maxsize=None)
def _a2_case(H, K):
    W = R.random_label_bytes(A2_N, H, 0.7, K, seed=1000 * H + K)
    I, M = R.counts_ref(W, K)
    return W, I, M, R.pair_hist(M, I)


@pytest.mark.parametrize("H", [37, 200])
@pytest.mark.parametrize("K,pack", A2_K_PACK, ids=[f"K{k}-{p}" for k, p in A2_K_PACK])
def test_row_stride_beyond_hpad(K, pack, H, monkeypatch):
    """ccmi.h: the first Hpad columns of an [n][ldl] matrix, Hpad <= ldl.  With ldl = Hpad + 16,
    Hpad + 144 and 2 Hpad the bytes at columns >= Hpad are live labels, so a load form chosen
    from ldl that is not masked back to Hpad adds counts: the exact-K dword form (K = 17, 18
    under CCMI_CO_PACK=exact: load_raw's `o + 16 <= ldl`, coassoc.hip:392, then realign's
    tail mask by Hpad, :461-468), the power-of-two forms (load_labels, :228, steps of HS | 128
    bytes inside Hpad) and the co-sampling kernel's 128-byte rows.  cc_coassoc builds the exact
    form only for K = 17 and 18 (coassoc.hip:1464-1469), so the 16-B clamped form of K < 10
    (:404-414) is not instantiated and K = 3, 8, 9 run padded to a power of two.  I, M and the
    counts, with and without the n x n matrices, equal numpy and the contiguous [n][Hpad] run."""
    if pack != "default":
        monkeypatch.setenv("CCMI_CO_PACK", pack)
    dev = engine.require_gpu()
    n, Hpad = A2_N, engine.pad_h(H)
    W, I_ref, M_ref, want = _a2_case(H, K)
    Lc = _upload(W, Hpad, dev)
    assert Lc.is_contiguous()
    I_c, M_c, c_c = _run(Lc, n, Hpad, K, want_full=True)
    for ldl in (Hpad + 16, Hpad + 144, 2 * Hpad):
        Lv = _upload(W, Hpad, dev, ldl=ldl, K=K, seed=ldl)
        assert Lv.stride(0) == ldl and Lv.shape == (n, Hpad) and Lv.data_ptr() % 16 == 0
        I, M, c_full = _run(Lv, n, Hpad, K, want_full=True)
        _, _, c_lean = _run(Lv, n, Hpad, K, want_full=False)
        for got, ref, con, what in ((I, I_ref, I_c, "I"), (M, M_ref, M_c, "M"), (c_full, want, c_c, "counts"),
                                    (c_lean, want, c_c, "counts without matrices")):
            np.testing.assert_array_equal(got, ref, err_msg=f"{what} ldl={ldl}")
            np.testing.assert_array_equal(got, con, err_msg=f"{what} ldl={ldl} against contiguous")


# ---------------------------------------------------------------- A3: counts above 32 767

A3_N, A3_H = 130, 32900


@functools.lru_cache(maxsize=None)
def _a3_case(K):
    n, H = A3_N, A3_H
    W = R.random_label_bytes(n, H, 0.8, K, seed=K)
    rng = np.random.default_rng(K + 1)
    # a row keeps a label of its own in a fraction q of its resamples (q from 0 to 1 over the
    # rows), so the consensus values spread over the 20 bins instead of piling up at 1 / K
    own = rng.integers(0, K, size=(n, 1)).astype(np.uint8)
    keep = (rng.random((n, H)) < np.linspace(0, 1, n)[:, None]) & (W != 0xFF)
    W = np.where(keep, own, W)
    top = W[:64].copy()  # rows 0..63: in every resample
    top[top == 0xFF] = rng.integers(0, K, size=int((top == 0xFF).sum())).astype(np.uint8)
    top[0] = np.arange(H) % K
    top[1] = (np.arange(H) + 1) % K  # never the label of row 0
    top[2:10] = rng.integers(0, K, size=H).astype(np.uint8)  # always one label
    W[:64] = top
    I, M = R.counts_ref(W, K)
    return W, I, M, R.pair_hist(M, I)


@pytest.mark.parametrize("K", [2, 3, 17, 100])
def test_counts_above_int16(K, coassoc_calls):
    """H = 32 900 (Hpad = 33 024): rows 0..63 are in every resample, so I = H > 32 767 there, the
    uint16 I tiles (packed at coassoc.hip:784-785, read back `& 0xFFFF` at :963) live in a
    torch.int16 tensor and must come back unsigned; rows 0 and 1 never share a label (M = 0),
    rows 2..9 always do (M = H).  Hpad + 1 is beyond cc_bin_table_max_rows(), so cc_coassoc is
    handed no table and every pair bins by division (consensus_bin, :105).  i8 (K = 2), FP4
    padded (K = 3, 100) and FP4 exact (K = 17) accumulators."""
    dev = engine.require_gpu()
    n, H, Hpad = A3_N, A3_H, engine.pad_h(A3_H)
    assert Hpad == 33024 and Hpad + 1 > _lib.load().cc_bin_table_max_rows()
    assert engine.bin_table(dev, Hpad + 1) is None
    W, I_ref, M_ref, want = _a3_case(K)
    assert I_ref[0, 63] == H and I_ref.max() == H > 32767
    assert M_ref[0, 1] == 0 and M_ref[2, 9] == H
    Lv = _upload(W, Hpad, dev)
    I, M, c_full = _run(Lv, n, Hpad, K, want_full=True)
    _, _, c_lean = _run(Lv, n, Hpad, K, want_full=False)
    assert coassoc_calls == [(None, 0), (None, 0)]
    np.testing.assert_array_equal(I, I_ref)
    np.testing.assert_array_equal(M, M_ref)
    np.testing.assert_array_equal(c_full, want)
    np.testing.assert_array_equal(c_lean, want)


def test_hpad_65536_is_refused():
    """Hpad = 65 536 would wrap the uint16 I tiles: cc_cosample and cc_coassoc return CC_ERR_ARG
    (check_common, coassoc.hip:1294) and launch nothing -- the tile buffer and the counters keep
    their contents.  The buffers are full size, so even an unrefused launch stays in bounds."""
    dev = engine.require_gpu()
    lib = _lib.load()
    n, Hpad = 2, 65536
    L = torch.zeros((n, Hpad), dtype=torch.uint8, device=dev)
    I_tiles = torch.full((1, engine.TILE * engine.TILE), 0x5A5A, dtype=torch.int16, device=dev)
    counts = torch.full((20,), 7, dtype=torch.int64, device=dev)
    edges = engine.edges_device(dev)
    st = engine.stream_ptr()
    assert lib.cc_cosample(L.data_ptr(), n, Hpad, Hpad, 0, 1, I_tiles.data_ptr(), None, st) == CC_ERR_ARG
    assert b"65535" in lib.cc_last_error()
    assert lib.cc_coassoc(L.data_ptr(), n, Hpad, Hpad, 2, 0, 1, I_tiles.data_ptr(), edges.data_ptr(),
                          counts.data_ptr(), None, None, 0, st) == CC_ERR_ARG
    assert b"65535" in lib.cc_last_error()
    torch.cuda.synchronize()
    assert bool((I_tiles == 0x5A5A).all()) and counts.tolist() == [7] * 20
    with pytest.raises(_lib.CCMIError, match="65535"):
        engine.cosample(L, n, Hpad, 0, 1)


# ---------------------------------------------------------------- A4: channel boundaries

@pytest.mark.parametrize("K", [1, 33, 63, 64, 65, 96, 127])
def test_every_channel_of_the_padded_slices(K):
    """Labels drawn uniformly over all K channels at the padding boundaries: K = 33, 63, 64 fill
    tiles_kernel<64> up to its last channel, K = 65, 96, 127 tiles_kernel<128> (the dispatch of
    coassoc.hip:1462-1476; expand_chunk_f4's channel slices `lab >> 3 == cq`, :334-337), K = 1
    the i8 form padded to two.  M against one A_c A_c^T per channel, and the 20 counts."""
    dev = engine.require_gpu()
    n, H = 300, 131
    Hpad = engine.pad_h(H)
    W = R.random_label_bytes(n, H, 0.7, K, seed=K)
    assert len(np.unique(W[W != 0xFF])) == K  # every channel is live
    I_ref, M_ref = R.counts_ref(W, K)
    want = R.pair_hist(M_ref, I_ref)
    Lv = _upload(W, Hpad, dev)
    I, M, c_full = _run(Lv, n, Hpad, K, want_full=True)
    _, _, c_lean = _run(Lv, n, Hpad, K, want_full=False)
    np.testing.assert_array_equal(I, I_ref)
    np.testing.assert_array_equal(M, M_ref)
    np.testing.assert_array_equal(c_full, want)
    np.testing.assert_array_equal(c_lean, want)


# ---------------------------------------------------------------- A5: n boundaries

@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 512])
def test_tile_aligned_and_tiny_n(n, K):
    """n on and next to the tile edge, and the smallest n.  At n = 256 and 512 no row is masked
    (`grow < n`, coassoc.hip:611) and `(bj + 1) * 256 <= n` (:843) holds with equality: at 512
    tile (0, 1) is interior and the last column block at once, and takes the unmasked table path
    only in the run without matrices, which must equal the run with them.  n = 1 has no pair at
    all, n = 2 one."""
    dev = engine.require_gpu()
    H = 37
    Hpad = engine.pad_h(H)
    W = R.random_label_bytes(n, H, 0.8, K, seed=10 * n + K)
    I_ref, M_ref = R.counts_ref(W, K)
    want = R.pair_hist(M_ref, I_ref)
    assert int(want.sum()) == n * (n - 1) // 2
    Lv = _upload(W, Hpad, dev)
    I, M, c_full = _run(Lv, n, Hpad, K, want_full=True)
    _, _, c_lean = _run(Lv, n, Hpad, K, want_full=False)
    np.testing.assert_array_equal(I, I_ref)
    np.testing.assert_array_equal(M, M_ref)
    np.testing.assert_array_equal(c_full, want)
    np.testing.assert_array_equal(c_lean, want)
    np.testing.assert_array_equal(c_lean, c_full)


# ---------------------------------------------------------------- cc_consensus

@pytest.mark.parametrize("n", [1, 3, 4, 8])
def test_consensus_small_n_full_range_counts(n):
    """cc_consensus at the smallest n of both kernels (n % 4 == 0: consensus_rows_kernel,
    coassoc.hip:1236, one 16-B access per row at n = 4; else the flat consensus_kernel, :1273),
    with co-sampling counts drawn up to 65 535 and I = 0 entries (never co-sampled: M = 0 and
    C = 0 / 1e-6 = 0), against numpy's float32 divide bit for bit."""
    dev = engine.require_gpu()
    rng = np.random.default_rng(n)
    I = rng.integers(0, 65536, size=(n, n))
    I = np.maximum(I, I.T)
    I[rng.random((n, n)) < 0.3] = 0
    I.flat[:: n + 1] = 65535
    if n > 1:
        I[0, 1] = 65535
        I[1, 0] = 0
    M = np.floor(I * rng.random((n, n))).astype(np.int64)
    if n > 1:
        M[0, 1] = 65535
    Md, Id = torch.from_numpy(M.astype(np.int32)).to(dev), torch.from_numpy(I.astype(np.int32)).to(dev)
    assert (Md.data_ptr() | Id.data_ptr()) % 16 == 0  # n % 4 == 0 then takes the row kernel
    C = engine.consensus(Md, Id).cpu().numpy()
    want = O.consensus_matrix(M.astype(np.uint16), I.astype(np.uint16))
    assert C.dtype == np.float32
    np.testing.assert_array_equal(C.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(np.diag(C), 1.0)
    assert np.all(C[(I == 0) & ~np.eye(n, dtype=bool)] == 0.0)
