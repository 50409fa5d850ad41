"""Device engine: torch-ROCm tensors as raw buffers around the libccmi C ABI.

Torch is plumbing here (device memory, the current HIP stream, torch.distributed);
every count, label and histogram is produced by the gfx950 kernels in
``csrc/`` through ``_lib``.  No function in this module has a CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .post import N_BINS, bin_edges32

TILE = 256
HALIGN = 128  # resample padding of the sample-major label matrix (Hpad % 128 == 0)


def require_gpu(device=None) -> torch.device:
    """The torch device to run on; raises if there is no GPU or no libccmi.so."""
    if not torch.cuda.is_available():
        raise _lib.CCMIError(
            "consensus_clustering_amd needs a ROCm GPU (torch.cuda.is_available() is False)")
    _lib.load()
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


# Optional per-launch HIP-event timing (bench.py): {kernel name: [(start, end), ...]}.
TIMERS = None


class timed:
    """Record HIP events around a launch on the current stream when TIMERS is enabled."""

    def __init__(self, name):
        self.name = name
        self.ev = None

    def __enter__(self):
        if TIMERS is not None:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()
        return self

    def __exit__(self, *exc):
        if self.ev is not None:
            self.ev[1].record()
            TIMERS.setdefault(self.name, []).append(self.ev)
        return False


def timer_summary(timers) -> dict:
    """{name: (launches, total ms)} after a synchronize."""
    return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in timers.items()}


def pad_h(H: int) -> int:
    return ((H + HALIGN - 1) // HALIGN) * HALIGN


def num_tiles(n: int) -> int:
    return int(_lib.load().cc_num_tiles(int(n)))


# ---------------------------------------------------------------- host-native RNG

def resample_indices(seed: int, n: int, m: int, h_begin: int, h_end: int, n_threads: int = 0) -> np.ndarray:
    """int32 [h_end-h_begin, m]: RandomState(seed+h).choice(n, m, replace=False) (CC.py:231-239)."""
    if seed is None:
        # the reference computes `self.random_state + i` (CC.py:232)
        raise TypeError("unsupported operand type(s) for +: 'NoneType' and 'int'")
    seed = int(seed)
    if seed < 0 or seed + h_end - 1 > 2**32 - 1:
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    out = np.empty((h_end - h_begin, m), dtype=np.int32)
    _lib.call("cc_resample_indices", ctypes.c_uint32(seed), h_begin, h_end, n, m,
              out.ctypes.data, n_threads)
    return out


# workspace cap of the swap-partner resampling (resamples run in batches that fit; 4 GiB holds
# every resample of C5 in one batch, one workgroup per resample across the whole GPU)
RESAMPLE_WIDE_WS = 4 << 30


RESAMPLE_SWAP_MAX_AUTO = 16384  # 'auto' uses the LDS swap chain up to this n, the wide form above


def resample_indices_device(seed: int, n: int, m: int, h_begin: int, h_end: int, device,
                            out: torch.Tensor | None = None, method: str = "auto") -> torch.Tensor:
    """int32 [h_end-h_begin, m] on the device: the same draws as resample_indices.
    method 'swap': cc_resample_device (the shuffle simulated in LDS; n <= 65536); 'wide':
    cc_resample_device_wide (any n, resolved from the swap partners); 'auto': wide when
    n > 16384 (faster from there: C3 n = 50k 7.3 against 24.7 ms; equal at n = 10k) else swap.  `out`: a contiguous int32 device tensor of that shape to fill (e.g. a
    row slice of the full [H, m] matrix)."""
    if seed is None:
        raise TypeError("unsupported operand type(s) for +: 'NoneType' and 'int'")
    seed = int(seed)
    if seed < 0 or seed + h_end - 1 > 2**32 - 1:
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    if out is None:
        out = torch.empty((h_end - h_begin, m), dtype=torch.int32, device=device)
    elif (tuple(out.shape) != (h_end - h_begin, m) or out.dtype != torch.int32 or not out.is_contiguous()
          or not out.is_cuda):
        raise ValueError("out must be a contiguous int32 device tensor of shape [h_end - h_begin, m]")
    if method == "auto":
        method = "wide" if n > RESAMPLE_SWAP_MAX_AUTO else "swap"
    if method == "swap":
        _lib.call("cc_resample_device", ctypes.c_uint32(seed), h_begin, h_end, n, m,
                  out.data_ptr() if out.numel() else None, stream_ptr(device))
    elif method == "wide":
        lib = _lib.load()
        nh = max(h_end - h_begin, 1)
        per = int(lib.cc_resample_device_wide_workspace_bytes(n, 1))
        nb = max(1, min(nh, RESAMPLE_WIDE_WS // max(per, 1)))
        ws = torch.empty(per * nb, dtype=torch.uint8, device=device)
        _lib.call("cc_resample_device_wide", ctypes.c_uint32(seed), h_begin, h_end, n, m,
                  out.data_ptr() if out.numel() else None, ws.data_ptr(), ws.numel(),
                  stream_ptr(device))
    else:
        raise ValueError("method must be 'auto', 'swap' or 'wide'")
    return out


def resample_device_max_n() -> int:
    """Largest n of the LDS shuffle (cc_resample_device); the wide form has no limit."""
    return int(_lib.load().cc_resample_device_max_n())


def random_sample(seed: int, count: int) -> np.ndarray:
    """RandomState(seed).random_sample(count) via the native MT19937."""
    out = np.empty(count, dtype=np.float64)
    _lib.call("cc_random_sample", ctypes.c_uint32(int(seed)), int(count),
              out.ctypes.data if count else None)
    return out


# ---------------------------------------------------------------- label matrices

def new_label_matrix(nK: int, n: int, Hpad: int, device) -> torch.Tensor:
    """uint8 [nK, n, Hpad] filled with 0xFF (= not sampled)."""
    return torch.full((nK, n, Hpad), 0xFF, dtype=torch.uint8, device=device)


def scatter_labels(idx_hm: torch.Tensor, labels_hm, n: int, out_nh: torch.Tensor, h_offset: int = 0):
    """out_nh[idx[h, r], h_offset + h] = labels[h, r] (or 0 when labels_hm is None)."""
    H, m = idx_hm.shape
    assert idx_hm.dtype == torch.int32 and idx_hm.is_contiguous()
    assert out_nh.dtype == torch.uint8 and out_nh.dim() == 2 and out_nh.shape[0] == n
    assert out_nh.stride(1) == 1
    ldl = out_nh.stride(0)
    if labels_hm is not None:
        assert labels_hm.dtype == torch.int32 and tuple(labels_hm.shape) == (H, m)
        labels_hm = labels_hm.contiguous()
    if H == 0 or m == 0:  # a rank that owns no resample (dist.shard) has nothing to place
        return  # (an empty tensor's data pointer is NULL, which cc_scatter_labels refuses)
    base = out_nh[:, h_offset:]
    _lib.call("cc_scatter_labels", _lib.ptr(idx_hm), _lib.ptr(labels_hm), H, m, n,
              base.data_ptr(), ldl, stream_ptr())


def copy_label_columns(src: torch.Tensor, col_src: int, dst: torch.Tensor, col_dst: int, width: int):
    """dst[..., col_dst:col_dst+width] = src[..., col_src:col_src+width] for two device uint8
    label matrices of the same leading shape (cc_copy_label_columns, one launch)."""
    assert src.dtype == torch.uint8 and dst.dtype == torch.uint8 and src.is_cuda and dst.is_cuda
    assert src.is_contiguous() and dst.is_contiguous() and src.shape[:-1] == dst.shape[:-1]
    rows = src.numel() // src.shape[-1] if src.numel() else 0
    _lib.call("cc_copy_label_columns", src.data_ptr(), src.shape[-1], int(col_src), dst.data_ptr(),
              dst.shape[-1], int(col_dst), rows, int(width), stream_ptr(src.device))


# ---------------------------------------------------------------- co-sampling / co-association

def cosample(labels_nh: torch.Tensor, n: int, Hpad: int, tile_begin: int, tile_end: int,
             want_full: bool = False):
    """I tiles (uint16 accumulator order) for [tile_begin, tile_end), optional full int32 I."""
    dev = labels_nh.device
    ntl = tile_end - tile_begin
    I_tiles = torch.empty((max(ntl, 0), TILE * TILE), dtype=torch.int16, device=dev)
    I_full = torch.zeros((n, n), dtype=torch.int32, device=dev) if want_full else None
    with timed("cc_cosample"):
        _lib.call("cc_cosample", labels_nh.data_ptr(), n, labels_nh.stride(0), Hpad, tile_begin,
                  tile_end, I_tiles.data_ptr(), _lib.ptr(I_full), stream_ptr())
    return I_tiles, I_full


def edges_device(device) -> torch.Tensor:
    return torch.from_numpy(bin_edges32().copy()).to(device)


_BIN_TABLES = {}


def bin_table(device, rows: int):
    """Cached cc_bin_table thresholds for co-sampling counts [0, rows), or None when the table
    is too large to stage on chip (cc_coassoc then bins by division)."""
    if rows > _lib.load().cc_bin_table_max_rows():
        return None
    key = (str(device), rows)
    t = _BIN_TABLES.get(key)
    if t is None:
        nbytes = int(_lib.load().cc_bin_table_bytes(rows))
        t = torch.zeros(nbytes // 2, dtype=torch.int16, device=device)
        _lib.call("cc_bin_table", rows, edges_device(device).data_ptr(), t.data_ptr(), nbytes,
                  stream_ptr())
        _BIN_TABLES[key] = t
    return t


def coassoc(labels_nh: torch.Tensor, n: int, Hpad: int, K: int, tile_begin: int, tile_end: int,
            I_tiles: torch.Tensor, edges: torch.Tensor, counts: torch.Tensor,
            M_full: torch.Tensor = None, use_table: bool = True):
    """Accumulate the strict-upper-pair histogram of C for one K into counts (int64[20])."""
    assert counts.dtype == torch.int64 and counts.numel() == N_BINS
    tab = bin_table(labels_nh.device, Hpad + 1) if use_table else None
    with timed("cc_coassoc"):
        _lib.call("cc_coassoc", labels_nh.data_ptr(), n, labels_nh.stride(0), Hpad, int(K),
                  tile_begin, tile_end, I_tiles.data_ptr(), edges.data_ptr(), counts.data_ptr(),
                  _lib.ptr(M_full), _lib.ptr(tab), Hpad + 1 if tab is not None else 0,
                  stream_ptr())


_SIDE_STREAMS = {}


def side_streams(device, count: int):
    """`count` cached HIP streams of `device` for independent launches (the per-K co-association
    launches of a fit): a launch covers only the tiles of one K, so at small n its last round of
    tiles leaves CUs idle that the next K's launch can fill."""
    key = str(device)
    have = _SIDE_STREAMS.setdefault(key, [])
    while len(have) < count:
        have.append(torch.cuda.Stream(device=device))
    return have[:count]


def coassoc_all(labels: torch.Tensor, n: int, Hpad: int, Ks, tile_begin: int, tile_end: int,
                I_tiles: torch.Tensor, counts: torch.Tensor, M_full=None, streams: int = 2):
    """coassoc for every K (labels[k], counts[k], M_full[k]), the launches dealt round robin over
    `streams` side streams forked from and joined back into the current stream.  The K are
    independent (own label matrix, own counters), so the results do not depend on the overlap."""
    dev = labels.device
    edges = edges_device(dev)
    bin_table(dev, Hpad + 1)  # staged once on the current stream, before any side stream reads it
    main = torch.cuda.current_stream(dev)
    if streams <= 1 or len(Ks) <= 1:
        for k, K in enumerate(Ks):
            coassoc(labels[k], n, Hpad, K, tile_begin, tile_end, I_tiles, edges, counts[k],
                    None if M_full is None else M_full[k])
        return
    ss = side_streams(dev, min(int(streams), len(Ks)))
    with timed("coassoc_band"):
        for s in ss:
            s.wait_stream(main)
        for k, K in enumerate(Ks):
            with torch.cuda.stream(ss[k % len(ss)]):
                coassoc(labels[k], n, Hpad, K, tile_begin, tile_end, I_tiles, edges, counts[k],
                        None if M_full is None else M_full[k])
        for s in ss:
            main.wait_stream(s)


def item_consensus_sums(labels_nh: torch.Tensor, n: int, Hpad: int, K: int, cl, Kc: int,
                        tile_begin: int = 0, tile_end: int = None, S: torch.Tensor = None,
                        tile_chunk: int = 2048) -> torch.Tensor:
    """int64 [n, Kc] on the device: S[i, c] += sum over j != i with cl[j] == c of C_ij * 2^40
    (exact integers) for the pairs of tiles [tile_begin, tile_end) (default: all of them), from
    the label matrix of one K.  cl: int32 [n] (device tensor, or any host int array), an id
    outside [0, Kc) = no cluster.  S is accumulated into when given (int64 [n, Kc], contiguous),
    else it starts at zero.  The range is walked `tile_chunk` tiles at a time (cc_cosample, then
    cc_item_consensus on the current stream), so the scratch is tile_chunk * 128 KiB of
    co-sampling tiles and no n x n buffer is ever held."""
    dev = labels_nh.device
    if tile_end is None:
        tile_end = num_tiles(n)
    if tile_chunk < 1:
        raise ValueError("tile_chunk must be at least 1")
    if not isinstance(cl, torch.Tensor):
        cl = torch.from_numpy(np.array(cl, dtype=np.int32))  # a copy: the caller's may be read-only
    cl = cl.to(device=dev, dtype=torch.int32).contiguous()
    if cl.numel() != n:
        raise ValueError(f"cl must hold one cluster id per item ({n}), got {cl.numel()}")
    if S is None:
        S = torch.zeros((n, max(int(Kc), 0)), dtype=torch.int64, device=dev)
    elif (S.dtype != torch.int64 or tuple(S.shape) != (n, Kc) or not S.is_contiguous()
          or S.device != dev):
        raise ValueError("S must be a contiguous int64 [n, Kc] tensor on the labels' device")
    tb = int(tile_begin)
    while True:
        te = min(tb + int(tile_chunk), int(tile_end))
        I_tiles, _ = cosample(labels_nh, n, Hpad, tb, te, want_full=False)
        with timed("cc_item_consensus"):
            _lib.call("cc_item_consensus", labels_nh.data_ptr(), n, labels_nh.stride(0), Hpad,
                      int(K), tb, te, _lib.ptr(I_tiles) or None, cl.data_ptr(), int(Kc),
                      S.data_ptr() or None, stream_ptr())
        del I_tiles  # the caching allocator reuses it for the next chunk (same stream)
        tb = te
        if tb >= tile_end:
            break
    return S


def agreement_num_tiles(HA: int, KA: int, HB: int = None, KB: int = None) -> int:
    """Tiles of cc_agreement_sums for A against B (HB columns of KB clusters), or, with HB None,
    for A with itself (the upper triangle of tiles)."""
    sym = HB is None
    return int(_lib.load().cc_agreement_num_tiles(int(HA), int(HA if sym else HB), int(KA),
                                                  int(KA if sym else KB), int(sym)))


def _label_columns(t: torch.Tensor, n: int, H: int, name: str):
    """(tensor, row stride) of a [n, >= H] uint8 label view with unit column stride ([n] when H = 1)."""
    if t.dim() == 1:
        t = t.unsqueeze(1)
    if (t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 2 or t.shape[0] != n or t.shape[1] < H
            or (t.shape[1] > 1 and t.stride(1) != 1)):
        raise ValueError(f"{name} must be a device uint8 [n, >= H] label view with unit column stride")
    return t, (t.stride(0) if n > 1 else max(t.shape[1], 1))


def agreement_sums(A_nh: torch.Tensor, HA: int, KA: int, n: int, B_nh: torch.Tensor = None, HB: int = None,
                   KB: int = None, tile_begin: int = 0, tile_end: int = None, out: torch.Tensor = None) -> torch.Tensor:
    """int64 [HA, HB, 4] on the device: (s0, s2, r2, c2) of the contingency table N of every pair
    (column h1 of A_nh, column h2 of B_nh) over the items present in both: s0 = sum N,
    s2 = sum N^2, r2 = sum_a (sum_b N)^2, c2 = sum_b (sum_a N)^2 (post.agreement_from_sums turns
    them into the adjusted Rand or Jaccard index).  A_nh: uint8 [n, >= HA] (any row stride),
    labels in [0, KA), any other byte = absent; B_nh likewise with HB, KB ([n] for one column),
    or None: A with itself, [HA, HA, 4].  Only the pairs of tiles [tile_begin, tile_end)
    (default: all of agreement_num_tiles) are written, with plain stores, into `out` when given
    (contiguous int64 [HA, HB, 4]), else into zeros.  cc_agreement_sums on the current stream; the
    scratch is the transposed columns, (HA + HB) rounded up to 128 each times n rounded up to 128 bytes."""
    dev = A_nh.device
    sym = B_nh is None
    HA, KA, n = int(HA), int(KA), int(n)
    HB, KB = (HA, KA) if sym else (int(HB), int(KB))
    A_nh, ldA = _label_columns(A_nh, n, HA, "A_nh")
    ldB = 0
    if not sym:
        B_nh, ldB = _label_columns(B_nh, n, HB, "B_nh")
        if B_nh.device != dev:
            raise ValueError("A_nh and B_nh must be on one device")
    if out is None:
        out = torch.zeros((max(HA, 0), max(HB, 0), 4), dtype=torch.int64, device=dev)
    elif (out.dtype != torch.int64 or tuple(out.shape) != (HA, HB, 4) or not out.is_contiguous()
          or out.device != dev):
        raise ValueError("out must be a contiguous int64 [HA, HB, 4] tensor on the labels' device")
    lib = _lib.load()
    if tile_end is None:
        tile_end = int(lib.cc_agreement_num_tiles(HA, HB, KA, KB, int(sym)))
    ws = torch.empty(int(lib.cc_agreement_workspace_bytes(n, HA, 0 if sym else HB)), dtype=torch.uint8, device=dev)
    with timed("cc_agreement_sums"):
        _lib.call("cc_agreement_sums", A_nh.data_ptr(), ldA, HA, KA, None if sym else B_nh.data_ptr(), ldB, HB, KB,
                  n, int(tile_begin), int(tile_end), out.data_ptr() or None, ws.data_ptr() or None, ws.numel(),
                  stream_ptr())
    return out


def consensus(M: torch.Tensor, I: torch.Tensor) -> torch.Tensor:
    n = M.shape[0]
    C = torch.empty((n, n), dtype=torch.float32, device=M.device)
    _lib.call("cc_consensus", M.data_ptr(), I.data_ptr(), n, C.data_ptr(), stream_ptr())
    return C


LINKAGE_METHODS = {"average": 0, "complete": 1, "weighted": 2}  # CC_LINK_* (include/ccmi.h)
_CC_LINK = dict(LINKAGE_METHODS, ward=3)  # ward: euclidean distances only (the base clusterer)


def linkage_raw(D: torch.Tensor, method: str) -> torch.Tensor:
    """nn_chain's merges (x, y, distance, size) in merge order, on the device (D overwritten)."""
    assert D.dtype == torch.float64 and D.dim() == 2 and D.shape[0] == D.shape[1] and D.is_contiguous()
    n = D.shape[0]
    Z = torch.empty((n - 1, 4), dtype=torch.float64, device=D.device)
    lib = _lib.load()
    ws = torch.empty(int(lib.cc_linkage_workspace_bytes(n)), dtype=torch.uint8, device=D.device)
    _lib.call("cc_linkage_nnchain", D.data_ptr(), n, _CC_LINK[method], Z.data_ptr(), ws.data_ptr(),
              ws.numel(), stream_ptr())
    _lib.call("cc_linkage_check", ws.data_ptr(), ws.numel(), stream_ptr())
    return Z


def linkage(D: torch.Tensor, method: str) -> np.ndarray:
    """scipy.cluster.hierarchy.linkage of the symmetric float64 [n, n] distances D (device; D is
    overwritten) for method in LINKAGE_METHODS: scipy's nn_chain on the device
    (cc_linkage_nnchain), then linkage()'s stable sort of the merges by distance and its union-find
    relabelling (scipy/cluster/_hierarchy.pyx: nn_chain, label) on the host.  Returns Z [n-1, 4]."""
    n = D.shape[0]
    Z = linkage_raw(D, method)
    from .post import linkage_finish

    return linkage_finish(Z.cpu().numpy(), n)


def linkage_single(D: torch.Tensor) -> np.ndarray:
    """sklearn's single-linkage tree of the rows behind the symmetric float64 [n, n] distances D
    (device, read only): mst_linkage_core's Prim edges on the device (cc_linkage_mst), then the
    stable sort and _single_linkage_label on the host (post.single_linkage_finish).  Z [n-1, 4]."""
    assert D.dtype == torch.float64 and D.dim() == 2 and D.shape[0] == D.shape[1] and D.is_contiguous()
    n = D.shape[0]
    out = torch.empty((n - 1, 3), dtype=torch.float64, device=D.device)
    ws = torch.empty(int(_lib.load().cc_linkage_mst_workspace_bytes(n)), dtype=torch.uint8, device=D.device)
    _lib.call("cc_linkage_mst", D.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr())
    _lib.call("cc_linkage_check", ws.data_ptr(), ws.numel(), stream_ptr())
    from .post import single_linkage_finish

    return single_linkage_finish(out.cpu().numpy(), n)


def manhattan(C: torch.Tensor) -> torch.Tensor:
    """float64 [n, n] manhattan distances between the rows of the float32 [n, n] C."""
    assert C.dtype == torch.float32 and C.dim() == 2 and C.is_contiguous()
    n, d = C.shape
    D = torch.empty((n, n), dtype=torch.float64, device=C.device)
    _lib.call("cc_manhattan", C.data_ptr(), n, d, D.data_ptr(), stream_ptr())
    return D


# ---------------------------------------------------------------- hierarchical base clusterer

LINKAGE_METHODS_HC = {"average": 0, "complete": 1, "ward": 3}  # CC_LINK_* of the base clusterer

# With fewer trees than this per launch of cc_hc_nnchain_batched (one workgroup each) the
# resamples go one after the other through cc_linkage_nnchain, whose grid form spreads one tree
# over up to 128 workgroups.  Measured on the MI355X at m = 8000 (DESIGN.md K10,
# profiles/hc/hc_measure.txt): the grid form takes 171 ms a tree; a batched launch takes 168 /
# 172 / 178 / 203 ms for 1 / 4 / 16 / 64 trees.  Two trees in a launch already take half the time
# of two grid-form runs; one tree ties (168 against 171 ms) and goes to the grid form, because a
# budget that holds a single tree means a large m, where the grid form wins (n = 50 000: 1.34
# against 4.2 s).
HC_BATCH_CROSSOVER = 2


def euclidean(X: torch.Tensor) -> torch.Tensor:
    """float64 [n, n] on the device: squareform(pdist(X, 'euclidean')) bit for bit, for the
    float32 or float64 rows X [n, d] (cc_euclidean)."""
    assert X.dim() == 2 and X.is_cuda and X.is_contiguous() and X.dtype in (torch.float32, torch.float64)
    n, d = X.shape
    D = torch.empty((n, n), dtype=torch.float64, device=X.device)
    with timed("cc_euclidean"):
        _lib.call("cc_euclidean", X.data_ptr(), int(X.dtype == torch.float64), n, d, D.data_ptr(),
                  stream_ptr(X.device))
    return D


PDIST_METRICS = {"euclidean": 0, "cityblock": 1, "cosine": 2, "correlation": 3}  # CC_METRIC_* (include/ccmi.h)


def pdist(X, metric: str) -> torch.Tensor:
    """float64 [n, n] on the device: squareform(scipy.spatial.distance.pdist(X, metric)) bit for
    bit, for the float32 or float64 rows X [n, d] and metric in PDIST_METRICS (cc_pdist).

    'correlation' is scipy's own two steps: the rows less their means, X - X.mean(axis=1,
    keepdims=True) on the float64 copy of X, computed by numpy on the host (its mean is a pairwise
    sum, which the cosine code then sees rounded as numpy rounds it), then the cosine kernel on the
    float64 upload.  A device tensor X is therefore copied to the host for this metric; a numpy
    array is accepted for it too."""
    if metric not in PDIST_METRICS:
        raise ValueError(f"metric must be one of {sorted(PDIST_METRICS)}, got {metric!r}")
    if metric == "correlation":
        dev = X.device if isinstance(X, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        Xh = X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X)
        Xh = np.ascontiguousarray(Xh, dtype=np.float64)
        X = torch.from_numpy(np.ascontiguousarray(Xh - Xh.mean(axis=1, keepdims=True))).to(dev)
    assert X.dim() == 2 and X.is_cuda and X.is_contiguous() and X.dtype in (torch.float32, torch.float64)
    n, d = X.shape
    D = torch.empty((n, n), dtype=torch.float64, device=X.device)
    # the rows are centred by now, and cc_pdist knows no CC_METRIC_CORRELATION: cosine on them
    code = PDIST_METRICS["cosine" if metric == "correlation" else metric]
    norms = torch.empty(n, dtype=torch.float64, device=X.device) if code == 2 else None
    with timed("cc_pdist"):
        _lib.call("cc_pdist", X.data_ptr(), int(X.dtype == torch.float64), n, d, code, D.data_ptr(),
                  _lib.ptr(norms), stream_ptr(X.device))
    return D


def _pdist_batched(X, idx_bm, cols_bq, metric, out=None):
    """pdist_batched, and with the distances the norms [B, m] the row pass wrote (cosine and
    correlation; None otherwise)."""
    if metric not in PDIST_METRICS:
        raise ValueError(f"metric must be one of {sorted(PDIST_METRICS)}, got {metric!r}")
    assert X.dim() == 2 and X.is_cuda and X.is_contiguous() and X.dtype in (torch.float32, torch.float64)
    assert idx_bm.dtype == torch.int32 and idx_bm.dim() == 2 and idx_bm.is_contiguous() and idx_bm.is_cuda
    assert cols_bq.dtype == torch.int32 and cols_bq.dim() == 2 and cols_bq.is_contiguous() and cols_bq.is_cuda
    n, d = X.shape
    B, m = idx_bm.shape
    md = cols_bq.shape[1]
    if cols_bq.shape[0] != B or B < 1 or m < 1 or md < 1:
        raise ValueError("idx must be [B, m] and cols [B, md] with B, m and md at least 1")
    # an entry outside its range would be read out of bounds by the row pass: checked here, on
    # the device tensors, before anything is launched
    lo, hi = (int(v) for v in torch.aminmax(idx_bm))
    if lo < 0 or hi >= n:
        raise ValueError(f"idx entries must lie in [0, {n}), got [{lo}, {hi}]")
    lo, hi = (int(v) for v in torch.aminmax(cols_bq))
    if lo < 0 or hi >= d:
        raise ValueError(f"cols entries must lie in [0, {d}), got [{lo}, {hi}]")
    code = PDIST_METRICS[metric]  # cc_pdist_batched centres the rows for correlation itself
    if out is None:
        out = torch.empty((B, m, m), dtype=torch.float64, device=X.device)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == B * m * m
    ws = torch.empty(int(_lib.load().cc_pdist_batched_workspace_bytes(B, m, md, code)) // 8, dtype=torch.float64,
                     device=X.device)
    with timed("cc_pdist_batched"):
        _lib.call("cc_pdist_batched", X.data_ptr(), int(X.dtype == torch.float64), n, d, idx_bm.data_ptr(),
                  cols_bq.data_ptr(), B, m, md, code, out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                  stream_ptr(X.device))
    return out.view(B, m, m), (ws[B * m * md:].view(B, m) if code >= 2 else None)


def pdist_batched(X: torch.Tensor, idx_bm: torch.Tensor, cols_bq: torch.Tensor, metric: str,
                  out: torch.Tensor = None) -> torch.Tensor:
    """float64 [B, m, m] on the device: out[b] = squareform(scipy.spatial.distance.pdist(
    X[idx[b]][:, cols[b]], metric)) bit for bit (cc_pdist_batched), for the float32 or float64
    rows X [n, d], the int32 rows idx [B, m] and ascending columns cols [B, md] of B resamples and
    metric in PDIST_METRICS; 'correlation' is centred on the device.  An idx or cols entry
    out of range raises ValueError before the launch."""
    return _pdist_batched(X, idx_bm, cols_bq, metric, out)[0]


DEGENERATE_ZERO_NORM, DEGENERATE_NOT_FINITE = 0, 1


class DegenerateResample(ValueError):
    """A resample has a row without distances under its feature subset, or distances that are
    not finite.  code = 4 * h + kind (DEGENERATE_*): the smallest code over the ranks names the
    lowest such resample (dist.first_failure)."""

    def __init__(self, code: int, metric: str):
        self.code, self.metric = int(code), metric
        h, kind = divmod(self.code, 4)
        if kind == DEGENERATE_ZERO_NORM and metric == "cosine":
            why = "Cosine affinity cannot be used when X contains zero vectors"
        elif kind == DEGENERATE_ZERO_NORM:
            why = "a row is constant, so its correlation distances are undefined"
        else:
            why = "the distances are not all finite"
        super().__init__(f"{why} (resample {h}, metric {metric!r}, on the resample's feature subset)")


def _degenerate_code(D: torch.Tensor, norms, h_first: int):
    """The DegenerateResample code of the first tree of a batch (D [B, m, m], norms [B, m] or
    None, tree b = resample h_first + b) that has a zero norm or a distance that is not finite,
    else None.  One pass over the batch and one device-to-host read of two flags per tree: a NaN
    or an infinity anywhere in a tree reaches the tree's sum; a tree whose finite distances
    overflow the sum is told apart by the exact test, which runs for flagged trees alone."""
    bad = ~torch.isfinite(D.flatten(1).sum(dim=1))
    zero = (norms == 0).any(dim=1) if norms is not None else torch.zeros_like(bad)
    flags = torch.stack([zero, bad]).cpu().numpy()
    for b in np.flatnonzero(flags.any(axis=0)):
        if flags[0, b]:
            return 4 * (int(h_first) + int(b)) + DEGENERATE_ZERO_NORM
        if not bool(torch.isfinite(D[b]).all()):
            return 4 * (int(h_first) + int(b)) + DEGENERATE_NOT_FINITE
    return None


def hc_gather(Dfull: torch.Tensor, idx_bm: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """float64 [B, m, m]: out[b] = Dfull[idx[b]][:, idx[b]] (cc_hc_gather)."""
    assert Dfull.dtype == torch.float64 and Dfull.dim() == 2 and Dfull.is_contiguous()
    assert idx_bm.dtype == torch.int32 and idx_bm.dim() == 2 and idx_bm.is_contiguous()
    B, m = idx_bm.shape
    if out is None:
        out = torch.empty((B, m, m), dtype=torch.float64, device=Dfull.device)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == B * m * m
    with timed("cc_hc_gather"):
        _lib.call("cc_hc_gather", Dfull.data_ptr(), Dfull.shape[0], idx_bm.data_ptr(), B, m,
                  out.data_ptr(), stream_ptr(Dfull.device))
    return out.view(B, m, m)


def hc_workspace(m: int, B: int, nK: int, device) -> torch.Tensor:
    return torch.empty(int(_lib.load().cc_hc_workspace_bytes(int(m), int(B), int(nK))), dtype=torch.uint8,
                       device=device)


def hc_nnchain_batched(Db: torch.Tensor, method: str, ws: torch.Tensor = None) -> torch.Tensor:
    """nn_chain's raw merges [B, m-1, 4] (x, y, distance, size in merge order) of the B trees over
    the symmetric float64 [B, m, m] distances Db (overwritten): cc_hc_nnchain_batched, then
    cc_hc_check, which raises when a tree's status word is set."""
    assert Db.dtype == torch.float64 and Db.dim() == 3 and Db.shape[1] == Db.shape[2] and Db.is_contiguous()
    B, m, _ = Db.shape
    if ws is None:
        ws = hc_workspace(m, B, 0, Db.device)
    Z = torch.empty((B, m - 1, 4), dtype=torch.float64, device=Db.device)
    with timed("cc_hc_nnchain_batched"):
        _lib.call("cc_hc_nnchain_batched", Db.data_ptr(), B, m, LINKAGE_METHODS_HC[method], Z.data_ptr(),
                  ws.data_ptr(), ws.numel(), stream_ptr(Db.device))
    _lib.call("cc_hc_check", ws.data_ptr(), B, stream_ptr(Db.device))
    return Z


def hc_cut(Z: torch.Tensor, idx_bm: torch.Tensor, Ks_d: torch.Tensor, h_begin: int, labels: torch.Tensor,
           ws: torch.Tensor = None):
    """labels[k, idx[b, r], h_begin + b] = the cluster of leaf r in the Ks[k]-cluster cut of tree b
    (cc_hc_cut), from the raw merges Z [B, m-1, 4]; the merges' stable ranks by distance come
    from torch.sort on the batch.  labels: uint8 [nK, n, Hpad] contiguous."""
    B, m1, _ = Z.shape
    m = m1 + 1
    assert Z.dtype == torch.float64 and Z.is_contiguous()
    assert idx_bm.dtype == torch.int32 and tuple(idx_bm.shape) == (B, m) and idx_bm.is_contiguous()
    assert Ks_d.dtype == torch.int32 and Ks_d.is_cuda and Ks_d.is_contiguous()
    nK = Ks_d.numel()
    assert labels.dtype == torch.uint8 and labels.dim() == 3 and labels.is_contiguous() and labels.shape[0] == nK
    if ws is None:
        ws = hc_workspace(m, B, nK, Z.device)
    with timed("cc_hc_cut"):
        order = torch.sort(Z[:, :, 2], dim=1, stable=True).indices
        rank = torch.empty((B, m1), dtype=torch.int32, device=Z.device)
        rank.scatter_(1, order, torch.arange(m1, dtype=torch.int32, device=Z.device).expand(B, m1))
        _lib.call("cc_hc_cut", Z.data_ptr(), rank.data_ptr(), idx_bm.data_ptr(), B, m, Ks_d.data_ptr(), nK,
                  int(h_begin), labels.data_ptr(), labels.shape[1], labels.shape[2], ws.data_ptr(), ws.numel(),
                  stream_ptr(Z.device))


def hc_tree_bytes(m: int, nK: int) -> int:
    """Device bytes one tree of a batch needs: its m x m float64 distances, its merges and their
    sort (values, indices, ranks), the chain state and the cut's links (cc_hc_workspace_bytes)."""
    m, nK = int(m), int(nK)
    return 8 * m * m + (32 + 8 + 8 + 4) * (m - 1) + 8 * m + 4 * nK * m + 512  # 512: status word, alignment


def hc_feature_bytes(m: int, md: int) -> int:
    """Device bytes one tree of a batch needs on top of hc_tree_bytes under feature subsampling:
    its compact float64 rows [m, md], their norms and its column indices."""
    return 8 * int(m) * int(md) + 8 * int(m) + 4 * int(md)


def _trees_per_batch(per: int, n: int, m: int, nh: int, budget: int, md, who: str) -> int:
    """min(nh, the trees of `per` bytes each that fit the budget next to the n x n distances);
    with md (feature subsampling) there is no n x n matrix and a tree needs hc_feature_bytes more.
    Raises when not one tree fits."""
    if md is not None:
        per += hc_feature_bytes(m, md)
        fit = int(budget) // per
        if fit < 1:
            raise ValueError(
                f"workspace_budget = {int(budget)} bytes cannot hold the {who} clusterer: one tree "
                f"of m = {int(m)} over {int(md)} features ({per} bytes) is needed")
    else:
        fit = (int(budget) - 8 * int(n) * int(n)) // per
        if fit < 1:
            raise ValueError(
                f"workspace_budget = {int(budget)} bytes cannot hold the {who} clusterer: the n x n "
                f"float64 distances ({8 * int(n) * int(n)} bytes) and one tree of m = {int(m)} "
                f"({per} bytes) are needed")
    return max(1, min(int(nh), int(fit)))


def hc_plan(n: int, m: int, nh: int, nK: int, budget: int, md: int = None):
    """(B, route) for the nh resamples of a rank: B = min(nh, (budget - 8 n^2) // bytes per tree)
    trees per launch; route 'batched' (cc_hc_nnchain_batched on B trees) or 'sequential' (one
    tree at a time through cc_linkage_nnchain, grid form for large m) when the budget holds fewer
    trees than HC_BATCH_CROSSOVER and fewer than the rank has.  Raises when the n x n distances
    and one tree do not fit the budget.

    md (feature subsampling: every tree computes its own distances from md columns,
    cc_pdist_batched): there is no n x n matrix, so the budget holds no 8 n^2 term, and a tree
    needs hc_feature_bytes(m, md) more."""
    B = _trees_per_batch(hc_tree_bytes(m, nK), n, m, nh, budget, md, "hierarchical")
    route = 'sequential' if B < min(int(nh), HC_BATCH_CROSSOVER) else 'batched'
    return B, route


def _resample_batches(Dfull, idx_d, h0, h1, B, X=None, cols_d=None, metric=None):
    """(a, rows, D) for the resamples [a, a + len(rows)) of [h0, h1), B at a time: rows = idx_d's
    rows and D [len(rows), m, m] their distances in one buffer that every batch reuses, gathered
    from Dfull (cc_hc_gather) or, with Dfull None, computed from each resample's own columns
    (cc_pdist_batched), where a batch that holds a degenerate resample raises DegenerateResample
    before it is handed out."""
    m = idx_d.shape[1]
    dev = X.device if Dfull is None else Dfull.device
    Db = torch.empty((B, m, m), dtype=torch.float64, device=dev)
    for a in range(h0, h1, B):
        b = min(a + B, h1)
        rows = idx_d[a:b].contiguous()
        if Dfull is None:
            D, norms = _pdist_batched(X, rows, cols_d[a:b].contiguous(), metric, out=Db[:b - a])
            code = _degenerate_code(D, norms, a)
            if code is not None:
                raise DegenerateResample(code, metric)
        else:
            D = hc_gather(Dfull, rows, out=Db[:b - a])
        yield a, rows, D


def hc_labels(Dfull: torch.Tensor, idx_d: torch.Tensor, h0: int, h1: int, Ks, method: str,
              labels: torch.Tensor, budget: int = None, route: str = 'auto', X: torch.Tensor = None,
              cols_d: torch.Tensor = None, metric: str = None) -> dict:
    """Fill labels[k, idx[h, r], h] for h in [h0, h1) and every K of Ks with the K-cluster cut of
    the `method` tree over Dfull[idx[h]][:, idx[h]] (AgglomerativeClustering.fit_predict of every
    (h, K), one tree per h).  idx_d: int32 [H, m] on the device.  budget: device bytes for Dfull
    and the trees (default: half the free memory plus Dfull, which exists already).  Returns the
    plan that ran: dict(route, batch, launches).

    Feature subsampling: Dfull None, and X [n, d] (device), cols_d int32 [H, md] (device, indexed
    by the global h like idx_d) and `metric` instead.  Tree h is then built over
    pdist(X[idx[h]][:, cols[h]], metric), computed per batch (cc_pdist_batched); budget: device
    bytes for the trees alone (default: half the free memory).  A resample with a row without
    distances under its columns, or with distances that are not finite, raises
    DegenerateResample for the first such h of the range, before that batch's trees."""
    feature = Dfull is None
    if feature:
        if X is None or cols_d is None or metric is None:
            raise ValueError("without Dfull, hc_labels needs X, cols_d and metric")
        n, dev, md = X.shape[0], X.device, cols_d.shape[1]
    else:
        n, dev, md = Dfull.shape[0], Dfull.device, None
    m = idx_d.shape[1]
    nh = h1 - h0
    nK = len(Ks)
    if budget is None:
        budget = (0 if feature else 8 * n * n) + torch.cuda.mem_get_info(dev)[0] // 2
    B, planned = hc_plan(n, m, max(nh, 1), nK, budget, md=md)
    if route == 'auto':
        route = planned
    if route not in ('batched', 'sequential'):
        raise ValueError("route must be 'auto', 'batched' or 'sequential'")
    if route == 'sequential':
        B = 1
    stats = dict(route=route, batch=B, launches=0)
    if feature:
        stats['feature_subsampling'] = md
    if nh <= 0 or nK == 0:
        return stats
    Ks_d = torch.tensor([int(K) for K in Ks], dtype=torch.int32, device=dev)
    ws = hc_workspace(m, B, nK, dev)
    for a, rows, D in _resample_batches(Dfull, idx_d, h0, h1, B, X, cols_d, metric):
        if route == 'batched':
            Z = hc_nnchain_batched(D, method, ws)
        else:
            with timed("cc_linkage_nnchain"):
                Z = linkage_raw(D[0], method).unsqueeze(0)
        hc_cut(Z, rows, Ks_d, a, labels, ws)
        stats['launches'] += 1
    return stats


# ---------------------------------------------------------------- PAM base clusterer

def pam_tree_bytes(m: int, nK: int, Kmax: int) -> int:
    """Device bytes one tree of a PAM batch needs: its m x m float64 distances, the BUILD state
    (score, near, medoid flags, the chain) and per K the SWAP state (near and second in item and
    in slot order, the best dTD per candidate, slots, the grouping, its medoids and segment
    offsets); cc_pam_workspace_bytes plus the distances."""
    m, nK, Kmax = int(m), int(nK), int(Kmax)
    per_k = (5 * 8 + 3 * 4) * m + 4 * (2 * Kmax + 1) + 8
    return 8 * m * m + (8 + 8 + 4) * m + 4 * Kmax + nK * per_k + 256 * (6 + 12)  # 256: alignment of each part


def pam_plan(n: int, m: int, nh: int, nK: int, Kmax: int, budget: int, md: int = None) -> int:
    """B = min(nh, (budget - 8 n^2) // bytes per tree) trees per batch for the nh resamples of a
    rank, as hc_plan counts them (md: feature subsampling, no n x n matrix, hc_feature_bytes more
    per tree).  Raises when the distances and one tree do not fit the budget."""
    return _trees_per_batch(pam_tree_bytes(m, nK, Kmax), n, m, nh, budget, md, "PAM")


def pam_batch(D: torch.Tensor, rows: torch.Tensor, Ks_d: torch.Tensor, Kmax: int, h_begin: int,
              labels: torch.Tensor, max_iter: int = 300, inertia: torch.Tensor = None,
              n_iter: torch.Tensor = None, medoids: torch.Tensor = None, ws: torch.Tensor = None) -> int:
    """PAM of every (tree b, K) over the distances D [B, m, m] (float64, device, read only):
    cc_pam_build, then cc_pam_swap_step until cc_pam_active reads 0 or max_iter iterations ran,
    then cc_pam_labels into labels[k, rows[b, r], h_begin + b] (uint8 [nK, n, Hpad]), inertia and
    n_iter ([nK, H], at column h_begin + b) and medoids (int32 [B, nK, Kmax], ascending, -1 padded).
    Ks_d: int32 [nK] on the device, every K in [1, Kmax], Kmax <= min(m, 127).  Returns the number
    of SWAP iterations launched."""
    assert D.dtype == torch.float64 and D.dim() == 3 and D.shape[1] == D.shape[2] and D.is_contiguous()
    B, m, _ = D.shape
    nK = Ks_d.numel()
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (B, m) and rows.is_contiguous()
    assert Ks_d.dtype == torch.int32 and Ks_d.is_cuda and Ks_d.is_contiguous()
    assert labels.dtype == torch.uint8 and labels.dim() == 3 and labels.is_contiguous() and labels.shape[0] == nK
    ldo = 0
    for t, dt in ((inertia, torch.float64), (n_iter, torch.int32)):
        if t is not None:
            assert t.dtype == dt and t.dim() == 2 and t.shape[0] == nK and t.is_contiguous()
            ldo = t.shape[1]
    if inertia is not None and n_iter is not None:
        assert inertia.shape == n_iter.shape
    if medoids is not None:
        assert medoids.dtype == torch.int32 and tuple(medoids.shape) == (B, nK, Kmax) and medoids.is_contiguous()
    dev = D.device
    if ws is None:
        ws = pam_workspace(m, B, nK, Kmax, dev)
    st = stream_ptr(dev)
    with timed("cc_pam_build"):
        _lib.call("cc_pam_build", D.data_ptr(), B, m, Ks_d.data_ptr(), nK, int(Kmax), ws.data_ptr(), ws.numel(), st)
    iterations = 0
    active = ctypes.c_int(0)
    with timed("cc_pam_swap"):
        while iterations < int(max_iter):
            _lib.call("cc_pam_swap_step", D.data_ptr(), B, m, Ks_d.data_ptr(), nK, int(Kmax), int(max_iter),
                      ws.data_ptr(), ws.numel(), st)
            _lib.call("cc_pam_active", ws.data_ptr(), ctypes.addressof(active), st)
            iterations += 1
            if active.value == 0:
                break
    with timed("cc_pam_labels"):
        _lib.call("cc_pam_labels", D.data_ptr(), rows.data_ptr(), B, m, Ks_d.data_ptr(), nK, int(Kmax), int(h_begin),
                  labels.data_ptr(), labels.shape[1], labels.shape[2], _lib.ptr(inertia), _lib.ptr(n_iter), ldo,
                  _lib.ptr(medoids), ws.data_ptr(), ws.numel(), st)
    return iterations


def pam_workspace(m: int, B: int, nK: int, Kmax: int, device) -> torch.Tensor:
    nbytes = int(_lib.load().cc_pam_workspace_bytes(int(m), int(B), int(nK), int(Kmax)))
    if nbytes == 0:
        raise ValueError(f"PAM on the device needs 1 <= K <= min(m, 127), m <= 65535 and at most 65535 trees a "
                         f"batch, got m = {m}, B = {B}, nK = {nK}, max K = {Kmax}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def pam_labels(Dfull: torch.Tensor, idx_d: torch.Tensor, h0: int, h1: int, Ks, labels: torch.Tensor,
               budget: int = None, max_iter: int = 300, X: torch.Tensor = None, cols_d: torch.Tensor = None,
               metric: str = None, inertia: torch.Tensor = None, n_iter: torch.Tensor = None) -> dict:
    """Fill labels[k, idx[h, r], h] for h in [h0, h1) and every K of Ks with PAM(n_clusters=K,
    max_iter=max_iter) over Dfull[idx[h]][:, idx[h]] (one BUILD chain per h serves every K).
    Arguments as hc_labels, feature subsampling (Dfull None; X, cols_d, metric) and
    DegenerateResample included; inertia / n_iter: optional [nK, H] device tensors filled at the
    columns [h0, h1).  Returns dict(route='batched', batch, launches, swap_iterations)."""
    feature = Dfull is None
    if feature:
        if X is None or cols_d is None or metric is None:
            raise ValueError("without Dfull, pam_labels needs X, cols_d and metric")
        n, dev, md = X.shape[0], X.device, cols_d.shape[1]
    else:
        n, dev, md = Dfull.shape[0], Dfull.device, None
    m = idx_d.shape[1]
    nh = h1 - h0
    Ks = [int(K) for K in Ks]
    nK = len(Ks)
    Kmax = max(Ks) if Ks else 1
    if budget is None:
        budget = (0 if feature else 8 * n * n) + torch.cuda.mem_get_info(dev)[0] // 2
    B = pam_plan(n, m, max(nh, 1), nK, Kmax, budget, md=md)
    stats = dict(route='batched', batch=B, launches=0, swap_iterations=0)
    if feature:
        stats['feature_subsampling'] = md
    if nh <= 0 or nK == 0:
        return stats
    if min(Ks) < 1 or Kmax > m:
        raise ValueError(f"every K must lie in [1, m = {m}], got {Ks}")
    Ks_d = torch.tensor(Ks, dtype=torch.int32, device=dev)
    ws = pam_workspace(m, B, nK, Kmax, dev)
    for a, rows, D in _resample_batches(Dfull, idx_d, h0, h1, B, X, cols_d, metric):
        stats['swap_iterations'] += pam_batch(D, rows, Ks_d, Kmax, a, labels, max_iter, inertia, n_iter, ws=ws)
        stats['launches'] += 1
    return stats


# ---------------------------------------------------------------- GMM base clusterer

class IllDefinedMixture(ValueError):
    """A mixture problem met a variance that is not positive, or a covariance whose Cholesky
    factorisation met a pivot that is not: sklearn's refusal, in its words."""

    def __init__(self):
        from .gmm import _ILL_DEFINED

        super().__init__(_ILL_DEFINED)


def _up256(v: int) -> int:
    return (int(v) + 255) & ~255


def _rows_bytes(m: int, md: int, Ks, doubles) -> int:
    """Device bytes one resample of a row batch needs: its compact float64 rows [m, md], its row and
    column indices and per K the arrays of the problem, doubles(K, Kp) float64 values (Kp = K
    rounded up to 16) rounded up to 256 bytes, and its 48-byte state."""
    per = 8 * m * md + 4 * m + 4 * md
    for K in Ks:
        per += _up256(8 * doubles(int(K), (int(K) + 15) & ~15)) + 64
    return per


def _plan_rows(per: int, fixed: int, nh: int, nK: int, budget: int, who: str, m: int, md: int) -> int:
    """min(nh, the resamples of `per` bytes each that fit the budget next to `fixed` bytes), at most
    65535 problems a launch.  Raises when one resample does not fit."""
    fit = (int(budget) - fixed) // per
    if fit < 1:
        raise ValueError(
            f"workspace_budget = {int(budget)} bytes cannot hold the {who} clusterer: one resample "
            f"of m = {int(m)} over {int(md)} features ({per + fixed} bytes) is needed")
    return max(1, min(int(nh), int(fit), 65535 // nK))


def _scalar_outputs(nK: int, labels: torch.Tensor, *outputs) -> int:
    """ldo, the row length that the [nK, H] output tensors of (tensor or None, dtype) pairs share
    (0 when all are None), after the asserts on them and on the label matrix [nK, n, Hpad]."""
    assert labels.dtype == torch.uint8 and labels.dim() == 3 and labels.is_contiguous() and labels.shape[0] == nK
    ldo = 0
    for t, dt in outputs:
        if t is not None:
            assert t.dtype == dt and t.dim() == 2 and t.shape[0] == nK and t.is_contiguous()
            assert ldo in (0, t.shape[1])
            ldo = t.shape[1]
    return ldo


def _row_batches(X64, idx_d, cols_d, h0, h1, B):
    """(a, rows, cols_b, Xb) for the resamples [a, a + len(rows)) of [h0, h1), B at a time: rows and
    cols_b (None without cols_d) = the rows of idx_d and cols_d, and Xb [len(rows), m, md] =
    X64[rows[b]][:, cols_b[b]] (cc_gmm_gather) in one buffer that every batch reuses.  A batch with
    an index outside its range raises ValueError before anything is launched for it."""
    assert X64.dtype == torch.float64 and X64.dim() == 2 and X64.is_contiguous() and X64.is_cuda
    assert idx_d.dtype == torch.int32 and idx_d.dim() == 2
    n, d = X64.shape
    m = idx_d.shape[1]
    md = d if cols_d is None else cols_d.shape[1]
    st = stream_ptr(X64.device)
    buf = torch.empty((B, m, md), dtype=torch.float64, device=X64.device)
    for a in range(h0, h1, B):
        rows = idx_d[a:min(a + B, h1)].contiguous()
        nb = rows.shape[0]
        # an entry outside its range would be read out of bounds by the gather: checked here, on the
        # device tensors, before anything is launched
        lo, hi = (int(v) for v in torch.aminmax(rows))
        if lo < 0 or hi >= n:
            raise ValueError(f"idx entries must lie in [0, {n}), got [{lo}, {hi}]")
        cols_b = None
        if cols_d is not None:
            cols_b = cols_d[a:a + nb].contiguous()
            assert cols_b.dtype == torch.int32 and cols_b.dim() == 2 and cols_b.shape[0] == nb
            lo, hi = (int(v) for v in torch.aminmax(cols_b))
            if lo < 0 or hi >= d:
                raise ValueError(f"cols entries must lie in [0, {d}), got [{lo}, {hi}]")
        Xb = buf[:nb]
        with timed("cc_gmm_gather"):
            _lib.call("cc_gmm_gather", X64.data_ptr(), n, d, rows.data_ptr(), _lib.ptr(cols_b), nb, m, md,
                      Xb.data_ptr(), st)
        yield a, rows, cols_b, Xb


def _rows_call(X64, idx_d, cols_d, h0, h1, Ks, budget):
    """(m, md, nh, Ks as ints, budget) of a *_labels call over rows; budget None: half the free memory."""
    if budget is None:
        budget = torch.cuda.mem_get_info(X64.device)[0] // 2
    md = X64.shape[1] if cols_d is None else cols_d.shape[1]
    return idx_d.shape[1], md, h1 - h0, [int(K) for K in Ks], budget


def gmm_bytes(m: int, md: int, Ks) -> int:
    """Device bytes one resample of a GMM batch needs: its compact float64 rows [m, md], its row and
    column indices and per K (Kp = K rounded up to 16) the responsibilities [m, Kp], the M-step
    sums [Kp, 2 md + 1], the E-step's operand image [Kp, 2 md], three constants per component, the
    16-row tile sums and the problem's 48-byte state: cc_gmm_workspace_bytes plus the rows."""
    m, md = int(m), int(md)
    return _rows_bytes(m, md, Ks, lambda K, Kp: m * Kp + Kp * (2 * md + 1) + Kp * 2 * md + 3 * Kp + (m + 15) // 16)


GMM_FULL_MD_MAX = 128  # the most features of the full-covariance kernels (csrc/gmm_full.hip)


def gmm_full_bytes(m: int, md: int, Ks) -> int:
    """gmm_bytes for the full-covariance model: next to the rows, the indices and per K the
    responsibilities [m, Kp], the M-step sums [Kp, md + 1], the means [Kp, md], the factors
    [K, md, md] (each covariance's lower triangle, then its precision factor in place), mu P
    [Kp, md], three constants per component, the 16-row tile sums and the state:
    cc_gmm_full_workspace_bytes plus the rows."""
    m, md = int(m), int(md)
    return _rows_bytes(m, md, Ks, lambda K, Kp: (m * Kp + Kp * (md + 1) + Kp * md + K * md * md + Kp * md + 3 * Kp
                                                 + (m + 15) // 16))


def gmm_plan(n: int, m: int, nh: int, Ks, md: int, budget: int, covariance: str = 'diag') -> int:
    """B = the resamples per batch for the nh resamples of a rank: as many as fit the budget next
    to the init label matrix (uint8 [nK, n, B rounded up to 128]: nK * n bytes a resample and 127
    columns of rounding), at most nh and at most 65535 problems a launch.  Raises when one
    resample does not fit."""
    nK = max(len(Ks), 1)
    per = (gmm_full_bytes if covariance == 'full' else gmm_bytes)(m, md, Ks) + nK * int(n)
    return _plan_rows(per, 1024 + 127 * nK * int(n), nh, nK, budget, "GMM", m, md)


def gmm_full_plan(n: int, m: int, nh: int, Ks, md: int, budget: int) -> int:
    """gmm_plan for the full-covariance model."""
    return gmm_plan(n, m, nh, Ks, md, budget, 'full')


def _gmm_entry(covariance: str, name: str) -> str:
    """The entry point `name` (workspace_bytes, start, em_step, finish) of the covariance type."""
    if covariance not in ('diag', 'full'):
        raise ValueError(f"covariance must be 'diag' or 'full', got {covariance!r}")
    return ("cc_gmm_full_" if covariance == 'full' else "cc_gmm_") + name


def gmm_workspace(m: int, md: int, B: int, Ks_h: np.ndarray, device, covariance: str = 'diag') -> torch.Tensor:
    fn = getattr(_lib.load(), _gmm_entry(covariance, "workspace_bytes"))
    nbytes = int(fn(int(m), int(md), int(B), Ks_h.ctypes.data, len(Ks_h)))
    if nbytes == 0:
        limit = f", at most {GMM_FULL_MD_MAX} features" if covariance == 'full' else ""
        raise ValueError(f"GMM on the device needs 1 <= K <= min(m, 127), at most 127 values of K{limit} and at most "
                         f"65535 problems a batch, got m = {m}, md = {md}, B = {B}, Ks = {Ks_h.tolist()}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def gmm_batch(X64, rows, cols_b, Xb, Ks_h, h_begin, labels, ws, n_init, seed, tol, reg_covar, max_iter,
              lower_bound, n_iter, converged, ldo, budget, covariance) -> int:
    """One batch of gmm_labels, (a, rows, cols_b, Xb) of _row_batches: per init the k-means labels
    of the float64 engine (BatchedKMeans.run_f64 with kpp_init = (init, n_init)), cc_gmm_start (cc_gmm_full_start under covariance 'full', and so on),
    cc_gmm_em_step until cc_gmm_active reads 0 or max_iter iterations ran, and cc_gmm_finish into
    labels[k, rows[b, r], h_begin + b] and lower_bound / n_iter / converged ([nK, ldo], at column
    h_begin + b) where the init is the best so far.  budget: the workspace budget of the k-means
    fits.  Returns the EM iterations launched; raises IllDefinedMixture as sklearn does."""
    from .kmeans import BatchedKMeans

    n = X64.shape[0]
    B, m, md = Xb.shape
    start, em_step, finish = (_gmm_entry(covariance, name) for name in ("start", "em_step", "finish"))
    st = stream_ptr(X64.device)
    shape = (B, m, md, Ks_h.ctypes.data, len(Ks_h))
    lab = torch.empty((len(Ks_h), n, pad_h(B)), dtype=torch.uint8, device=X64.device)  # each init's k-means labels
    iterations = 0
    active, failed = ctypes.c_int(0), ctypes.c_int(0)
    for init in range(int(n_init)):
        with timed("gmm_kmeans_init"):
            bk = BatchedKMeans([int(K) for K in Ks_h], n_init=1, max_iter=300, tol=1e-4, random_state=seed,
                               workspace_budget=budget)
            bk.run_f64(X64, rows, n, B, m, 0, B, lab, cols_d=cols_b, kpp_init=(init, int(n_init)))
        with timed("cc_gmm_start"):
            _lib.call(start, Xb.data_ptr(), rows.data_ptr(), *shape, lab.data_ptr(), n, lab.shape[2], 0,
                      float(reg_covar), ws.data_ptr(), ws.numel(), st)
        with timed("cc_gmm_em"):
            for _ in range(int(max_iter)):
                _lib.call(em_step, Xb.data_ptr(), *shape, float(tol), float(reg_covar), int(max_iter),
                          ws.data_ptr(), ws.numel(), st)
                _lib.call("cc_gmm_active", ws.data_ptr(), ctypes.addressof(active), ctypes.addressof(failed), st)
                iterations += 1
                if active.value == 0:
                    break
        if failed.value:
            raise IllDefinedMixture()
        with timed("cc_gmm_finish"):
            _lib.call(finish, Xb.data_ptr(), rows.data_ptr(), *shape, int(init > 0), int(h_begin),
                      labels.data_ptr(), labels.shape[1], labels.shape[2], _lib.ptr(lower_bound), _lib.ptr(n_iter),
                      _lib.ptr(converged), ldo, ws.data_ptr(), ws.numel(), st)
    return iterations


def gmm_labels(X64: torch.Tensor, idx_d: torch.Tensor, h0: int, h1: int, Ks, labels: torch.Tensor,
               budget: int = None, n_init: int = 1, seed: int = 0, tol: float = 1e-3, reg_covar: float = 1e-6,
               max_iter: int = 100, cols_d: torch.Tensor = None, lower_bound: torch.Tensor = None,
               n_iter: torch.Tensor = None, converged: torch.Tensor = None, covariance: str = 'diag') -> dict:
    """Fill labels[k, idx[h, r], h] for h in [h0, h1) and every K of Ks with GMM(n_components=K, ...)
    (covariance 'diag') or FullGMM(n_components=K, ...) ('full': the cc_gmm_full_ entry points,
    md <= 128), with n_init, random_state=seed, tol, reg_covar and max_iter,
    over X64[idx[h]] (float64 [n, d], device), under feature subsampling over X64[idx[h]][:, cols[h]]
    (cols_d int32 [H, md], device, indexed by the global h like idx_d).  budget: device bytes for the
    batches (default: half the free memory); lower_bound / n_iter / converged: optional [nK, H]
    device tensors filled at the columns [h0, h1).  Returns dict(route='batched', batch, launches,
    em_iterations, inits)."""
    n, dev = X64.shape[0], X64.device
    m, md, nh, Ks, budget = _rows_call(X64, idx_d, cols_d, h0, h1, Ks, budget)
    _gmm_entry(covariance, "start")
    B = gmm_plan(n, m, max(nh, 1), Ks, md, budget, covariance)
    stats = dict(route='batched', batch=B, launches=0, em_iterations=0, inits=int(n_init))
    if cols_d is not None:
        stats['feature_subsampling'] = md
    if nh <= 0 or not Ks:
        return stats
    if min(Ks) < 1 or max(Ks) > m:
        raise ValueError(f"every K must lie in [1, m = {m}], got {Ks}")
    Ks_h = np.ascontiguousarray(np.asarray(Ks, dtype=np.int32))
    ldo = _scalar_outputs(len(Ks), labels, (lower_bound, torch.float64), (n_iter, torch.int32),
                          (converged, torch.uint8))
    ws = gmm_workspace(m, md, B, Ks_h, dev, covariance)
    for a, rows, cols_b, Xb in _row_batches(X64, idx_d, cols_d, h0, h1, B):
        stats['em_iterations'] += gmm_batch(X64, rows, cols_b, Xb, Ks_h, a, labels, ws, n_init, seed, tol,
                                            reg_covar, max_iter, lower_bound, n_iter, converged, ldo, budget,
                                            covariance)
        stats['launches'] += 1
    return stats


# ---------------------------------------------------------------- NMF base clusterer

def nmf_bytes(m: int, md: int, Ks) -> int:
    """Device bytes one resample of an NMF batch needs: its compact float64 rows [m, md], its row and
    column indices and per K (Kp = K rounded up to 16) W [m, Kp], H and W^T X [Kp, md] each, H H^T
    and W^T W [Kp, Kp] each, the 16-row tile sums of the error and the problem's 48-byte state:
    cc_nmf_workspace_bytes plus the rows."""
    m, md = int(m), int(md)
    return _rows_bytes(m, md, Ks, lambda K, Kp: m * Kp + 2 * Kp * md + 2 * Kp * Kp + (m + 15) // 16)


def nmf_plan(n: int, m: int, nh: int, Ks, md: int, budget: int, n_init: int = 1) -> int:
    """B = the resamples per batch for the nh resamples of a rank: as many as fit the budget next
    to the normals of every init (float64, (m + md) * sum(Ks) values an init, shared by the
    resamples), at most nh and at most 65535 problems a launch.  Raises when one resample does not
    fit."""
    fixed = 1024 + 8 * int(n_init) * (int(m) + int(md)) * sum(int(K) for K in Ks)
    return _plan_rows(nmf_bytes(m, md, Ks), fixed, nh, max(len(Ks), 1), budget, "NMF", m, md)


def nmf_workspace(m: int, md: int, B: int, Ks_h: np.ndarray, device) -> torch.Tensor:
    nbytes = int(_lib.load().cc_nmf_workspace_bytes(int(m), int(md), int(B), Ks_h.ctypes.data, len(Ks_h)))
    if nbytes == 0:
        raise ValueError(f"NMF on the device needs 1 <= K <= 127, at most 127 values of K and at most 65535 problems "
                         f"a batch, got m = {m}, md = {md}, B = {B}, Ks = {Ks_h.tolist()}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def nmf_normals(seed: int, m: int, md: int, Ks, n_init: int, device):
    """The absolute normals of every init on the device: per K one RandomState(seed) and per init
    |N_H| [K, md] drawn first, then |N_W| [m, K] (nmf.init_normals).  Returns (W, H): float64
    [n_init, m * sum(Ks)] and [n_init, md * sum(Ks)], the values of each K concatenated."""
    from .nmf import init_normals

    Ws = [[] for _ in range(int(n_init))]
    Hs = [[] for _ in range(int(n_init))]
    for K in Ks:
        rs = np.random.RandomState(seed)
        for i in range(int(n_init)):
            W, H = init_normals(rs, int(m), int(md), int(K))
            Ws[i].append(W.ravel())
            Hs[i].append(H.ravel())
    W = torch.from_numpy(np.stack([np.concatenate(w) for w in Ws])).to(device)
    H = torch.from_numpy(np.stack([np.concatenate(h) for h in Hs])).to(device)
    return W.contiguous(), H.contiguous()


NMF_TEST_EVERY = 10  # sklearn's stopping test runs at the iterations that are multiples of 10


def nmf_batch(rows, Xb, Ks_h, h_begin, labels, normals, ws, tol, max_iter, reconstruction_err, n_iter, converged,
              ldo) -> int:
    """One batch of nmf_labels, (a, rows, _, Xb) of _row_batches, from normals = nmf_normals(...),
    whose first extent is n_init: per init cc_nmf_start, cc_nmf_steps ten iterations a call until
    cc_gmm_active reads 0 (one synchronisation per stopping test), and cc_nmf_finish into
    labels[k, rows[b, r], h_begin + b] and reconstruction_err / n_iter / converged ([nK, ldo], at
    column h_begin + b) where the init is the best so far.  Returns the iterations launched."""
    B, m, md = Xb.shape
    NW, NH = normals
    sumK = int(Ks_h.sum())
    for t, width in ((NW, m * sumK), (NH, md * sumK)):
        assert t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == width and t.is_contiguous() and t.is_cuda
    st = stream_ptr(Xb.device)
    shape = (B, m, md, Ks_h.ctypes.data, len(Ks_h))
    iterations = 0
    active, failed = ctypes.c_int(0), ctypes.c_int(0)
    max_iter = int(max_iter)
    for init in range(NW.shape[0]):
        with timed("cc_nmf_start"):
            _lib.call("cc_nmf_start", Xb.data_ptr(), *shape, NW[init].data_ptr(), NH[init].data_ptr(), ws.data_ptr(),
                      ws.numel(), st)
        with timed("cc_nmf_steps"):
            first = 1
            while first <= max_iter:
                # up to the next stopping test, or to max_iter where there is none (tol = 0)
                count = min(NMF_TEST_EVERY, max_iter - first + 1) if tol > 0 else max_iter - first + 1
                _lib.call("cc_nmf_steps", Xb.data_ptr(), *shape, first, count, float(tol), max_iter, ws.data_ptr(),
                          ws.numel(), st)
                first += count
                iterations += count
                _lib.call("cc_gmm_active", ws.data_ptr(), ctypes.addressof(active), ctypes.addressof(failed), st)
                if active.value == 0:
                    break
        with timed("cc_nmf_finish"):
            _lib.call("cc_nmf_finish", Xb.data_ptr(), rows.data_ptr(), *shape, int(init > 0), int(h_begin),
                      labels.data_ptr(), labels.shape[1], labels.shape[2], _lib.ptr(reconstruction_err),
                      _lib.ptr(n_iter), _lib.ptr(converged), ldo, ws.data_ptr(), ws.numel(), st)
    return iterations


def nmf_labels(X64: torch.Tensor, idx_d: torch.Tensor, h0: int, h1: int, Ks, labels: torch.Tensor,
               budget: int = None, n_init: int = 1, seed: int = 0, tol: float = 1e-4, max_iter: int = 200,
               cols_d: torch.Tensor = None, reconstruction_err: torch.Tensor = None, n_iter: torch.Tensor = None,
               converged: torch.Tensor = None) -> dict:
    """Fill labels[k, idx[h, r], h] for h in [h0, h1) and every K of Ks with NMF(n_components=K,
    n_init, random_state=seed, tol, max_iter) over X64[idx[h]] (float64 [n, d], non-negative, device),
    under feature subsampling over X64[idx[h]][:, cols[h]] (cols_d int32 [H, md], device, indexed by
    the global h like idx_d).  The normals come from numpy on the host and are uploaded once per
    call.  budget: device bytes for the batches (default: half the free memory);
    reconstruction_err / n_iter / converged: optional [nK, H] device tensors filled at the columns
    [h0, h1).  Returns dict(route='batched', batch, launches, iterations, inits)."""
    n, dev = X64.shape[0], X64.device
    m, md, nh, Ks, budget = _rows_call(X64, idx_d, cols_d, h0, h1, Ks, budget)
    B = nmf_plan(n, m, max(nh, 1), Ks, md, budget, n_init)
    stats = dict(route='batched', batch=B, launches=0, iterations=0, inits=int(n_init))
    if cols_d is not None:
        stats['feature_subsampling'] = md
    if nh <= 0 or not Ks:
        return stats
    if min(Ks) < 1 or max(Ks) > 127:
        raise ValueError(f"every K must lie in [1, 127], got {Ks}")
    Ks_h = np.ascontiguousarray(np.asarray(Ks, dtype=np.int32))
    ldo = _scalar_outputs(len(Ks), labels, (reconstruction_err, torch.float64), (n_iter, torch.int32),
                          (converged, torch.uint8))
    ws = nmf_workspace(m, md, B, Ks_h, dev)
    with timed("nmf_normals"):
        normals = nmf_normals(int(seed), m, md, Ks, n_init, dev)
    for a, rows, _, Xb in _row_batches(X64, idx_d, cols_d, h0, h1, B):
        stats['iterations'] += nmf_batch(rows, Xb, Ks_h, a, labels, normals, ws, tol, max_iter, reconstruction_err,
                                         n_iter, converged, ldo)
        stats['launches'] += 1
    return stats
