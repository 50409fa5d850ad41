"""cc_scatter_labels and cc_copy_label_columns (csrc/coassoc.hip:1201-1227) against numpy, byte
for byte over the whole destination: what they address is written, everything else keeps its
fill, and calls outside the contract of include/ccmi.h are refused before any launch."""
import numpy as np
import pytest
import torch

from consensus_clustering_amd import _lib, engine

pytestmark = pytest.mark.gpu

CC_OK, CC_ERR_ARG = 0, -1


def _scatter_ref(out, idx, lab, n, h_offset=0):
    """The numpy loop of ccmi.h's rule: out[idx[h, r], h_offset + h] = lab[h, r] (0 without
    labels); an idx outside [0, n) addresses no row and is skipped."""
    out = out.copy()
    H, m = idx.shape
    for h in range(H):
        for r in range(m):
            row = int(idx[h, r])
            if 0 <= row < n:
                out[row, h_offset + h] = 0 if lab is None else lab[h, r] & 0xFF
    return out


def _case(n, H, m, K, seed):
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.permutation(n)[:m] for _ in range(H)]).astype(np.int32)
    lab = rng.integers(0, K, size=(H, m)).astype(np.int32)
    return idx, lab


@pytest.mark.parametrize("h_offset,width", [(0, 41), (7, 64), (23, 64)])
@pytest.mark.parametrize("with_labels", [True, False])
def test_scatter_labels_into_a_wider_matrix(h_offset, width, with_labels):
    """engine.scatter_labels with a non-zero h_offset into a wider matrix (the fit only ever
    passes 0), and labels_hm = None (the sampled flag: writes 0): scatter_labels_kernel's
    `row * ldl + h` (coassoc.hip:1209) from a base moved h_offset columns in, row stride
    unchanged.  Every byte not addressed keeps its 0xFF."""
    dev = engine.require_gpu()
    n, H, m, K = 90, 41, 55, 100
    idx, lab = _case(n, H, m, K, seed=h_offset)
    out = engine.new_label_matrix(1, n, width, dev)[0]
    engine.scatter_labels(torch.from_numpy(idx).to(dev), torch.from_numpy(lab).to(dev) if with_labels else None,
                          n, out, h_offset=h_offset)
    want = _scatter_ref(np.full((n, width), 0xFF, np.uint8), idx, lab if with_labels else None, n, h_offset)
    assert (want != 0xFF).sum() == H * m
    np.testing.assert_array_equal(out.cpu().numpy(), want)


def test_scatter_labels_skips_rows_outside_the_matrix():
    """ccmi.h: an idx entry outside [0, n) is skipped (coassoc.hip:1208).  -1, n and n + 5 among
    the indices write nothing anywhere -- the matrix is one allocation with guard rows of 0xFF on
    both sides of the n rows handed in, and all of it is compared."""
    dev = engine.require_gpu()
    n, H, m, K, guard = 60, 33, 40, 9, 8
    idx, lab = _case(n, H, m, K, seed=5)
    rng = np.random.default_rng(6)
    bad = rng.random((H, m)) < 0.2
    idx[bad] = rng.choice(np.array([-1, n, n + 5], dtype=np.int32), size=int(bad.sum()))
    assert {-1, n, n + 5} <= set(idx.ravel().tolist())
    whole = torch.full((guard + n + guard, 128), 0xFF, dtype=torch.uint8, device=dev)
    engine.scatter_labels(torch.from_numpy(idx).to(dev), torch.from_numpy(lab).to(dev), n, whole[guard:guard + n])
    want = np.full((guard + n + guard, 128), 0xFF, np.uint8)
    want[guard:guard + n] = _scatter_ref(want[guard:guard + n], idx, lab, n)
    assert (want != 0xFF).sum() == int((~bad).sum())
    np.testing.assert_array_equal(whole.cpu().numpy(), want)


@pytest.mark.parametrize("H,m", [(0, 5), (5, 0), (0, 0)])
def test_scatter_labels_empty_writes_nothing(H, m):
    """H = 0 or m = 0 (a rank that owns no resample): CC_OK from the C entry point with live
    pointers, nothing launched; and engine.scatter_labels accepts the empty tensors."""
    dev = engine.require_gpu()
    n = 10
    out = engine.new_label_matrix(1, n, 128, dev)[0]
    live = torch.zeros(8, dtype=torch.int32, device=dev)
    rc = _lib.load().cc_scatter_labels(live.data_ptr(), live.data_ptr(), H, m, n, out.data_ptr(), 128,
                                       engine.stream_ptr())
    assert rc == CC_OK
    idx = torch.zeros((H, m), dtype=torch.int32, device=dev)
    engine.scatter_labels(idx, idx.clone(), n, out)
    engine.scatter_labels(idx, None, n, out)
    torch.cuda.synchronize()
    assert bool((out == 0xFF).all())


def test_scatter_labels_refusals():
    """ldl < H, a null pointer, n <= 0 and a negative size return CC_ERR_ARG (coassoc.hip:1334)
    and leave the matrix untouched."""
    dev = engine.require_gpu()
    lib = _lib.load()
    n, H, m = 10, 40, 4
    idx = torch.zeros((H, m), dtype=torch.int32, device=dev)
    out = engine.new_label_matrix(1, n, 128, dev)[0]
    st = engine.stream_ptr()
    i, o = idx.data_ptr(), out.data_ptr()
    for args in ((i, i, H, m, n, o, H - 1),   # ldl < H
                 (None, i, H, m, n, o, 128), (i, i, H, m, n, None, 128),
                 (i, i, H, m, 0, o, 128), (i, i, -1, m, n, o, 128), (i, i, H, -1, n, o, 128)):
        assert lib.cc_scatter_labels(*args, st) == CC_ERR_ARG, args
        assert b"cc_scatter_labels" in lib.cc_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0xFF).all())
    with pytest.raises(_lib.CCMIError, match="ldl >= H"):  # through the engine: a matrix narrower than H
        engine.scatter_labels(idx, None, n, engine.new_label_matrix(1, n, 32, dev)[0])


def _sentinel(shape, dev, salt):
    a = (np.arange(int(np.prod(shape)), dtype=np.int64) * 37 + salt) % 251
    return torch.from_numpy(a.astype(np.uint8).reshape(shape)).to(dev)


@pytest.mark.parametrize("width", [0, 1, 13, 128])
@pytest.mark.parametrize("col_src,col_dst,ld_src,ld_dst", [(3, 5, 160, 256), (0, 128, 128, 256), (17, 0, 256, 128)])
def test_copy_label_columns(width, col_src, col_dst, ld_src, ld_dst):
    """dst[..., col_dst : col_dst + width] = src[..., col_src : col_src + width] on [nK, n, ld]
    tensors (copy_label_columns_kernel, coassoc.hip:1217-1227: one thread per byte,
    `r * ld + col + j`), unaligned columns (3 -> 5), different strides, widths from nothing to a
    whole 128-column block; the destination starts as a sentinel pattern and every byte outside
    the window keeps it."""
    dev = engine.require_gpu()
    nK, n = 3, 37
    src, dst = _sentinel((nK, n, ld_src), dev, 1), _sentinel((nK, n, ld_dst), dev, 2)
    want = dst.cpu().numpy().copy()
    want[..., col_dst:col_dst + width] = src.cpu().numpy()[..., col_src:col_src + width]
    engine.copy_label_columns(src, col_src, dst, col_dst, width)
    np.testing.assert_array_equal(dst.cpu().numpy(), want)
    np.testing.assert_array_equal(src.cpu().numpy(), _sentinel((nK, n, ld_src), dev, 1).cpu().numpy())


def test_copy_label_columns_refusals():
    """A window past either stride, a negative column or size, and a null pointer with a
    non-empty window return CC_ERR_ARG (coassoc.hip:1349-1350) with the destination untouched; a
    null pointer with an empty window is CC_OK."""
    dev = engine.require_gpu()
    lib = _lib.load()
    rows, ld_s, ld_d = 20, 64, 48
    src, dst = _sentinel((rows, ld_s), dev, 3), _sentinel((rows, ld_d), dev, 4)
    before = dst.cpu().numpy().copy()
    st = engine.stream_ptr()
    s, d = src.data_ptr(), dst.data_ptr()
    for args in ((s, ld_s, 60, d, ld_d, 0, rows, 5),    # past the source stride
                 (s, ld_s, 0, d, ld_d, 44, rows, 5),    # past the destination stride
                 (s, ld_s, 0, d, ld_d, 0, rows, 49),    # wider than the destination
                 (s, ld_s, -1, d, ld_d, 0, rows, 5), (s, ld_s, 0, d, ld_d, -1, rows, 5),
                 (s, ld_s, 0, d, ld_d, 0, -1, 5), (s, ld_s, 0, d, ld_d, 0, rows, -1),
                 (None, ld_s, 0, d, ld_d, 0, rows, 5), (s, ld_s, 0, None, ld_d, 0, rows, 5)):
        assert lib.cc_copy_label_columns(*args, st) == CC_ERR_ARG, args
        assert b"cc_copy_label_columns" in lib.cc_last_error()
    assert lib.cc_copy_label_columns(None, ld_s, 0, None, ld_d, 0, rows, 0, st) == CC_OK
    assert lib.cc_copy_label_columns(None, ld_s, 0, None, ld_d, 0, 0, 5, st) == CC_OK
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dst.cpu().numpy(), before)
    with pytest.raises(_lib.CCMIError, match="window"):
        engine.copy_label_columns(src, 60, _sentinel((rows, ld_d), dev, 4), 0, 5)
