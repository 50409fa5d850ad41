"""Plain numpy references and inputs shared by the consensus edge tests (no GPU, no code under
test): the co-sampling and co-association counts of a sample-major label matrix as float64
products (one per channel, no per-resample loop), the 20 histogram counts of C, and the
cc_manhattan test input with the three float64 summation orders it has to tell apart."""
import functools

import numpy as np

from oracle import cc_oracle as O

UNSAMPLED = 0xFF


def label_matrix(idx, lab, n):
    """uint8 [n, H]: W[idx[h, r], h] = lab[h, r], 0xFF where row i is not in resample h."""
    H = idx.shape[0]
    W = np.full((n, H), UNSAMPLED, dtype=np.uint8)
    W[idx, np.arange(H)[:, None]] = lab
    return W


def counts_ref(W, K):
    """(I, M) int64 [n, n] of the label bytes W [n, H] (0xFF = not sampled): I = S S^T over the
    sampled indicator, M = sum over the K channels of A_c A_c^T with A_c = [W == c].  float64
    products of 0/1 matrices: exact below 2^53."""
    S = (W != UNSAMPLED).astype(np.float64)
    I = np.rint(S @ S.T).astype(np.int64)
    M = np.zeros_like(I)
    for c in range(K):
        A = (W == c).astype(np.float64)
        M += np.rint(A @ A.T).astype(np.int64)
    return I, M


def pair_hist(M, I):
    """numpy's 20 counts of the strict upper triangle of C = f32(M) / f32(I + 1e-6)."""
    n = M.shape[0]
    C = O.consensus_matrix(M.astype(np.uint16), I.astype(np.uint16))
    return np.histogram(C[np.triu_indices(n, 1)], bins=20, range=(0, 1))[0]


def uniform_case(n, H, frac, K, seed):
    """(idx int32 [H, m], lab int32 [H, m]): H resamples of m = frac n rows, labels uniform over
    all K channels."""
    rng = np.random.default_rng(seed)
    m = max(1, int(frac * n))
    idx = np.argsort(rng.random((H, n)), axis=1)[:, :m].astype(np.int32)
    lab = rng.integers(0, K, size=(H, m)).astype(np.int32)
    return idx, lab


def random_label_bytes(n, H, p, K, seed):
    """uint8 [n, H]: each entry sampled with probability p and then labelled uniformly over all
    K channels, else 0xFF."""
    rng = np.random.default_rng(seed)
    W = rng.integers(0, K, size=(n, H)).astype(np.uint8)
    W[rng.random((n, H)) >= p] = UNSAMPLED
    return W


@functools.lru_cache(maxsize=None)
def manhattan_input(n, d, seed=0):
    """float32 [n, d]: standard normals times 2^e, e uniform in [-30, 30).  The |differences| of
    such values span 60 binades, so their float64 sums round and depend on the order of the
    terms (values from [0, 1) sum exactly in float64 in any order)."""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((n, d)) * np.exp2(rng.integers(-30, 30, size=(n, d)))
    C = C.astype(np.float32)
    C.setflags(write=False)
    return C


def _term(C64, k):
    return np.abs(C64[:, k][:, None] - C64[:, k][None, :])  # [n, n], exact in float64


def _sum_terms(C, ks):
    C64 = np.asarray(C, dtype=np.float64)
    D = np.zeros((C64.shape[0], C64.shape[0]))
    for k in ks:
        D += _term(C64, k)
    return D


def manhattan_sequential(C):
    """D_ij = sum_k |C_ik - C_jk| in float64, k increasing, one accumulator: the scalar loop."""
    return _sum_terms(C, range(C.shape[1]))


def manhattan_reversed(C):
    """The same terms summed with k decreasing."""
    return _sum_terms(C, range(C.shape[1] - 1, -1, -1))


def manhattan_two_accumulators(C):
    """The same terms in an even-k and an odd-k accumulator, added at the end (a k loop unrolled
    by two, as a re-associated kernel would sum)."""
    return _sum_terms(C, range(0, C.shape[1], 2)) + _sum_terms(C, range(1, C.shape[1], 2))
