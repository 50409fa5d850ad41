"""Numpy reference of the agreement sums (not collected by pytest): for label columns with one
byte per item, a cluster in [0, K) or anything else = absent, the contingency table N of the
items present in both columns and (s0, s2, r2, c2) = (sum N, sum N^2, sum of squared row sums,
sum of squared column sums).  Shared by tests/test_agreement_host.py and tests/test_gpu_agreement.py."""
import numpy as np


def contingency(u, v, Ku, Kv):
    """int64 [Ku, Kv]: N[a][b] = #{items with u = a and v = b}; ids outside [0, K) count nowhere."""
    u = np.asarray(u).astype(np.int64)
    v = np.asarray(v).astype(np.int64)
    both = (u >= 0) & (u < Ku) & (v >= 0) & (v < Kv)
    N = np.zeros((Ku, Kv), dtype=np.int64)
    np.add.at(N, (u[both], v[both]), 1)
    return N


def pair_sums(u, v, Ku, Kv):
    N = contingency(u, v, Ku, Kv)
    return np.array([N.sum(), (N * N).sum(), (N.sum(axis=1) ** 2).sum(), (N.sum(axis=0) ** 2).sum()],
                    dtype=np.int64)


def group_sums(A, KA, B=None, KB=None):
    """int64 [HA, HB, 4] for the columns of A [n, HA] against those of B [n, HB] (default: A)."""
    A = np.asarray(A)
    if B is None:
        B, KB = A, KA
    B = np.asarray(B)
    out = np.zeros((A.shape[1], B.shape[1], 4), dtype=np.int64)
    for h1 in range(A.shape[1]):
        for h2 in range(B.shape[1]):
            out[h1, h2] = pair_sums(A[:, h1], B[:, h2], KA, KB)
    return out


def confusion_from_sums(s):
    """sklearn's pair_confusion_matrix [[C00, C01], [C10, C11]] from (s0, s2, r2, c2), in Python ints."""
    s0, s2, r2, c2 = (int(x) for x in s)
    c11, c01, c10 = s2 - s0, c2 - s2, r2 - s2
    return [[s0 * s0 - c01 - c10 - s2, c01], [c10, c11]]
