"""Host finish of the item / cluster consensus (post.item_consensus_from_sums,
post.cluster_consensus_from_sums): Monti's m_i(c) and m(c) from the exact int64 sums
S[i, c] = sum_{j != i, cl[j] == c} C_ij * 2^40, against brute-force float64 means of C (no GPU)."""
import numpy as np
import pytest

from consensus_clustering_amd import post

TWO40 = float(1 << 40)


def _random_consensus(n, H, rng):
    """A symmetric float32 C of the form the fit produces: f32(M) / f32(I + 1e-6), 0 <= M <= I <= H,
    with pairs never co-sampled (I = 0)."""
    I = rng.integers(0, H + 1, size=(n, n))
    I = np.triu(I, 1)
    I = I + I.T
    M = np.floor(I * rng.random((n, n))).astype(np.int64)
    M = np.triu(M, 1)
    M = M + M.T
    M[rng.random((n, n)) < 0.2] = 0
    M = np.minimum(M, M.T)
    same = np.triu(rng.random((n, n)) < 0.1, 1)
    M = np.where(same | same.T, I, M)  # pairs always together: M = I
    C = np.divide(M, I + 1e-6, dtype=np.float32)
    assert (C == C.T).all() and C.min() >= 0 and C.max() <= 1
    return C


def _sums(C, labels, Kc):
    """Q @ onehot in int64: Q = int64(float64(C) * 2^40) with the diagonal zeroed."""
    x = C.astype(np.float64) * TWO40
    Q = x.astype(np.int64)
    assert (Q.astype(np.float64) == x).all(), "C * 2^40 must be an integer"
    np.fill_diagonal(Q, 0)
    onehot = np.zeros((len(labels), Kc), dtype=np.int64)
    ok = (labels >= 0) & (labels < Kc)
    onehot[np.flatnonzero(ok), labels[ok]] = 1
    return Q @ onehot


def _brute(C, labels, Kc):
    n = len(labels)
    C = C.astype(np.float64)
    item = np.full((n, Kc), np.nan)
    clus = np.full(Kc, np.nan)
    for c in range(Kc):
        members = np.flatnonzero(labels == c)
        for i in range(n):
            others = members[members != i]
            if len(others):
                item[i, c] = C[i, others].sum() / len(others)
        if len(members) >= 2:
            sub = C[np.ix_(members, members)]
            clus[c] = np.triu(sub, 1).sum() * 2.0 / (len(members) * (len(members) - 1))
    return item, clus


@pytest.mark.parametrize("n,H,Kc,seed", [(400, 1000, 6, 0), (257, 65535, 17, 1), (50, 25, 3, 2), (2, 5, 2, 3)])
def test_means_from_sums_match_brute_force(n, H, Kc, seed):
    rng = np.random.default_rng(seed)
    C = _random_consensus(n, H, rng)
    labels = rng.integers(0, Kc, size=n)
    S = _sums(C, labels, Kc)
    # the sums themselves: each row sum of the products, exactly
    for c in range(Kc):
        col = np.array([sum(int(q) for j, q in enumerate((C[i].astype(np.float64) * TWO40).astype(np.int64))
                            if j != i and labels[j] == c) for i in range(min(n, 20))], dtype=np.int64)
        np.testing.assert_array_equal(S[:len(col), c], col)
    item = post.item_consensus_from_sums(S, labels, Kc)
    clus = post.cluster_consensus_from_sums(S, labels, Kc)
    ref_item, ref_clus = _brute(C, labels, Kc)
    assert item.dtype == np.float64 and item.shape == (n, Kc) and clus.shape == (Kc,)
    np.testing.assert_array_equal(np.isnan(item), np.isnan(ref_item))
    np.testing.assert_array_equal(np.isnan(clus), np.isnan(ref_clus))
    # S is exact; one float64 conversion and one division round (2^-52 each); the brute-force
    # numpy sum of <= 400 terms adds less than 1e-13
    np.testing.assert_allclose(item, ref_item, rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose(clus, ref_clus, rtol=1e-12, atol=0, equal_nan=True)
    ok = ~np.isnan(item)
    assert (item[ok] >= 0).all() and (item[ok] <= 1).all()


def test_nan_cases():
    rng = np.random.default_rng(5)
    n, Kc = 40, 5
    C = _random_consensus(n, 100, rng)
    labels = rng.integers(0, 2, size=n)  # ids 0 and 1 populated
    labels[7] = 2                        # id 2: a singleton; id 3: empty; id 4: two members
    labels[11] = labels[12] = 4
    S = _sums(C, labels, Kc)
    item = post.item_consensus_from_sums(S, labels, Kc)
    clus = post.cluster_consensus_from_sums(S, labels, Kc)
    assert np.isnan(item[7, 2])                          # an item's own singleton cluster
    others = np.arange(n) != 7
    assert not np.isnan(item[others, 2]).any()           # everyone else has one partner there
    np.testing.assert_allclose(item[others, 2], C[others, 7].astype(np.float64), rtol=1e-15)
    assert np.isnan(item[:, 3]).all()                    # an empty cluster id
    assert np.isnan(clus[2]) and np.isnan(clus[3])       # singleton and empty: no pair
    assert not np.isnan(clus[[0, 1, 4]]).any()
    assert clus[4] == float(C[11, 12])


def test_masked_labels_belong_to_no_cluster():
    rng = np.random.default_rng(6)
    n, Kc = 30, 3
    C = _random_consensus(n, 50, rng)
    labels = rng.integers(0, Kc, size=n)
    labels[::3] = -1
    S = _sums(C, labels, Kc)
    item = post.item_consensus_from_sums(S, labels, Kc)
    ref_item, ref_clus = _brute(C, labels, Kc)
    np.testing.assert_allclose(item, ref_item, rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(post.cluster_consensus_from_sums(S, labels, Kc), ref_clus, rtol=1e-12,
                               equal_nan=True)


def test_cluster_total_beyond_int64_is_exact():
    """8 members with S = 2^61 each: T_c = 2^64 does not fit int64; m(c) = 2^64 / (2^40 * 56)."""
    labels = np.zeros(8, dtype=np.int64)
    S = np.full((8, 1), 1 << 61, dtype=np.int64)
    got = post.cluster_consensus_from_sums(S, labels, 1)
    assert got[0] == (1 << 64) / ((1 << 40) * 56)
    # a total whose low bits matter: exact integer sum, one rounding
    S2 = S.copy()
    S2[0, 0] += 1
    want = ((1 << 64) + 1) / ((1 << 40) * 56)
    assert post.cluster_consensus_from_sums(S2, labels, 1)[0] == want


def test_shape_is_checked():
    with pytest.raises(ValueError):
        post.item_consensus_from_sums(np.zeros((3, 2), np.int64), np.zeros(4, np.int64), 2)
    with pytest.raises(ValueError):
        post.cluster_consensus_from_sums(np.zeros((4, 3), np.int64), np.zeros(4, np.int64), 2)
