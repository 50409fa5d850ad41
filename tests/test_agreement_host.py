"""Host side of the pairwise agreement (post.agreement_from_sums) and the numpy reference of the
four sums (tests/agreement_ref.py) against sklearn's pair_confusion_matrix and
adjusted_rand_score and against brute-force pair counting.  No GPU."""
import itertools

import numpy as np
import pytest
from sklearn.metrics import adjusted_rand_score
from sklearn.metrics.cluster import pair_confusion_matrix

from consensus_clustering_amd import post
from tests.agreement_ref import confusion_from_sums, group_sums, pair_sums

ABSENT = 0xFF


def _pair(n, K, noise, absent, seed):
    """Two uint8 label columns: v repeats u except a `noise` share of random labels; an `absent`
    share of each column is 0xFF."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, K, size=n)
    v = np.where(rng.random(n) < noise, rng.integers(0, K, size=n), u)
    u = np.where(rng.random(n) < absent, ABSENT, u).astype(np.uint8)
    v = np.where(rng.random(n) < absent, ABSENT, v).astype(np.uint8)
    return u, v


PAIRS = [(n, K, noise, absent)
         for (n, K) in [(50, 2), (1000, 3), (1000, 127), (20_000, 8), (200_000, 20), (200_000, 127)]
         for noise in (0.0, 0.3, 0.999)
         for absent in (0.0, 0.2)]


@pytest.mark.parametrize("n,K,noise,absent", PAIRS)
def test_sums_are_sklearns_pair_confusion_matrix_and_ari(n, K, noise, absent):
    u, v = _pair(n, K, noise, absent, seed=n + K)
    s = pair_sums(u, v, K, K)
    both = (u != ABSENT) & (v != ABSENT)
    assert s[0] == both.sum()
    ref = pair_confusion_matrix(u[both], v[both])
    assert confusion_from_sums(s) == [[int(x) for x in row] for row in ref]
    ari = post.agreement_from_sums(s, 'ari')
    assert ari.shape == () and ari.dtype == np.float64
    want = adjusted_rand_score(u[both], v[both])
    print(f"n={n} K={K} noise={noise} absent={absent}: ari {float(ari)!r} sklearn {want!r} "
          f"diff {abs(float(ari) - want):.3g}")
    assert abs(float(ari) - want) <= 1e-12


def _brute(u, v, Ku, Kv):
    tp = fp = fn = 0
    ok = [i for i in range(len(u)) if u[i] < Ku and v[i] < Kv]
    for i, j in itertools.combinations(ok, 2):
        su, sv = u[i] == u[j], v[i] == v[j]
        tp += su and sv
        fn += su and not sv
        fp += sv and not su
    return len(ok), tp, fp, fn


@pytest.mark.parametrize("n,K,noise,absent", [(60, 3, 0.3, 0.2), (60, 7, 0.9, 0.0), (41, 2, 0.4, 0.5),
                                              (9, 4, 0.5, 0.3)])
def test_jaccard_is_brute_force_pair_counting(n, K, noise, absent):
    u, v = _pair(n, K, noise, absent, seed=7 * n + K)
    m, tp, fp, fn = _brute(u, v, K, K)
    assert m >= 2 and (fp or fn)
    got = post.agreement_from_sums(pair_sums(u, v, K, K), 'jaccard')
    assert float(got) == tp / (tp + fp + fn)


def test_vectorised_over_leading_axes():
    rng = np.random.default_rng(3)
    A = np.where(rng.random((300, 5)) < 0.3, ABSENT, rng.integers(0, 4, size=(300, 5))).astype(np.uint8)
    S = group_sums(A, 4)
    for index in post.AGREEMENT_INDICES:
        R = post.agreement_from_sums(S, index)
        assert R.shape == (5, 5) and R.dtype == np.float64
        np.testing.assert_array_equal(R, R.T)
        np.testing.assert_array_equal(np.diag(R), 1.0)
        for h1 in range(5):
            for h2 in range(5):
                assert R[h1, h2] == post.agreement_from_sums(S[h1, h2], index)


def test_fewer_than_two_shared_items_is_nan():
    u = np.array([0, 1, ABSENT, ABSENT], dtype=np.uint8)
    v = np.array([ABSENT, 1, 0, ABSENT], dtype=np.uint8)
    s1 = pair_sums(u, v, 2, 2)
    assert s1[0] == 1
    s0 = pair_sums(u, np.full(4, ABSENT, dtype=np.uint8), 2, 2)
    assert s0[0] == 0
    for index in post.AGREEMENT_INDICES:
        assert np.isnan(post.agreement_from_sums(s1, index))
        assert np.isnan(post.agreement_from_sums(s0, index))


def test_identical_columns_and_all_singletons_give_one():
    u, _ = _pair(500, 6, 0.0, 0.2, seed=1)
    same = pair_sums(u, u, 6, 6)
    relabelled = pair_sums(u, np.where(u == ABSENT, ABSENT, (u + 1) % 6).astype(np.uint8), 6, 6)
    singles = pair_sums(np.arange(100, dtype=np.uint8), np.arange(100, dtype=np.uint8)[::-1].copy(), 100, 100)
    assert singles[0] == 100 and singles[1] == 100
    for index in post.AGREEMENT_INDICES:
        assert post.agreement_from_sums(same, index) == 1.0
        assert post.agreement_from_sums(relabelled, index) == 1.0
        assert post.agreement_from_sums(singles, index) == 1.0


def test_unknown_index_and_bad_shape_raise():
    s = pair_sums(*_pair(50, 2, 0.3, 0.0, seed=0), 2, 2)
    with pytest.raises(ValueError):
        post.agreement_from_sums(s, 'rand')
    with pytest.raises(ValueError):
        post.agreement_from_sums(s[:3], 'ari')


def test_exchanging_r2_and_c2_is_the_transposed_pair():
    u, v = _pair(400, 5, 0.6, 0.2, seed=11)
    v = (v // 2 * (v != ABSENT) + ABSENT * (v == ABSENT)).astype(np.uint8)  # 3 coarser clusters: r2 != c2
    s, t = pair_sums(u, v, 5, 3), pair_sums(v, u, 3, 5)
    assert s[2] != s[3]
    np.testing.assert_array_equal(t, s[[0, 1, 3, 2]])
    for index in post.AGREEMENT_INDICES:
        assert post.agreement_from_sums(s, index) == post.agreement_from_sums(t, index)
