"""Host checks behind the consensus edge tests (no GPU): the cc_manhattan test input really
separates summation orders, scipy's pdist sums in the order ccmi.h names, and the numpy
references of tests/consensus_edges_ref.py agree with the oracle's per-resample definitions."""
import numpy as np
import pytest
from scipy.spatial.distance import pdist, squareform

from oracle import cc_oracle as O
from tests import consensus_edges_ref as R


def _differing(A, B):
    n = A.shape[0]
    iu = np.triu_indices(n, 1)
    return float(np.mean(A[iu] != B[iu]))


def test_manhattan_input_separates_summation_orders():
    """The scaled-normal input of the GPU test (n = 130, d = 37, seed 0): the sequential float64
    sum over k differs from the reversed sum and from the even/odd two-accumulator sum in at
    least a quarter of the pairs, so a cc_manhattan whose k loop were re-associated could not
    equal scipy bit for bit on it."""
    C = R.manhattan_input(130, 37)
    seq = R.manhattan_sequential(C)
    rev, two = _differing(seq, R.manhattan_reversed(C)), _differing(seq, R.manhattan_two_accumulators(C))
    print(f"pairs differing from the sequential sum: reversed {rev:.3f}, two accumulators {two:.3f}")
    assert rev >= 0.25 and two >= 0.25


def test_unit_interval_input_cannot_separate_them():
    """Why the new input exists: float32 values from [0, 1) (test_manhattan_kernel_matches_scipy's
    data, same generator and shapes) have |differences| that sum exactly in float64, so every
    order gives the same bits and the 'scipy's order' claim could not fail on them."""
    rng = np.random.default_rng(3)
    for n, d in ((29, 29), (300, 300), (257, 70)):
        C = rng.random((n, d)).astype(np.float32)
        seq = R.manhattan_sequential(C)
        assert _differing(seq, R.manhattan_reversed(C)) == 0.0
        assert _differing(seq, R.manhattan_two_accumulators(C)) == 0.0


@pytest.mark.parametrize("n,d", [(1, 1), (2, 3), (40, 15), (130, 4), (130, 37)])
def test_scipy_cityblock_is_the_sequential_sum(n, d):
    """The order scipy really uses: pdist(C, 'cityblock') equals the one-accumulator float64 loop
    over increasing k bit for bit on the order-sensitive input (and so is a reference that tells
    cc_manhattan's order apart)."""
    C = R.manhattan_input(n, d)
    np.testing.assert_array_equal(squareform(pdist(C, "cityblock")), R.manhattan_sequential(C))


@pytest.mark.parametrize("K", [1, 2, 5, 33])
def test_product_references_match_the_oracle(K):
    """counts_ref (sampled-indicator product, one product per channel) equals the oracle's
    per-resample co-sampling and co-association counts."""
    n, H = 70, 23
    idx, lab = R.uniform_case(n, H, 0.6, K, seed=K)
    W = R.label_matrix(idx, lab, n)
    I, M = R.counts_ref(W, K)
    np.testing.assert_array_equal(I, O.cosample_matrix(idx.astype(np.int64), n))
    np.testing.assert_array_equal(M, O.coassoc_matrix(idx.astype(np.int64), lab.astype(np.int64), K, n))
    assert R.pair_hist(M, I).sum() == n * (n - 1) // 2
