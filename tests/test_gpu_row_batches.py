"""The range check of the row-batch driver (engine._row_batches), which the GMM, FullGMM and NMF
clusterers share: a row or column index outside its range is refused from the device tensors
before anything is launched, so the label matrix stays untouched."""
import numpy as np
import pytest
import torch

from consensus_clustering_amd import engine

pytestmark = pytest.mark.gpu

N, M, D, H, KS = 40, 32, 5, 2, [2]


def _labels_of(who, X64, idx_d, labels, cols_d):
    if who == 'nmf':
        return engine.nmf_labels(X64, idx_d, 0, H, KS, labels, cols_d=cols_d)
    return engine.gmm_labels(X64, idx_d, 0, H, KS, labels, cols_d=cols_d, covariance=who)


@pytest.mark.parametrize("who", ['diag', 'full', 'nmf'])
def test_an_index_outside_its_range_is_refused_before_any_launch(who):
    rs = np.random.RandomState(7)
    X64 = torch.from_numpy(np.abs(rs.normal(size=(N, D)))).cuda()
    idx = np.stack([rs.choice(N, size=M, replace=False) for _ in range(H)]).astype(np.int32)
    cols = np.stack([rs.choice(D, size=3, replace=False) for _ in range(H)]).astype(np.int32)
    bad_idx, bad_cols = idx.copy(), cols.copy()
    bad_idx[1, M - 1] = N
    bad_cols[1, 0] = D
    for rows, columns, message in ((bad_idx, None, "idx entries must lie in"),
                                   (idx, bad_cols, "cols entries must lie in")):
        labels = engine.new_label_matrix(len(KS), N, engine.pad_h(H), "cuda")
        with pytest.raises(ValueError, match=message):
            _labels_of(who, X64, torch.from_numpy(rows).cuda(),
                       labels, None if columns is None else torch.from_numpy(columns).cuda())
        torch.cuda.synchronize()
        assert bool((labels == 0xFF).all())
