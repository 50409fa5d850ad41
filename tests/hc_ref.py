"""Host references for the cut of the hierarchical base clusterer (no GPU, no kernel's method):
synthetic trees in nn_chain's raw form, of a shape that data never gives (the caterpillar), and
a sequential restatement of the K-cluster cut to compare cc_hc_cut with."""
import numpy as np


def synthetic_merges(m, kind, rs=None):
    """Raw merges [m-1, 4] in nn_chain's form: row j is (x, y, distance, size) with x < y, slot x
    dies and slot y keeps the union.  kind 'chain': merge j is (j, j + 1), the caterpillar whose
    slot j dies into j + 1 (depth m - 1); 'bypass': the caterpillar that passes slot m - 2 by
    (..., (m - 4, m - 3), (m - 3, m - 1), then (m - 2, m - 1); depth m - 2; the chain itself
    below m = 3); 'random': two live slots drawn uniformly from rs (a RandomState).  The
    distances are 0, 1, ..., m - 2 (strictly increasing: rank = merge order); a caller that
    wants ties or another order overwrites column 2.

    Why 'bypass': a cluster of the chain is an interval of slots with its root on top, so an
    ancestor that is not yet the root has as many roots below it as the root has, and gets the
    right id.  In 'bypass' the cut at K = 2 leaves slot m - 2 a root of its own, just below the
    root m - 1 of all the others: every ancestor short of the root then counts one root fewer."""
    Z = np.empty((m - 1, 4), dtype=np.float64)
    Z[:, 2] = np.arange(m - 1)
    if kind in ("chain", "bypass"):
        Z[:, 0] = np.arange(m - 1)
        Z[:, 1] = np.arange(1, m)
        Z[:, 3] = np.arange(2, m + 1)
        if kind == "bypass" and m >= 3:
            Z[m - 3, 1] = m - 1
        return Z
    if kind != "random":
        raise ValueError(kind)
    live = np.arange(m)  # the live slots are live[:count], in no order
    size = np.ones(m, dtype=np.int64)
    for j in range(m - 1):
        count = m - j
        p = int(rs.randint(count))
        q = int(rs.randint(count - 1))
        q += q >= p  # uniform over the other live slots
        a, b = int(live[p]), int(live[q])
        x, y = (a, b) if a < b else (b, a)
        size[y] += size[x]
        Z[j, 0], Z[j, 1], Z[j, 3] = x, y, size[y]
        live[p if a == x else q] = live[count - 1]  # x leaves the live set
    return Z


def reference_cut(Z, m, K):
    """Labels [m] of the K-cluster cut of the raw merges Z, as hclust.hip defines it: the merges
    are ranked by distance (stable), slot x of a merge of rank < m - K links to its y, a leaf's
    cluster is the root of its slot, and a root's id is the number of roots below it.  Resolved
    sequentially from the highest slot down (links only point upward), not by pointer jumping."""
    Z = np.asarray(Z)
    order = np.argsort(Z[:, 2], kind="mergesort")
    kept = order[: max(m - K, 0)]
    link = np.arange(m)
    link[Z[kept, 0].astype(np.int64)] = Z[kept, 1].astype(np.int64)
    is_root = link == np.arange(m)
    root = link.tolist()
    for i in range(m - 1, -1, -1):
        root[i] = root[root[i]]  # root[link[i]] is final: link[i] >= i
    ids = np.cumsum(is_root) - 1
    return ids[np.asarray(root, dtype=np.int64)]
