"""Shared init-0 seeding of the d <= 128 k-means engine (kmeans.hip): within a unit, the init-0
problems of one trial class (equal 2 + floor(ln K)) follow the k-means++ chain of the class's
largest K instead of seeding themselves.  Labels, inertia and n_iter must be bit-identical to
independent seeding, and the seeding work of the followers must really be gone."""
import numpy as np
import pytest
import torch

from consensus_clustering_amd import engine
from consensus_clustering_amd.kmeans import BatchedKMeans, local_trials, prepare_rows

pytestmark = pytest.mark.gpu

N, M, H, SEED = 500, 400, 6, 7
DIMS = [128, 50, 20]  # the DP = 128, 64 and 32 instantiations

_DATA = {}


def data(d):
    """Rows, resamples and the device row image for feature count d (built once per d)."""
    if d not in _DATA:
        dev = engine.require_gpu()
        rng = np.random.default_rng(100 + d)
        centers = rng.uniform(-10, 10, size=(6, d))
        X = (centers[rng.integers(0, 6, size=N)] + rng.normal(size=(N, d))).astype(np.float32)
        idx = engine.resample_indices(SEED, N, M, 0, H)
        _DATA[d] = (dev, torch.from_numpy(idx).to(dev)) + tuple(prepare_rows(X, dev))
    return _DATA[d]


def run(d, Ks, n_init=3, seedmax=None):
    dev, idx_d, Xd, xn, _, Xhl, e = data(d)
    L = engine.new_label_matrix(len(Ks), N, engine.pad_h(H), dev)
    inert = torch.zeros((len(Ks), H), dtype=torch.float32, device=dev)
    nit = torch.zeros((len(Ks), H), dtype=torch.int32, device=dev)
    bk = BatchedKMeans(Ks, n_init=n_init, random_state=SEED, seedmax=seedmax)
    bk.run(Xd, xn, d, idx_d, N, H, M, 0, H, L, np.float32, inertia=inert, n_iter=nit, Xhl=Xhl, scale_exp=e)
    torch.cuda.synchronize()
    return L.cpu().numpy(), inert.cpu().numpy(), nit.cpu().numpy(), bk.stats.cpu().numpy(), bk.units


def same(a, b, what):
    for x, y, name in zip(a[:3], b[:3], ("labels", "inertia", "n_iter")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}")


def columns(Ks):
    return {K: 1 + (K - 1) * local_trials(K) for K in Ks}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.delenv("CCMI_KM_SHARE_SEED", raising=False)
    monkeypatch.delenv("CCMI_SEEDMAX", raising=False)
    monkeypatch.setenv("CCMI_NSUB", "1")  # one unit per resample: every class shares


@pytest.mark.parametrize("d", DIMS)
def test_alone_against_in_range(d):
    """A single K has no follower: its fit must equal the same K fitted inside the range 2..12
    (trial classes {2}, {3..7}, {8..12}), where all but 2, 7 and 12 follow."""
    Ks = list(range(2, 13))
    full = run(d, Ks)
    assert full[4].shape[0] == 1 and full[4][0, 0] == 3 * len(Ks)
    for k, K in enumerate(Ks):
        one = run(d, [K])
        same([x[k:k + 1] for x in full[:3]], one, f"d={d} K={K}")


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("Ks,n_init,seedmax,nsub", [
    ([3, 5, 8, 20], 3, None, 1),   # gaps in the range
    ([1, 2], 3, None, 1),          # K' = 1 is ready after the leader's first sweep
    ([4], 3, None, 1),             # no follower
    ([2, 3, 4, 5, 8, 9, 12], 1, None, 1),
    ([2, 3, 4, 5, 8, 9, 12], 3, 1, 1),
    ([2, 3, 4, 5, 8, 9, 12], 3, 32, 1),
    ([2, 3, 4, 5, 6, 7, 8, 9, 12], 3, None, 2),  # classes split over units
    ([2, 3, 4, 5, 6, 7, 8, 9, 12], 3, None, 3),
    ([21, 30, 54], 3, None, 1),        # inside trial class 5 (K = 21..54): 54 leads
    ([55, 90, 127], 3, None, 1),       # inside trial class 6 = TMAX (K >= 55): 127 leads
    ([20, 21, 54, 55], 3, None, 1),    # across both class boundaries: leaders 20, 54, 55
])
def test_switch_on_against_off(monkeypatch, d, Ks, n_init, seedmax, nsub):
    monkeypatch.setenv("CCMI_NSUB", str(nsub))
    on = run(d, Ks, n_init, seedmax)
    monkeypatch.setenv("CCMI_KM_SHARE_SEED", "0")
    off = run(d, Ks, n_init, seedmax)
    assert on[4].shape[0] == min(nsub, len(Ks))
    same(on, off, f"d={d} Ks={Ks} n_init={n_init} seedmax={seedmax} n_sub={nsub}")
    assert on[3][1] <= off[3][1]


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("Ks,n_init", [(list(range(2, 13)), 3), ([3, 5, 8, 20], 3), ([1, 2], 2), ([4], 3)])
def test_follower_seeding_work_is_gone(monkeypatch, d, Ks, n_init):
    """stats[1] counts candidate columns x rows.  Independent seeding sweeps 1 + (K-1) t_K columns
    per (K, init); with sharing, init 0 sweeps only the columns of each class's largest K."""
    col = columns(Ks)
    lead = {}
    for K in Ks:
        lead[local_trials(K)] = max(lead.get(local_trials(K), 0), K)
    shared = (n_init - 1) * sum(col.values()) + sum(col[K] for K in lead.values())
    on = run(d, Ks, n_init)
    assert on[4].shape[0] == 1
    assert on[3][1] == M * H * shared
    monkeypatch.setenv("CCMI_KM_SHARE_SEED", "0")
    off = run(d, Ks, n_init)
    assert off[3][1] == M * H * n_init * sum(col.values())
