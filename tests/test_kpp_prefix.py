"""The invariant the shared init-0 seeding of the d <= 128 k-means engine relies on: every K
replays RandomState(seed), so init 0 draws the same first centre for every K, and within a trial
class (equal 2 + floor(ln K)) the uniforms of init 0 of K are a prefix of those of the class's
largest K."""
import numpy as np
import pytest

from consensus_clustering_amd import kmeans


@pytest.mark.parametrize("seed,m,dtype", [(0, 400, np.float32), (23, 40000, np.float32), (7, 1000, np.float64)])
def test_init0_streams_are_prefixes_within_a_trial_class(seed, m, dtype):
    Ks = list(range(1, 41))
    u, pos, stride = kmeans.kpp_tables(Ks, 3, seed, m, dtype)
    assert np.all(pos[:, 0] == pos[0, 0])
    classes = {}
    for k, K in enumerate(Ks):
        classes.setdefault(kmeans.local_trials(K), []).append(k)
    assert len(classes) == 4  # t = 2: {1, 2}, 3: {3..7}, 4: {8..20}, 5: {21..40}
    for t, members in classes.items():
        lead = max(members, key=lambda k: Ks[k])
        for k in members:
            L = 1 + (Ks[k] - 1) * t
            assert L <= stride
            np.testing.assert_array_equal(u[k, 0, :L], u[lead, 0, :L])
