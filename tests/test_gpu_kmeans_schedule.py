"""The sweep scheduler and the post-sweep label compare of the d <= 128 k-means engine against the
engine's own output at the commit named in tests/golden/engine/schedule_parent.npz, before the
scheduler moved from one thread to a wave and the compare kept its loads in flight.

The labels, inertia and n_iter of a fit do not depend on how the problems are packed into sweeps,
so they alone would not catch a scheduler that packs differently.  The engine's own counters do:
stats[0:8] = Lloyd column-rows, seeding column-rows, M-step rows, relocations, sweeps, slot tiles,
sparse item-sweeps, label changes.  Identical sweep and slot-tile counts mean the same items went
into the same sweeps; identical label changes mean the compare counted every row.  Everything is
compared exactly.

Every case runs all its problems in ONE unit per resample (CCMI_NSUB=1), so that the capacity
rules of the scheduler bind:
  seedcap    K = 8..20, n_init 3, 32 seeding slots, every problem seeding on its own
             (CCMI_KM_SHARE_SEED=0): 32 seeding problems want 128 candidate half-steps against
             the 80 of a sweep, so the seeding walk runs out of steps; later the 39 Lloyd items
             need about 700 slots against 256, so the Lloyd walk skips and S.rr rotates;
  share      the same with shared init-0 seeding (followers, fgo);
  lloydcap   K = 2, 3, 4 with n_init 16: 48 Lloyd items in 192 slots against the 44 Lloyd steps;
             its seeding problems draw 2 or 3 candidates, so here the seeding walk, out of
             steps for a problem with 3, goes on to one with 2 (a skip, not a stop);
  seed1/3    K = 8..20 with 1 and 3 seeding slots (admission from ST_WAIT one at a time);
at d = 32, 64 (pair mode) and 128, with n = 2503
(m = 2002: no multiple of 4, 16 or 64), H = 2; and at d = 128
  bigm       n = 12 000, H = 1, K = 9 and 20: m = 9600, a wave's compare segment is 1200 rows,
             two 1024-row batches of which the second is partial.
The blobs touch (as in test_gpu_kmeans_postsweep.py), so that every K runs Lloyd iterations past
the first dense ones.

The fixture is written by tests/golden/make_schedule.py, on the GPU, with the library of that
commit; the generator also checks that the capacity rules did bind in the capacity cases.
"""
import contextlib
import hashlib
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN, digest
from tests.test_gpu_kmeans import blobs, run_gpu

pytestmark = pytest.mark.gpu

SCHEDULE_GOLDEN = "engine/schedule_parent.npz"  # under tests/golden/ (see test_gpu_kmeans_postsweep.py)
K_TRUE, FRAC, SEED = 8, 0.8, 5
STD = {128: 12.0, 64: 3.0, 32: 3.0}  # cluster_std of the blobs by d
KS_WIDE = list(range(8, 21))
N_SMALL, N_BIG = 2503, 12000
STAT_NAMES = ("lloyd", "seed", "mrows", "reloc", "sweeps", "ctiles", "sparse", "changes")

# name -> (Ks, n_init, seedmax, share, n, H)
KINDS = {
    "seedcap": (KS_WIDE, 3, 32, False, N_SMALL, 2),
    "share": (KS_WIDE, 3, 32, True, N_SMALL, 2),
    "lloydcap": ([2, 3, 4], 16, 32, True, N_SMALL, 2),
    "seed1": (KS_WIDE, 3, 1, True, N_SMALL, 2),
    "seed3": (KS_WIDE, 3, 3, True, N_SMALL, 2),
    "bigm": ([9, 20], 3, 32, True, N_BIG, 1),
}
CAPACITY_KINDS = ("seedcap", "share", "lloydcap")  # their sweeps are more than any one K's alone
CASES = [(kind, d) for d in (128, 64, 32) for kind in KINDS if kind != "bigm"] + [("bigm", 128)]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


_data = {}


def case_data(n, d):
    if (n, d) not in _data:
        _data[n, d] = blobs(n, d, K_TRUE, seed=n + d, std=STD[d])
    return _data[n, d]


@contextlib.contextmanager
def launch_env(seedmax, share, env=os.environ):
    new = {"CCMI_NSUB": "1", "CCMI_SEEDMAX": str(seedmax), "CCMI_KM_SHARE_SEED": "1" if share else "0"}
    old = {k: env.get(k) for k in new}
    env.update(new)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                env.pop(k, None)
            else:
                env[k] = v


def run_case(kind, d, Ks=None):
    """What the fixture stores of one case (of its K list, or of the K list given)."""
    ks, n_init, seedmax, share, n, H = KINDS[kind]
    Ks = ks if Ks is None else Ks
    with launch_env(seedmax, share):
        _, labs, inert, nit, stats = run_gpu(case_data(n, d), Ks, H, FRAC, SEED, n_init=n_init)
    return dict(labels_sha256=np.array([_sha(labs[k].astype(np.uint8)) for k in range(labs.shape[0])]),
                inertia_bits=np.ascontiguousarray(inert).view(np.uint32).copy(),
                n_iter=nit.astype(np.int32), stats=stats[:8].astype(np.int64))


def fixture_key(kind, d):
    return f"{kind}_d{d}_"


FIELDS = ("labels_sha256", "inertia_bits", "n_iter", "stats")


@pytest.mark.parametrize("kind,d", CASES)
def test_schedule_is_pinned(kind, d):
    z = np.load(os.path.join(GOLDEN, SCHEDULE_GOLDEN), allow_pickle=False)
    n = KINDS[kind][4]
    assert digest(case_data(n, d)) == str(z[f"d{d}_n{n}_x_sha256"])
    got = run_case(kind, d)
    key = fixture_key(kind, d)
    print(f"{kind} d={d}: " + ", ".join(f"{s} {int(v)}" for s, v in zip(STAT_NAMES, got["stats"])) +
          f"; parent sweeps {int(z[key + 'stats'][4])}, n_iter {got['n_iter'].tolist()}")
    for name in FIELDS:
        np.testing.assert_array_equal(got[name], z[key + name], err_msg=key + name)
