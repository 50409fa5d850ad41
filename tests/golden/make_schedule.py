"""Pin the sweep scheduler of the d <= 128 k-means engine: tests/golden/engine/schedule_parent.npz.

Like make_postsweep.py this records the ENGINE's own output, here of the library before the
scheduler moved from one thread to a wave and the label compare kept its loads in flight.  It
needs a GPU, and it is only meaningful when run with the library of the commit named in the
file's ``commit`` entry:

    python tests/golden/make_schedule.py COMMIT [OUT.npz]

The cases and what is stored per case (per K the labels' sha256, inertia as float32 bits, n_iter,
the engine's counters stats[0:8], and the digest of X) are those of
tests/test_gpu_kmeans_schedule.py.  The generator fails unless the cases exercise what the test
relies on: every d = 128 case must have had sparse item-sweeps (stats[6] > 0), and every capacity
case must have swept more often than any one of its K run alone (summed over the resamples): were
no capacity rule binding, the unit would need only as many sweeps as its slowest K.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.conftest import digest  # noqa: E402
from tests import test_gpu_kmeans_schedule as T  # noqa: E402


def main(commit, out=os.path.join(HERE, T.SCHEDULE_GOLDEN)):
    arrays = dict(commit=np.array(commit))
    problems = []
    for kind, d in T.CASES:
        Ks, _, _, _, n, _ = T.KINDS[kind]
        arrays[f"d{d}_n{n}_x_sha256"] = np.array(digest(T.case_data(n, d)))
        got = T.run_case(kind, d)
        print(f"{kind} d={d}: " + ", ".join(f"{s} {int(v)}" for s, v in zip(T.STAT_NAMES, got["stats"])) +
              f" n_iter={got['n_iter'].tolist()}", flush=True)
        for name in T.FIELDS:
            arrays[T.fixture_key(kind, d) + name] = got[name]
        if d == 128 and not got["stats"][6] > 0:
            problems.append(f"{kind} d={d}: no sparse item-sweep")
        if kind in T.CAPACITY_KINDS:
            alone = [int(T.run_case(kind, d, [K])["stats"][4]) for K in Ks]
            print(f"  sweeps of each K alone: {alone}", flush=True)
            if not int(got["stats"][4]) > max(alone):
                problems.append(f"{kind} d={d}: {int(got['stats'][4])} sweeps, no more than a K alone ({max(alone)})")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")
    for line in problems:
        print("PROBLEM", line)
    assert not problems, "the cases do not meet what the test asserts of them"


if __name__ == "__main__":
    main(*sys.argv[1:3])
