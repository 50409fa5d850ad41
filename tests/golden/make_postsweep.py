"""Pin the post-sweep phase of the d <= 128 k-means engine: tests/golden/engine/postsweep_parent.npz.

Like make_narrow_reloc.py this records the ENGINE's own output, here of the library before the
post-sweep element-wise passes were restructured (parent commit c49cbe8 plus the CCMI_KM_LSEG
knob, which changes nothing in the kernel).  It needs a GPU, and it is only meaningful when run with the library of the commit named in the
file's ``commit`` entry:

    python tests/golden/make_postsweep.py COMMIT [OUT.npz]

The cases and what is stored per run (per K the labels' sha256, inertia as float32 bits, n_iter,
and the digest of X) are those of tests/test_gpu_kmeans_postsweep.py.  Every d = 128 run must
have had sparse item-sweeps (stats[6] > 0), the packed and the alone runs of a K must agree, and
the small capacity must change no label for K <= the number of blobs.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.conftest import digest  # noqa: E402
from tests import test_gpu_kmeans_postsweep as T  # noqa: E402


def main(commit, out=os.path.join(HERE, T.POSTSWEEP_GOLDEN)):
    arrays = dict(commit=np.array(commit))
    problems = []
    for n in T.NS_SPARSE:
        arrays[f"d128_n{n}_x_sha256"] = np.array(digest(T.case_data(n, 128)))
        runs = {lseg: T.sparse_runs(n, lseg) for lseg in T.LSEGS}
        for lseg, rr in runs.items():
            for run, (got, labs) in rr.items():
                print(f"n={n} lseg={lseg} run={run}: sparse item-sweeps {int(got['sparse_item_sweeps'])} "
                      f"n_iter={got['n_iter'].tolist()}", flush=True)
                if not got["sparse_item_sweeps"] > 0:
                    problems.append(f"n={n} lseg={lseg} run={run}: no sparse item-sweep (drop the case)")
                for name in ("labels_sha256", "inertia_bits", "n_iter"):
                    arrays[T.fixture_key(n, 128, lseg, run) + name] = got[name]
            for k, K in enumerate(T.KS_SPARSE):
                for name in ("labels_sha256", "inertia_bits", "n_iter"):
                    if not np.array_equal(rr["all"][0][name][k], rr[K][0][name][0]):
                        problems.append(f"n={n} lseg={lseg} K={K} {name}: packed and alone runs differ")
        for lseg in T.LSEGS[1:]:
            differ = []
            for k, K in enumerate(T.KS_SPARSE):
                same = np.array_equal(runs[lseg]["all"][1][k], runs[0]["all"][1][k])
                bits = np.array_equal(runs[lseg]["all"][0]["inertia_bits"][k], runs[0]["all"][0]["inertia_bits"][k])
                if not (same or K > T.K_TRUE):
                    problems.append(f"n={n} lseg={lseg} K={K}: the capacity changed a label")
                differ.append((K, same, bits))
            print(f"n={n} lseg={lseg} against the default capacity (K, labels equal, inertia bits equal): {differ}")
    for d, n in T.NARROW:
        arrays[f"d{d}_n{n}_x_sha256"] = np.array(digest(T.case_data(n, d)))
        got = T.narrow_run(d, n)
        print(f"d={d} n={n}: n_iter={got['n_iter'].tolist()}", flush=True)
        for name in ("labels_sha256", "inertia_bits", "n_iter"):
            arrays[T.fixture_key(n, d, 0, "all") + name] = got[name]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")
    for line in problems:
        print("PROBLEM", line)
    assert not problems, "the cases do not meet what the test asserts of them"


if __name__ == "__main__":
    main(*sys.argv[1:3])
