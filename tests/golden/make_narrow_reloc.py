"""Pin the d <= 128 engine's empty-cluster relocation: tests/golden/engine/narrow_reloc.npz.

Unlike the other fixtures this one records the ENGINE's own output, because the expectation is
the engine's lowest-index tie rule (sklearn's order among tied farthest rows is numpy's
argpartition's, which is unspecified).  It needs a GPU, and it is only meaningful when run at
the commit named in the file's ``commit`` entry: build that commit's library, then

    python tests/golden/make_narrow_reloc.py COMMIT [OUT.npz]

The cases, the recipe and what is stored per case (labels uint8, inertia as float32 bits,
n_iter, the relocation counter, and the digest of X) are those of
tests/test_gpu_kmeans.py::test_narrow_relocation_is_pinned.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.conftest import digest  # noqa: E402
from tests.test_gpu_kmeans import NARROW_RELOC_GOLDEN, NARROW_RELOC_SEEDS, narrow_reloc_run  # noqa: E402


def main(commit, out=os.path.join(HERE, NARROW_RELOC_GOLDEN)):
    arrays = dict(commit=np.array(commit))
    for d, seeds in NARROW_RELOC_SEEDS.items():
        total = 0
        for seed in seeds:
            X, got = narrow_reloc_run(seed, d)
            key = f"d{d}_s{seed}_"
            arrays[key + "x_sha256"] = np.array(digest(X))
            for name, val in got.items():
                arrays[key + name] = val
            total += int(got["relocations"])
            print(f"d={d} seed={seed} n={X.shape[0]} relocations={got['relocations']} "
                  f"n_iter={got['n_iter'].tolist()}", flush=True)
        assert total > 0, f"d={d}: no relocation over {seeds}: swap in further seeds"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:3])
