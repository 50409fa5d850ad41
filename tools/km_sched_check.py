"""Diagnostic: the wave scheduler of the d <= 128 k-means engine against the serial reference.

Builds libccmi_schedcheck.so (-DCC_KM_SCHED_CHECK) next to the package unless it is already there
(`--rebuild` forces it; build it where there is no GPU, the run then only loads it).  In that
build every sweep also runs the serial schedule() on a copy of the engine state, and every 32-bit
word of the two states is compared: stats[122] counts the words that differ, stats[123] the sweeps
compared.  Runs the cases of tests/test_gpu_kmeans_schedule.py and C3 at H = 8; exits non-zero on
a mismatch.

    python tools/km_sched_check.py [--rebuild] [--build-only]
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "consensus_clustering_amd")
LIB = os.path.join(PKG, os.environ.get("KM_SCHED_CHECK_LIB", "libccmi_schedcheck.so"))
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -falign-loops=64 -DCC_KM_SCHED_CHECK"

if "--rebuild" in sys.argv or not os.path.exists(LIB):
    subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", str(min(16, os.cpu_count() or 1)),
                    "HIPFLAGS=" + FLAGS + " " + os.environ.get("KM_SCHED_CHECK_EXTRA", ""),
                    "OUT=" + LIB, "BUILD=../../build/ccmi_schedcheck"], check=True)
if "--build-only" in sys.argv:
    sys.exit(0)

os.environ["CCMI_LIB"] = LIB
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import CONFIGS, SEED, make_blobs_f32  # noqa: E402
from consensus_clustering_amd import engine  # noqa: E402
from consensus_clustering_amd.kmeans import BatchedKMeans, prepare_rows  # noqa: E402
from tests import test_gpu_kmeans_schedule as T  # noqa: E402
from tests.test_gpu_kmeans import run_gpu  # noqa: E402

total = 0
for kind, d in T.CASES:
    Ks, n_init, seedmax, share, n, H = T.KINDS[kind]
    with T.launch_env(seedmax, share):
        stats = run_gpu(T.case_data(n, d), Ks, H, T.FRAC, T.SEED, n_init=n_init)[4]
    print(f"{kind} d={d}: sweeps {int(stats[4])}, compared {int(stats[123])}, words that differ {int(stats[122])}",
          flush=True)
    assert stats[123] == stats[4], "the check did not run every sweep"
    total += int(stats[122])

cfg, H = CONFIGS["c3"], 8
dev = engine.require_gpu()
X = make_blobs_f32(cfg["n"], cfg["d"], cfg["k_true"], seed=SEED)
n, d = X.shape
m = int(cfg["frac"] * n)
idx_d = torch.from_numpy(engine.resample_indices(SEED, n, m, 0, H)).to(dev)
Xd, xn, _, Xhl, e = prepare_rows(X, dev)
L = engine.new_label_matrix(len(cfg["Ks"]), n, engine.pad_h(H), dev)
bk = BatchedKMeans(cfg["Ks"], n_init=3, random_state=SEED)
bk.run(Xd, xn, d, idx_d, n, H, m, 0, H, L, np.float32, Xhl=Xhl, scale_exp=e)
torch.cuda.synchronize()
stats = bk.stats.cpu().numpy()
print(f"c3 H={H}: sweeps {int(stats[4])}, compared {int(stats[123])}, words that differ {int(stats[122])}", flush=True)
assert stats[123] == stats[4], "the check did not run every sweep"
total += int(stats[122])
print("scheduler check:", "zero mismatches" if total == 0 else f"{total} WORDS DIFFER")
sys.exit(1 if total else 0)
