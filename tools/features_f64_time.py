"""Timing of feature subsampling on the float64 k-means (cc_kmeans_f64_cols): `fit`
of the default KMeans at a float64 C2-like shape (n = 10 000, d = 64, 6 blobs, K = 2..15, H = 64)
with feature_subsampling = 0.8 against 1.0 on the same build, and the 16-worker host loop on the
same column subsets.

    python tools/features_f64_time.py [OUT.txt] [--rounds 9] [--fractions 1.0,0.8] [--no-host]

Three warm-up fits of each setting, then `rounds` rounds; the settings alternate inside a round
and the round's order flips from one round to the next.  Every fit is timed twice: HIP events
around it on the current stream and a wall clock between two synchronisations.  Prints every line
and, with a file argument, also writes it to that file.  profiles/kmeans/features_f64_measure.txt
holds a session of these runs.

`--fractions 1.0` times the plain path alone: with CCMI_LIB naming another build of the library
(the parent commit's) the same tool times that build, for an alternating comparison.

The two setup kernels and the engine run inside one call, so HIP events around the call give their
sum; the split comes from a kernel trace (--trace-fit runs two fits of the first fraction and
nothing else, for `rocprofv3 --kernel-trace --stats -- python tools/features_f64_time.py --trace-fit`)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sklearn.datasets import make_blobs  # noqa: E402

from consensus_clustering_amd import ConsensusClustering, _lib  # noqa: E402

_p = argparse.ArgumentParser()
_p.add_argument("out", nargs="?")
_p.add_argument("--rounds", type=int, default=9)
_p.add_argument("--fractions", default="1.0,0.8")
_p.add_argument("--no-host", action="store_true")
_p.add_argument("--trace-fit", action="store_true")
OPT = _p.parse_args()
OUT = open(OPT.out, "a") if OPT.out else None
ROUNDS = OPT.rounds
FRACTIONS = [float(f) for f in OPT.fractions.split(",")]
Ks, H = list(range(2, 16)), 64


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    if OUT is not None:
        OUT.write(s + "\n")
        OUT.flush()


def fit(X, fraction, n_jobs=1, precision="auto"):
    """(estimator, HIP-event ms, synchronised wall ms) of one fit."""
    cc = ConsensusClustering(K_range=Ks, n_iterations=H, subsampling=0.8, random_state=0, plot_cdf=False,
                             n_jobs=n_jobs, keep_matrices=False, feature_subsampling=fraction, precision=precision)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    e0.record()
    cc.fit(X)
    e1.record()
    torch.cuda.synchronize()
    return cc, e0.elapsed_time(e1), (time.perf_counter() - t) * 1e3


def spread(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    X, _ = make_blobs(n_samples=10_000, n_features=64, centers=6, cluster_std=1.0, center_box=(-10, 10),
                      shuffle=True, random_state=0)
    X = X.astype(np.float32).astype(np.float64)
    if OPT.trace_fit:
        fit(X, FRACTIONS[0])
        fit(X, FRACTIONS[0])
        return
    say(f"== float64 C2-like: n={X.shape[0]} d={X.shape[1]} {X.dtype} K={Ks[0]}..{Ks[-1]} H={H} default KMeans; "
        f"{torch.cuda.get_device_name()}; library {_lib.LIB_PATH if 'CCMI_LIB' in os.environ else 'in-tree'} "
        f"({_lib.load().cc_build_id().decode()})")
    for _ in range(3):
        for f in FRACTIONS:
            fit(X, f)
    ev = {f: [] for f in FRACTIONS}
    wall = {f: [] for f in FRACTIONS}
    cluster = {f: [] for f in FRACTIONS}
    last = {}
    for r in range(ROUNDS):
        for f in (FRACTIONS if r % 2 == 0 else FRACTIONS[::-1]):
            cc, e, w = fit(X, f)
            assert cc.backend_ == "gpu-kmeans" and cc.precision_ == "f64"
            ev[f].append(e)
            wall[f].append(w)
            cluster[f].append(cc.timings_["cluster"] * 1e3)
            last[f] = cc
    say(f"median (min .. max) of {ROUNDS} fits, ms; 3 warm-up fits each; the settings alternate inside a round")
    for f in FRACTIONS:
        say(f"feature_subsampling={f}: HIP events {spread(ev[f])}, wall {spread(wall[f])}, "
            f"cluster stage (wall) {spread(cluster[f])}; columns "
            f"{X.shape[1] if last[f].feature_indices_ is None else last[f].feature_indices_.shape[1]}, "
            f"Lloyd iterations {int(last[f].kmeans_n_iter_.sum())}")
    if len(FRACTIONS) > 1:
        a, b = FRACTIONS[1], FRACTIONS[0]
        say(f"ratio {a} / {b} of the medians: HIP events {statistics.median(ev[a]) / statistics.median(ev[b]):.3f}, "
            f"cluster stage {statistics.median(cluster[a]) / statistics.median(cluster[b]):.3f}")
    sub = [f for f in FRACTIONS if f < 1]
    if sub and not OPT.no_host:
        f = sub[0]
        for rep in range(2):
            ch, _, w = fit(X, f, n_jobs=16, precision="fast")  # 'fast' keeps the host loop under feature subsampling
            assert ch.backend_ == "host-clusterer"
            say(f"host loop n_jobs=16, feature_subsampling={f}, run {rep}: wall {w:.0f} ms, cluster stage "
                f"{ch.timings_['cluster'] * 1e3:.0f} ms")
        same = all(np.array_equal(last[f].pair_counts_[K], ch.pair_counts_[K]) for K in Ks)
        say(f"pair counts of the device and the host fit identical: {same}; the host cluster stage is "
            f"{ch.timings_['cluster'] * 1e3 / statistics.median(cluster[f]):.1f}x the device's")


if __name__ == "__main__":
    main()
