"""Timing of feature subsampling on the device trees: `fit` with
feature_subsampling = 0.8 against 1.0 on the same build at the parity-blobs shape (n = 3000,
d = 32, float32, K = 2..12, H = 60, average linkage, correlation), the stage split of the 0.8 fit
from HIP events, and the 16-worker host loop with the same column subsets.

    python tools/features_time.py [OUT.txt] [--rounds 9] [--no-host]

Three warm-up fits of each setting, then `rounds` rounds; the two settings alternate inside a
round and the round's order flips from one round to the next.  Every fit is timed twice: HIP
events around it on the current stream and a wall clock between two synchronisations.  Prints
every line and, with a file argument, also writes it to that file.

The two kernels of cc_pdist_batched run inside one call, so HIP events around the call give
their sum; their split comes from a kernel trace (--trace-fit runs two 0.8 fits and nothing else,
for `rocprofv3 --kernel-trace --stats -- python tools/features_time.py --trace-fit`)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sklearn.cluster import AgglomerativeClustering  # noqa: E402
from sklearn.datasets import make_blobs  # noqa: E402

from consensus_clustering_amd import ConsensusClustering, engine  # noqa: E402

_p = argparse.ArgumentParser()
_p.add_argument("out", nargs="?")
_p.add_argument("--rounds", type=int, default=9)
_p.add_argument("--no-host", action="store_true")
_p.add_argument("--trace-fit", action="store_true")
OPT = _p.parse_args()
OUT = open(OPT.out, "w") if OPT.out else None
ROUNDS = OPT.rounds
Ks, H = list(range(2, 13)), 60


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    if OUT is not None:
        OUT.write(s + "\n")
        OUT.flush()


def fit(X, fraction, how="device", n_jobs=1):
    """(estimator, HIP-event ms, synchronised wall ms) of one fit."""
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="average", metric="correlation"),
                             clusterer_options={}, K_range=Ks, n_iterations=H, subsampling=0.8, random_state=0,
                             plot_cdf=False, hierarchical=how, n_jobs=n_jobs, keep_matrices=False,
                             feature_subsampling=fraction)
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
    X, _ = make_blobs(n_samples=3000, n_features=32, centers=6, cluster_std=1.0, center_box=(-10, 10),
                      shuffle=True, random_state=0)
    X = X.astype(np.float32)
    if OPT.trace_fit:
        fit(X, 0.8)
        fit(X, 0.8)
        return
    say(f"== parity blobs: n={X.shape[0]} d={X.shape[1]} {X.dtype} K={Ks[0]}..{Ks[-1]} H={H} average linkage, "
        f"correlation; {torch.cuda.get_device_name()}")
    for _ in range(3):
        fit(X, 0.8)
        fit(X, 1.0)
    ev = {0.8: [], 1.0: []}
    wall = {0.8: [], 1.0: []}
    cluster = {0.8: [], 1.0: []}
    last = {}
    for r in range(ROUNDS):
        for f in ((0.8, 1.0) if r % 2 == 0 else (1.0, 0.8)):
            cc, e, w = fit(X, f)
            ev[f].append(e)
            wall[f].append(w)
            cluster[f].append(cc.timings_["cluster"] * 1e3)
            last[f] = cc
    say(f"median (min .. max) of {ROUNDS} fits, ms; 3 warm-up fits each; the settings alternate inside a round")
    for f in (0.8, 1.0):
        say(f"feature_subsampling={f}: HIP events {spread(ev[f])}, wall {spread(wall[f])}, "
            f"cluster stage (wall) {spread(cluster[f])}; plan {last[f].hc_stats_}")
    say(f"ratio 0.8 / 1.0 of the medians: HIP events {statistics.median(ev[0.8]) / statistics.median(ev[1.0]):.3f}, "
        f"cluster stage {statistics.median(cluster[0.8]) / statistics.median(cluster[1.0]):.3f}")
    for f in (0.8, 1.0):
        runs = []
        for _ in range(3):
            engine.TIMERS = {}
            fit(X, f)
            runs.append(engine.timer_summary(engine.TIMERS))
            engine.TIMERS = None
        say(f"stages of the {f} fit from HIP events, (launches, median ms of 3 fits):",
            {k: (runs[0][k][0], round(statistics.median(r[k][1] for r in runs), 2)) for k in runs[0]})
    if not OPT.no_host:
        for rep in range(2):
            ch, _, w = fit(X, 0.8, how="host", n_jobs=16)
            say(f"host loop n_jobs=16, feature_subsampling=0.8, run {rep}: wall {w:.0f} ms, cluster stage "
                f"{ch.timings_['cluster'] * 1e3:.0f} ms")
        same = all(np.array_equal(last[0.8].pair_counts_[K], ch.pair_counts_[K]) for K in Ks)
        say(f"pair counts of the device and the host fit identical: {same}; the host cluster stage is "
            f"{ch.timings_['cluster'] * 1e3 / statistics.median(cluster[0.8]):.1f}x the device's")


if __name__ == "__main__":
    main()
