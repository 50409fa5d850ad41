"""Timing of the PAM base clusterer on the device at a C2-like shape: n = 10 000,
d = 64 blobs (float32), subsampling 0.8 (m = 8000), K = 2..15, H = 64, metric correlation.

    python tools/pam_time.py [OUT.txt] [--fits 3] [--host-resamples 16] [--no-host] [--small]

One warm-up fit, then `fits` timed fits: the stage times of `fit` (wall clocks between
synchronisations, `timings_`), and HIP events around cc_pam_build, the SWAP loop and cc_pam_labels.
cc_pam_build streams 8 m^2 bytes per tree and step in its gain pass, so 8 m^2 * Kmax * H bytes
over the time of the whole call (the small pick kernels and the problem set-up included) is a
lower bound of the gain pass's rate; the pass alone comes from a kernel trace (--trace-fit runs
one warm-up and one fit and nothing else, for `rocprofv3 --kernel-trace --stats -- python
tools/pam_time.py --trace-fit`).

The host PAM on 16 workers is timed on a sample of the same fit's problems: the first
`host-resamples` resamples at K = 2, 8 and 15 through api.host_fit_predict(n_jobs=16), and their
labels are compared with the device's.  Prints every line and, with a file argument, also writes
it to that file.  --small: a toy shape to rehearse the script."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sklearn.datasets import make_blobs  # noqa: E402

from consensus_clustering_amd import PAM, ConsensusClustering, api, engine  # noqa: E402

_p = argparse.ArgumentParser()
_p.add_argument("out", nargs="?")
_p.add_argument("--fits", type=int, default=3)
_p.add_argument("--host-resamples", type=int, default=16)
_p.add_argument("--no-host", action="store_true")
_p.add_argument("--trace-fit", action="store_true")
_p.add_argument("--small", action="store_true")
OPT = _p.parse_args()
OUT = open(OPT.out, "w") if OPT.out else None
N, D_, H = (600, 16, 8) if OPT.small else (10_000, 64, 64)
Ks = list(range(2, 16))
HBM_PEAK = 8.0e12


class HostPAM(PAM):
    """A subclass: the host loop."""


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    if OUT is not None:
        OUT.write(s + "\n")
        OUT.flush()


def fit(X):
    cc = ConsensusClustering(clusterer=PAM(metric="correlation"), clusterer_options={}, K_range=Ks, n_iterations=H,
                             subsampling=0.8, random_state=0, plot_cdf=False, keep_matrices=False)
    torch.cuda.synchronize()
    t = time.perf_counter()
    cc.fit(X)
    torch.cuda.synchronize()
    return cc, (time.perf_counter() - t) * 1e3


def spread(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    X, _ = make_blobs(n_samples=N, n_features=D_, centers=6, cluster_std=1.0, center_box=(-10, 10), shuffle=True,
                      random_state=0)
    X = X.astype(np.float32)
    m = int(0.8 * N)
    cc, _ = fit(X)  # warm-up
    if OPT.trace_fit:
        fit(X)
        return
    say(f"== C2-like: n={N} d={D_} {X.dtype} blobs, subsampling 0.8 (m={m}), K={Ks[0]}..{Ks[-1]}, H={H}, PAM "
        f"metric correlation; {torch.cuda.get_device_name()}")
    say(f"plan {cc.pam_stats_}; swaps per problem: max {int(cc.pam_n_iter_.max())}, mean "
        f"{float(cc.pam_n_iter_.float().mean()):.2f}")
    wall, stages, kern = [], {}, {}
    for _ in range(OPT.fits):
        engine.TIMERS = {}
        cc, w = fit(X)
        summary = engine.timer_summary(engine.TIMERS)
        engine.TIMERS = None
        wall.append(w)
        for k, v in cc.timings_.items():
            stages.setdefault(k, []).append(v * 1e3)
        for k, (_, ms) in summary.items():
            kern.setdefault(k, []).append(ms)
    say(f"median (min .. max) of {OPT.fits} fits after 1 warm-up fit, ms")
    say(f"fit wall {spread(wall)}")
    say("fit stages (timings_):", {k: spread(v) for k, v in stages.items()})
    say("HIP events, summed over the launches of a fit:", {k: spread(v) for k, v in kern.items()})
    nbytes = 8 * m * m * max(Ks) * H
    t_build = statistics.median(kern["cc_pam_build"]) * 1e-3
    say(f"BUILD: {max(Ks)} steps x {H} trees x 8 m^2 = {nbytes / 1e9:.1f} GB streamed by the gain pass; over the whole "
        f"cc_pam_build call ({t_build * 1e3:.1f} ms, pick and set-up kernels included) that is at least "
        f"{nbytes / t_build / 1e12:.2f} TB/s = {100 * nbytes / t_build / HBM_PEAK:.0f} % of the 8 TB/s HBM peak")
    if OPT.no_host:
        return
    nh = min(OPT.host_resamples, H)
    idx = cc.resampling_indices_[:nh]
    L = cc.labels_.cpu().numpy()
    total = 0.0
    for K in (2, 8, 15):
        t = time.perf_counter()
        lab = api.host_fit_predict(HostPAM(n_clusters=K, metric="correlation"), X, idx, 16, "multiprocessing")
        dt = time.perf_counter() - t
        total += dt
        same = all(np.array_equal(L[Ks.index(K), idx[h], h], lab[h]) for h in range(nh))
        say(f"host PAM, 16 workers, K={K}: {nh} resamples in {dt:.1f} s; labels equal to the device's: {same}")
    scale = (H / nh) * (len(Ks) / 3)
    say(f"host sample: {total:.1f} s for {3 * nh} of the fit's {H * len(Ks)} problems; scaled by {scale:.1f} (mean over "
        f"the three K) the host clustering stage of the whole fit is about {total * scale:.0f} s on 16 workers, "
        f"against {statistics.median(stages['cluster']) / 1e3:.2f} s on the device (an estimate, not a measured fit)")


if __name__ == "__main__":
    main()
