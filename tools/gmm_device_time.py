"""Timing of the GMM base clusterer on the device at the float64 C2-like shape of
tools/features_f64_time.py: n = 10 000, d = 64 blobs (float64), subsampling 0.8 (m = 8000),
K = 2..15, H = 64, n_init 1 and 3.

    python tools/gmm_device_time.py [OUT.txt] [--fits 3] [--no-host] [--small] [--full]

Per n_init: one warm-up fit, then `fits` timed fits of ConsensusClustering(clusterer=GMM()): the
clustering stage (`timings_['cluster']`, a wall clock between synchronisations) and HIP events
around every kernel group and around the k-means initialisation (engine.timed).  Then the same fit
on the host, once each: the 16-worker host loop of the same GMM (a subclass, so `backend_` is
'host-clusterer') and of sklearn's GaussianMixture(covariance_type='diag'), both on the same
resamples; the host GMM fit's pair counts are compared with the device fit's.  Prints every line
and, with a file argument, also writes it to that file.  --small: a toy shape to rehearse the
script.  --full: the full-covariance model (FullGMM) against its own host loop and
sklearn's GaussianMixture(covariance_type='full'); where the pair counts differ, the problems
whose labels differ are listed with the device's and a host refit's n_iter and lower bound."""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sklearn.datasets import make_blobs  # noqa: E402
from sklearn.mixture import GaussianMixture  # noqa: E402

from consensus_clustering_amd import GMM, ConsensusClustering, FullGMM, engine  # noqa: E402

_p = argparse.ArgumentParser()
_p.add_argument("out", nargs="?")
_p.add_argument("--fits", type=int, default=3)
_p.add_argument("--no-host", action="store_true")
_p.add_argument("--small", action="store_true")
_p.add_argument("--full", action="store_true")
OPT = _p.parse_args()
OUT = open(OPT.out, "w") if OPT.out else None
N, D_, H = (600, 16, 8) if OPT.small else (10_000, 64, 64)
Ks = list(range(2, 16))


class HostGMM(GMM):
    """A subclass: the host loop."""


class HostFullGMM(FullGMM):
    """A subclass: the host loop."""


COV = 'full' if OPT.full else 'diag'
DEV, HOST = (FullGMM, HostFullGMM) if OPT.full else (GMM, HostGMM)


def differing(dev, host, X, n_init, limit=8, also=()):
    """The (K, h) problems whose labels differ between the device fit and a host fit, and for the
    first `limit` the device's n_iter and bound next to a host refit's (the device fit's seed,
    rows and columns).  also: (k, h) problems listed whether they differ or not; the --small
    rehearsal passes one, so that this report runs even though nothing differs."""
    a, b = dev.labels_.cpu().numpy(), host.labels_.cpu().numpy()
    idx, cols = dev.resampling_indices_, dev.feature_indices_
    where = [(k, h) for k in range(len(Ks)) for h in range(H) if not np.array_equal(a[k, :, h], b[k, :, h])]
    say(f"   labels differ in {len(where)} of {len(Ks) * H} problems: (K, h) {[(Ks[k], h) for k, h in where]}")
    for k, h in (list(also) + where)[:limit]:
        rows = X[idx[h]] if cols is None else X[idx[h]][:, cols[h]]
        ref = DEV(n_components=Ks[k], n_init=n_init, random_state=dev.random_state).fit(rows)
        nd = int((a[k, idx[h], h] != b[k, idx[h], h]).sum())
        lb = float(dev.gmm_lower_bound_[k, h])
        say(f"   K={Ks[k]} h={h}: {nd} of {idx.shape[1]} rows differ; device n_iter {int(dev.gmm_n_iter_[k, h])} "
            f"bound {lb!r}; host n_iter {ref.n_iter_} bound {ref.lower_bound_!r} (relative difference "
            f"{abs(lb - ref.lower_bound_) / abs(ref.lower_bound_):.2e}, tol 1e-3 on the bound's change)")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    if OUT is not None:
        OUT.write(s + "\n")
        OUT.flush()


def fit(X, est, n_init, n_jobs=1):
    cc = ConsensusClustering(clusterer=est, clusterer_options={'n_init': n_init}, K_range=Ks, n_iterations=H,
                             subsampling=0.8, random_state=0, plot_cdf=False, keep_matrices=False, n_jobs=n_jobs,
                             parallelization_method='multiprocessing')
    torch.cuda.synchronize()
    t = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # sklearn's ConvergenceWarning in the host loops
        cc.fit(X)
    torch.cuda.synchronize()
    return cc, (time.perf_counter() - t) * 1e3


def spread(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    X, _ = make_blobs(n_samples=N, n_features=D_, centers=6, cluster_std=1.0, center_box=(-10, 10), shuffle=True,
                      random_state=0)
    X = X.astype(np.float32).astype(np.float64)
    m = int(0.8 * N)
    say(f"== float64 C2-like: n={N} d={D_} {X.dtype} blobs, subsampling 0.8 (m={m}), K={Ks[0]}..{Ks[-1]}, H={H}, "
        f"{DEV.__name__} ({COV}, tol 1e-3, max_iter 100); {torch.cuda.get_device_name()}")
    for n_init in (1, 3):
        cc, _ = fit(X, DEV(), n_init)  # warm-up
        assert cc.backend_ == "gpu-gmm" and cc.gmm_covariance_type_ == COV
        say(f"-- n_init={n_init}: plan {cc.gmm_stats_}; EM iterations per problem (winning init): max "
            f"{int(cc.gmm_n_iter_.max())}, mean {float(cc.gmm_n_iter_.float().mean()):.2f}; converged "
            f"{int(cc.gmm_converged_.sum())} of {cc.gmm_converged_.numel()}")
        wall, stages, kern = [], {}, {}
        for _ in range(OPT.fits):
            engine.TIMERS = {}
            cc, w = fit(X, DEV(), n_init)
            summary = engine.timer_summary(engine.TIMERS)
            engine.TIMERS = None
            wall.append(w)
            for k, v in cc.timings_.items():
                stages.setdefault(k, []).append(v * 1e3)
            for k, (_, ms) in summary.items():
                kern.setdefault(k, []).append(ms)
        say(f"device: median (min .. max) of {OPT.fits} fits after 1 warm-up fit, ms")
        say(f"fit wall {spread(wall)}; cluster stage (timings_['cluster']) {spread(stages['cluster'])}")
        say("HIP events, summed over the launches of a fit:", {k: spread(v) for k, v in kern.items()})
        if OPT.no_host:
            continue
        dev_s = statistics.median(stages['cluster']) / 1e3
        host, w = fit(X, HOST(), n_init, n_jobs=16)
        assert host.backend_ == "host-clusterer"
        same = all(np.array_equal(cc.pair_counts_[K], host.pair_counts_[K]) for K in Ks)
        host_s = host.timings_['cluster']
        say(f"host {DEV.__name__} (gmm.py), 16 workers: cluster stage {host_s:.2f} s, {H * len(Ks) / host_s:.0f} resample-fits/s; "
            f"pair counts identical to the device fit's: {same}")
        if not same or OPT.small:
            differing(cc, host, X, n_init, also=[(len(Ks) - 1, H - 1)] if OPT.small else ())
        sk, w = fit(X, GaussianMixture(covariance_type=COV), n_init, n_jobs=16)
        assert sk.backend_ == "host-clusterer"
        sk_s = sk.timings_['cluster']
        same_sk = all(np.array_equal(cc.pair_counts_[K], sk.pair_counts_[K]) for K in Ks)
        say(f"sklearn GaussianMixture('{COV}'), 16 workers: cluster stage {sk_s:.2f} s, {H * len(Ks) / sk_s:.0f} "
            f"resample-fits/s; pair counts identical to the device fit's: {same_sk}")
        if not same_sk:
            differing(cc, sk, X, n_init, limit=0)
        say(f"device cluster stage {dev_s:.3f} s, {H * len(Ks) / dev_s:.0f} resample-fits/s: {host_s / dev_s:.1f}x the "
            f"16-worker host {DEV.__name__}, {sk_s / dev_s:.1f}x the 16-worker sklearn loop (host runs measured once)")


if __name__ == "__main__":
    main()
