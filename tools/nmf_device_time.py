"""Timing of the NMF base clusterer on the device at the float64 C2-like shape of
tools/gmm_device_time.py with non-negative rows: n = 10 000, d = 64 (float64, the absolute values of
the blobs), subsampling 0.8 (m = 8000), K = 2..15, H = 64, n_init 1 and 3.

    python tools/nmf_device_time.py [OUT.txt] [--fits 3] [--no-host] [--small] [--one-fit]

Per n_init: one warm-up fit, then `fits` timed fits of ConsensusClustering(clusterer=NMF()): the
clustering stage (`timings_['cluster']`, a wall clock between synchronisations) and HIP events
around every kernel group (engine.timed).  Then the same fit on the host, once each: the 16-worker
host loop of the same NMF (a subclass, so `backend_` is 'host-clusterer') and, at n_init = 1, of
sklearn's NMF(init='random', solver='mu') wrapped with the label rule, both on the same resamples;
the host fits' pair counts are compared with the device fit's.  Prints every line and, with a file
argument, also writes it to that file.  --small: a toy shape to rehearse the script.  --one-fit: one
device fit at n_init = 1 and nothing else (the fit a kernel trace is taken of)."""
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

from consensus_clustering_amd import NMF, ConsensusClustering, engine  # noqa: E402
from consensus_clustering_amd.nmf import labels_of  # noqa: E402

_p = argparse.ArgumentParser()
_p.add_argument("out", nargs="?")
_p.add_argument("--fits", type=int, default=3)
_p.add_argument("--no-host", action="store_true")
_p.add_argument("--small", action="store_true")
_p.add_argument("--one-fit", action="store_true")
OPT = _p.parse_args()
OUT = open(OPT.out, "w") if OPT.out else None
N, D_, H = (600, 16, 8) if OPT.small else (10_000, 64, 64)
Ks = list(range(2, 16))


class HostNMF(NMF):
    """A subclass: the host loop."""


class SkNMF:
    """sklearn's NMF(init='random', solver='mu') with the label rule of nmf.py."""

    def __init__(self, n_components=1, random_state=None):
        self.n_components = n_components
        self.random_state = random_state

    def get_params(self, deep=True):
        return dict(n_components=self.n_components, random_state=self.random_state)

    def set_params(self, **params):
        for k, v in params.items():
            setattr(self, k, v)
        return self

    def fit_predict(self, X, y=None):
        from sklearn.decomposition import NMF as Sk

        sk = Sk(self.n_components, init='random', solver='mu', random_state=self.random_state)
        W = sk.fit_transform(X)
        return labels_of(W, sk.components_)


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    if OUT is not None:
        OUT.write(s + "\n")
        OUT.flush()


def fit(X, est, n_init, n_jobs=1):
    opts = {} if isinstance(est, SkNMF) else {'n_init': n_init}
    cc = ConsensusClustering(clusterer=est, clusterer_options=opts, K_range=Ks, n_iterations=H, subsampling=0.8,
                             random_state=0, plot_cdf=False, keep_matrices=False, n_jobs=n_jobs,
                             parallelization_method='multiprocessing')
    torch.cuda.synchronize()
    t = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # sklearn's ConvergenceWarning in the host loop
        cc.fit(X)
    torch.cuda.synchronize()
    return cc, (time.perf_counter() - t) * 1e3


def spread(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    X, _ = make_blobs(n_samples=N, n_features=D_, centers=6, cluster_std=1.0, center_box=(-10, 10), shuffle=True,
                      random_state=0)
    X = np.abs(X.astype(np.float32).astype(np.float64))
    m = int(0.8 * N)
    say(f"== float64 C2-like, non-negative: n={N} d={D_} {X.dtype} |blobs|, subsampling 0.8 (m={m}), K={Ks[0]}..{Ks[-1]}, "
        f"H={H}, NMF (tol 1e-4, max_iter 200); {torch.cuda.get_device_name()}")
    if OPT.one_fit:
        cc, w = fit(X, NMF(), 1)
        say(f"one fit, n_init=1: wall {w:.1f} ms, cluster stage {cc.timings_['cluster'] * 1e3:.1f} ms, plan {cc.nmf_stats_}")
        return
    for n_init in (1, 3):
        cc, _ = fit(X, NMF(), n_init)  # warm-up
        assert cc.backend_ == "gpu-nmf"
        say(f"-- n_init={n_init}: plan {cc.nmf_stats_}; iterations per problem (winning init): min "
            f"{int(cc.nmf_n_iter_.min())}, max {int(cc.nmf_n_iter_.max())}, mean "
            f"{float(cc.nmf_n_iter_.float().mean()):.2f}; converged {int(cc.nmf_converged_.sum())} of "
            f"{cc.nmf_converged_.numel()}")
        wall, stages, kern = [], {}, {}
        for _ in range(OPT.fits):
            engine.TIMERS = {}
            cc, w = fit(X, NMF(), n_init)
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
        host, w = fit(X, HostNMF(), n_init, n_jobs=16)
        assert host.backend_ == "host-clusterer"
        same = all(np.array_equal(cc.pair_counts_[K], host.pair_counts_[K]) for K in Ks)
        host_s = host.timings_['cluster']
        say(f"host NMF (nmf.py), 16 workers: cluster stage {host_s:.2f} s, {H * len(Ks) / host_s:.0f} resample-fits/s; "
            f"pair counts identical to the device fit's: {same}")
        if not same:
            a, b = cc.labels_.cpu().numpy(), host.labels_.cpu().numpy()
            where = [(Ks[k], h) for k in range(len(Ks)) for h in range(H) if not np.array_equal(a[k, :, h], b[k, :, h])]
            say(f"   labels differ in {len(where)} of {len(Ks) * H} problems: (K, h) {where[:40]}")
        line = f"device cluster stage {dev_s:.3f} s, {H * len(Ks) / dev_s:.0f} resample-fits/s: {host_s / dev_s:.1f}x the 16-worker host NMF"
        if n_init == 1:
            sk, w = fit(X, SkNMF(), 1, n_jobs=16)
            assert sk.backend_ == "host-clusterer"
            sk_s = sk.timings_['cluster']
            same_sk = all(np.array_equal(cc.pair_counts_[K], sk.pair_counts_[K]) for K in Ks)
            say(f"sklearn NMF(init='random', solver='mu') with the label rule, 16 workers: cluster stage {sk_s:.2f} s, "
                f"{H * len(Ks) / sk_s:.0f} resample-fits/s; pair counts identical to the device fit's: {same_sk}")
            line += f", {sk_s / dev_s:.1f}x the 16-worker sklearn loop"
        say(line + " (host runs measured once)")


if __name__ == "__main__":
    main()
