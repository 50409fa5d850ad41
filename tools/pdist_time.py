"""Timing of cc_pdist: every metric beside cc_euclidean at n = 8000, d = 128,
float32, HIP events around single launches (warm-up, then the median of repeated launches, the
metrics alternating inside a round), and the blobs_n400_d8_k4 fit with
AgglomerativeClustering(linkage='average', metric='correlation') on the device against the host
loop.

    python tools/pdist_time.py [OUT.txt]

Prints every line and, with an argument, also writes it to that file."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sklearn.cluster import AgglomerativeClustering  # noqa: E402

from consensus_clustering_amd import ConsensusClustering, _lib, engine  # noqa: E402

OUT = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    if OUT is not None:
        OUT.write(s + "\n")
        OUT.flush()


def kernels(n=8000, d=128, warmup=3, reps=15):
    say(f"== cc_pdist beside cc_euclidean: n={n} d={d}, one launch each, HIP events, warm-up {warmup}, "
        f"median (min .. max) of {reps}")
    rs = np.random.RandomState(0)
    Xh = rs.randn(n, d).astype(np.float32)
    X32 = torch.from_numpy(Xh).cuda()
    X64c = torch.from_numpy(Xh.astype(np.float64) - Xh.astype(np.float64).mean(axis=1, keepdims=True)).cuda()
    D = torch.empty((n, n), dtype=torch.float64, device="cuda")
    norms = torch.empty(n, dtype=torch.float64, device="cuda")
    st = engine.stream_ptr()
    runs = {
        "cc_euclidean f32": lambda: _lib.call("cc_euclidean", X32.data_ptr(), 0, n, d, D.data_ptr(), st),
        "cc_pdist cityblock f32": lambda: _lib.call("cc_pdist", X32.data_ptr(), 0, n, d, 1, D.data_ptr(), None, st),
        "cc_pdist cosine f32 (norms + tiles)": lambda: _lib.call("cc_pdist", X32.data_ptr(), 0, n, d, 2,
                                                                  D.data_ptr(), norms.data_ptr(), st),
        "cc_pdist cosine f64 centred rows (correlation)": lambda: _lib.call(
            "cc_pdist", X64c.data_ptr(), 1, n, d, 2, D.data_ptr(), norms.data_ptr(), st),
    }
    times = {k: [] for k in runs}
    for rep in range(warmup + reps):
        for name, f in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            if rep >= warmup:
                times[name].append(a.elapsed_time(b))
    base = statistics.median(times["cc_euclidean f32"])
    for name, t in times.items():
        med = statistics.median(t)
        say(f"{name}: {med:.3f} ms ({min(t):.3f} .. {max(t):.3f}), {med / base:.2f}x cc_euclidean")
    torch.cuda.synchronize()
    t = time.perf_counter()
    engine.pdist(X32, "correlation")
    torch.cuda.synchronize()
    say(f"engine.pdist(X, 'correlation') from a device tensor, with the host centring and both copies: "
        f"{(time.perf_counter() - t) * 1e3:.1f} ms wall")


def fixture_fit():
    z = np.load(os.path.join(ROOT, "tests", "golden", "blobs_n400_d8_k4.npz"), allow_pickle=False)
    X = np.ascontiguousarray(z["X"], dtype=np.float32)
    say(f"== blobs_n400_d8_k4 float32, AgglomerativeClustering(linkage='average', metric='correlation'), "
        "K=2..7 H=24 subsampling 0.8: wall time of fit, median of the runs after a warm-up")

    def fit(how):
        cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage="average", metric="correlation"),
                                 clusterer_options={}, K_range=list(range(2, 8)), n_iterations=24, subsampling=0.8,
                                 random_state=3, plot_cdf=False, hierarchical=how)
        torch.cuda.synchronize()
        t = time.perf_counter()
        cc.fit(X)
        torch.cuda.synchronize()
        return cc, time.perf_counter() - t

    res = {}
    for how, reps in (("device", 7), ("host", 3)):
        fit(how)
        runs = [fit(how) for _ in range(reps)]
        res[how] = runs[0][0]
        ts = [t for _, t in runs]
        say(f"hierarchical='{how}' ({runs[0][0].backend_}): {statistics.median(ts) * 1e3:.1f} ms "
            f"({min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f}), cluster stage "
            f"{statistics.median(c.timings_['cluster'] for c, _ in runs) * 1e3:.1f} ms")
    same = all(np.array_equal(res["device"].pair_counts_[K], res["host"].pair_counts_[K]) for K in range(2, 8))
    say(f"pair counts identical: {same}")


if __name__ == "__main__":
    kernels()
    fixture_fit()
