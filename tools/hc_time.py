"""Timing of the hierarchical base clusterer: `fit` on the device against the
16-worker host path at two shapes (parity blobs n = 3000; m = 8000), the per-stage split from
HIP events, and the batched / grid-form crossover at m = 8000.

    python tools/hc_time.py [OUT.txt [--linkage]]

Prints every line and, with an argument, also writes it to that file.  --linkage times the tree
builders alone: the crossover and every form of the linkage loops (`linkage_forms`); CCMI_LIB
names another build of the library to time beside this one."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sklearn.cluster import AgglomerativeClustering  # noqa: E402
from sklearn.datasets import make_blobs  # noqa: E402

from consensus_clustering_amd import ConsensusClustering, engine  # noqa: E402

OUT = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    if OUT is not None:
        OUT.write(s + "\n")
        OUT.flush()


def fit(X, Ks, H, link, how, n_jobs=1):
    cc = ConsensusClustering(clusterer=AgglomerativeClustering(linkage=link), clusterer_options={},
                             K_range=Ks, n_iterations=H, subsampling=0.8, random_state=0, plot_cdf=False,
                             hierarchical=how, n_jobs=n_jobs, keep_matrices=False)
    torch.cuda.synchronize()
    t = time.perf_counter()
    cc.fit(X)
    torch.cuda.synchronize()
    return cc, time.perf_counter() - t


def shape(name, X, Ks, H, link):
    say(f"== {name}: n={X.shape[0]} d={X.shape[1]} {X.dtype} K={Ks[0]}..{Ks[-1]} H={H} linkage={link}")
    fit(X[:400], Ks[:2], 4, link, "device")  # warm-up: library load, allocator
    engine.TIMERS = {}
    cc, t = fit(X, Ks, H, link, "device")
    stages = engine.timer_summary(engine.TIMERS)
    engine.TIMERS = None
    say(f"device: total {t:.3f} s, timings_ {({k: round(v, 4) for k, v in cc.timings_.items()})}, plan {cc.hc_stats_}")
    say("device stages (launches, ms):", {k: (v[0], round(v[1], 2)) for k, v in stages.items()})
    engine.TIMERS = {}
    cc2, t2 = fit(X, Ks, H, link, "device")
    stages2 = engine.timer_summary(engine.TIMERS)
    engine.TIMERS = None
    say(f"device again: total {t2:.3f} s, cluster {cc2.timings_['cluster']:.3f} s")
    say("device again stages (launches, ms):", {k: (v[0], round(v[1], 2)) for k, v in stages2.items()})
    ch, th = fit(X, Ks, H, link, "host", n_jobs=16)
    say(f"host n_jobs=16: total {th:.3f} s, timings_ {({k: round(v, 4) for k, v in ch.timings_.items()})}")
    same = all(np.array_equal(cc.pair_counts_[K], ch.pair_counts_[K]) for K in Ks)
    say(f"pair counts identical: {same}; speed-up of the cluster stage {ch.timings_['cluster'] / cc2.timings_['cluster']:.1f}x")


def crossover(m):
    say(f"== crossover at m={m} (average linkage)")
    rs = np.random.RandomState(0)
    X = torch.from_numpy(rs.randn(m, 16).astype(np.float32)).cuda()
    D = engine.euclidean(X)
    idx1 = torch.arange(m, dtype=torch.int32, device="cuda")

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    engine.linkage_raw(D.clone(), "average")
    for rep in range(2):
        Dc = D.clone()
        say(f"cc_linkage_nnchain (grid form), one tree: {timed(lambda: engine.linkage_raw(Dc, 'average')) * 1e3:.1f} ms")
    for B in (1, 4, 16, 64):
        Db = engine.hc_gather(D, idx1.repeat(B, 1).contiguous())
        say(f"cc_hc_nnchain_batched B={B}: {timed(lambda: engine.hc_nnchain_batched(Db, 'average')) * 1e3:.1f} ms")
        del Db


def linkage_forms(reps=5):
    """Every form of the one nn_chain loop and the one Prim loop: many small trees through
    cc_hc_nnchain_batched (a step is short there, so a workgroup barrier more or less shows), and
    one n = 20 000 tree of cityblock distances through cc_linkage_nnchain / cc_linkage_mst on the
    default grid and in one workgroup (CCMI_LINK_G=0).  Median (min .. max) of `reps` calls after a
    warm-up, wall time around a synchronise, and a digest of the output to compare two builds."""
    import hashlib

    from consensus_clustering_amd import _lib

    def digest(t):
        return hashlib.sha1(t.cpu().numpy().tobytes()).hexdigest()[:12]

    def timed(make, run):
        ts, out = [], None
        for rep in range(reps + 1):
            arg = make()
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = run(arg)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
            del arg
        ts = ts[1:]
        return f"{np.median(ts):.2f} ms ({min(ts):.2f} .. {max(ts):.2f}), output {digest(out)}"

    say(f"== linkage forms: median (min .. max) of {reps} calls, one warm-up")
    rs = np.random.RandomState(0)
    for B, m in ((4096, 33), (64, 1025)):
        X = torch.from_numpy(rs.randn(m, 16).astype(np.float32)).cuda()
        Db = engine.hc_gather(engine.euclidean(X), torch.arange(m, dtype=torch.int32, device="cuda").repeat(B, 1).contiguous())
        say(f"cc_hc_nnchain_batched B={B} m={m} average: "
            + timed(Db.clone, lambda d: engine.hc_nnchain_batched(d, "average")))
        del Db
    n = 20000
    D = engine.pdist(torch.from_numpy(rs.rand(n, 16).astype(np.float32)).cuda(), "cityblock")

    def mst(d):
        out = torch.empty((n - 1, 3), dtype=torch.float64, device="cuda")
        ws = torch.empty(int(_lib.load().cc_linkage_mst_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
        _lib.call("cc_linkage_mst", d.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), engine.stream_ptr())
        _lib.call("cc_linkage_check", ws.data_ptr(), ws.numel(), engine.stream_ptr())
        return out

    for G in (None, "0"):
        if G is None:
            os.environ.pop("CCMI_LINK_G", None)
        else:
            os.environ["CCMI_LINK_G"] = G
        how = "CCMI_LINK_G unset" if G is None else f"CCMI_LINK_G={G}"
        say(f"cc_linkage_nnchain n={n} average, {how}: " + timed(D.clone, lambda d: engine.linkage_raw(d, "average")))
        say(f"cc_linkage_mst n={n}, {how}: " + timed(lambda: D, mst))
    os.environ.pop("CCMI_LINK_G", None)


def main():
    if "--linkage" in sys.argv[2:]:  # the tree builders alone
        crossover(8000)
        linkage_forms()
        return
    X, _ = make_blobs(n_samples=3000, n_features=32, centers=6, cluster_std=1.0, center_box=(-10, 10),
                      shuffle=True, random_state=0)
    shape("parity blobs", X.astype(np.float32), list(range(2, 13)), 60, "average")
    crossover(8000)
    Xb, _ = make_blobs(n_samples=10000, n_features=16, centers=8, cluster_std=1.0, center_box=(-10, 10),
                       shuffle=True, random_state=1)
    shape("m = 8000", Xb.astype(np.float32), list(range(2, 7)), 16, "average")


if __name__ == "__main__":
    main()
