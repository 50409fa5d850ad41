"""Timings of the item-consensus route (HIP events, warmed up, median of RUNS):
(a) engine.item_consensus_sums at n = 50 000, H = 1000, K = 8, Kc = 8, random labels;
(b) the cc_coassoc launch for K = 8 at that shape (all tiles, co-sampling tiles precomputed);
(c) at n = 20 000: the materialised route (cosample full, coassoc full, consensus, * 2^40,
    index_add by cluster) against item_consensus_sums.

    python tools/icl_time.py [output.txt [K [kernel]]]
                                               (profiles/icl/icl_timing.txt is one run's output)
K (default 8) is the number of label values of (a), (b) and (c); with a third argument "kernel"
only line (a'), the cc_item_consensus launch alone, is timed (an A/B of two libraries)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from consensus_clustering_amd import engine  # noqa: E402

RUNS, WARM = 10, 3
dev = engine.require_gpu()
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def timed_ms(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def report(name, ts):
    say(f"{name}: median {statistics.median(ts):.3f} ms  mean {statistics.mean(ts):.3f}  min {min(ts):.3f}  "
        f"max {max(ts):.3f}  runs {len(ts)}  raw {[round(t, 3) for t in ts]}")
    return statistics.median(ts)


def make(n, H, K, Kc, frac=0.8, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    Hpad = engine.pad_h(H)
    L = torch.full((n, Hpad), 0xFF, dtype=torch.uint8, device=dev)
    lab = torch.randint(0, K, (n, H), generator=g, device=dev, dtype=torch.uint8)
    keep = torch.rand((n, H), generator=g, device=dev) < frac
    L[:, :H] = torch.where(keep, lab, torch.full_like(lab, 0xFF))
    cl = torch.randint(0, Kc, (n,), generator=g, device=dev, dtype=torch.int32)
    return L, Hpad, cl


say("device", torch.cuda.get_device_name(0), "runs", RUNS, "warm-up", WARM)

# (a), (b): the C3 shape
n, H, K, Kc = 50000, 1000, int(sys.argv[2]) if len(sys.argv) > 2 else 8, 8
KERNEL_ONLY = len(sys.argv) > 3 and sys.argv[3] == "kernel"
L, Hpad, cl = make(n, H, K, Kc)
nt = engine.num_tiles(n)
say(f"shape n={n} H={H} Hpad={Hpad} K={K} Kc={Kc} tiles={nt}")
if not KERNEL_ONLY:
    a_ms = report("(a) item_consensus_sums, tile_chunk 2048 (cosample + item kernel per chunk)",
                  timed_ms(lambda: engine.item_consensus_sums(L, n, Hpad, K, cl, Kc)))
    engine.TIMERS = {}
    engine.item_consensus_sums(L, n, Hpad, K, cl, Kc)
    torch.cuda.synchronize()
    for k, (cnt, ms) in engine.timer_summary(engine.TIMERS).items():
        say(f"    one call, per kernel: {k}: {cnt} launches, {ms:.3f} ms")
    engine.TIMERS = None

I_tiles, _ = engine.cosample(L, n, Hpad, 0, nt)
S = torch.zeros((n, Kc), dtype=torch.int64, device=dev)
S_chunked = engine.item_consensus_sums(L, n, Hpad, K, cl, Kc)
a1_ms = report("(a') cc_item_consensus alone, one launch over all tiles (co-sampling tiles precomputed)",
               timed_ms(lambda: engine._lib.call("cc_item_consensus", L.data_ptr(), n, L.stride(0), Hpad, K, 0, nt,
                                                 I_tiles.data_ptr(), cl.data_ptr(), Kc, S.data_ptr(),
                                                 engine.stream_ptr())))
assert bool((S == (WARM + RUNS) * S_chunked).all()), "one launch and the chunked walk disagree"
if KERNEL_ONLY:
    sys.exit(0)
edges = engine.edges_device(dev)
counts = torch.zeros(20, dtype=torch.int64, device=dev)
b_ms = report(f"(b) cc_coassoc K={K}, one launch over all tiles (FP4 contraction + histogram)",
              timed_ms(lambda: engine.coassoc(L, n, Hpad, K, 0, nt, I_tiles, edges, counts)))
c_ms = report("    cc_cosample, one launch over all tiles", timed_ms(lambda: engine.cosample(L, n, Hpad, 0, nt)))
say(f"ratios: (a)/(b) = {a_ms / b_ms:.2f}  (a')/(b) = {a1_ms / b_ms:.2f}")
del I_tiles, S, S_chunked, L, cl
torch.cuda.empty_cache()

# (c): n = 20 000, both routes
n = 20000
L, Hpad, cl = make(n, H, K, Kc, seed=1)
nt = engine.num_tiles(n)
say(f"shape n={n} H={H} K={K} Kc={Kc} tiles={nt}")


def materialised():
    I_t, I_full = engine.cosample(L, n, Hpad, 0, nt, want_full=True)
    M = torch.zeros((n, n), dtype=torch.int32, device=dev)
    cnt = torch.zeros(20, dtype=torch.int64, device=dev)
    engine.coassoc(L, n, Hpad, K, 0, nt, I_t, edges, cnt, M)
    C = engine.consensus(M, I_full)
    del M, I_full, I_t
    Q = (C.double() * float(1 << 40)).long()
    del C
    Q.fill_diagonal_(0)
    return torch.zeros((n, Kc), dtype=torch.int64, device=dev).index_add_(1, cl.long(), Q)


S_mat = materialised()
S_new = engine.item_consensus_sums(L, n, Hpad, K, cl, Kc)
assert bool((S_mat == S_new).all()), "the two routes disagree"
say("both routes give the same S at n = 20 000")
del S_mat, S_new
m_ms = report("(c) materialised route", timed_ms(materialised))
torch.cuda.reset_peak_memory_stats()
base = torch.cuda.memory_allocated()
materialised()
torch.cuda.synchronize()
say(f"    materialised route peak memory above the inputs: {(torch.cuda.max_memory_allocated() - base) / 2**30:.2f} GiB")
i_ms = report("(c) item_consensus_sums", timed_ms(lambda: engine.item_consensus_sums(L, n, Hpad, K, cl, Kc)))
torch.cuda.reset_peak_memory_stats()
base = torch.cuda.memory_allocated()
engine.item_consensus_sums(L, n, Hpad, K, cl, Kc)
torch.cuda.synchronize()
say(f"    item_consensus_sums peak memory above the inputs: {(torch.cuda.max_memory_allocated() - base) / 2**30:.2f} GiB")
say(f"ratio: item_consensus_sums / materialised = {i_ms / m_ms:.2f}")
