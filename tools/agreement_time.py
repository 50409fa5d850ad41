"""Timings of the pairwise agreement sums (HIP events, warmed up, median of RUNS), uniformly random
labels with 20 % absent:
(a) engine.agreement_sums at the C3 shape (n = 50 000, H = 1000) for K = 8 and K = 20, the fraction
    of the int8 MFMA peak (5.03 POPS, as bench.py takes it) credited with n (H (K + 1))^2 ops (two
    per multiply-add of the triangle of pairs), the executed ops with the KP padding beside it, and
    the call over the single tile [0, 1): the transposition plus one tile, an upper bound of the
    transposition;
(b) at the C2 shape (n = 10 000, H = 500, K = 6): the route in plain torch (a materialised float32
    one-hot [n, H (K + 1)], O.T @ O, the four reductions in int64) against engine.agreement_sums,
    equal sums asserted;
(c) the peak memory above the inputs of both routes at (b).

    python tools/agreement_time.py [output.txt [trace]]
                                       (profiles/agreement/agreement_measure.txt is one run's output)
With a second argument "trace" only the two calls of (a) run, three times each after one warm-up:
the run to put under a kernel trace, whose per-kernel times split the transposition from the
tile kernel."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from consensus_clustering_amd import engine  # noqa: E402

RUNS, WARM = 10, 3
I8_PEAK_OPS = 5.033e15
dev = engine.require_gpu()
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
TRACE = len(sys.argv) > 2 and sys.argv[2] == "trace"


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


def make(n, H, K, absent=0.2, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    Hpad = engine.pad_h(H)
    L = torch.full((n, Hpad), 0xFF, dtype=torch.uint8, device=dev)
    lab = torch.randint(0, K, (n, H), generator=g, device=dev, dtype=torch.uint8)
    keep = torch.rand((n, H), generator=g, device=dev) >= absent
    L[:, :H] = torch.where(keep, lab, torch.full_like(lab, 0xFF))
    return L


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return peak


say("device", torch.cuda.get_device_name(0), "runs", RUNS, "warm-up", WARM)

# (a): the C3 shape
n, H = 50000, 1000
for K in (8, 20):
    L = make(n, H, K)
    nt = engine.agreement_num_tiles(H, K)
    if TRACE:
        for _ in range(4):
            engine.agreement_sums(L, H, K, n)
        torch.cuda.synchronize()
        say(f"trace run: n={n} H={H} K={K} tiles={nt}: 4 calls")
        continue
    kp = 4
    while kp < K + 1:
        kp *= 2
    credited = float(n) * (H * (K + 1)) ** 2
    executed = 2.0 * nt * 256 * 256 * ((n + 127) // 128 * 128)
    say(f"shape n={n} H={H} K={K} KP={kp} tiles={nt} credited ops {credited:.4g} executed ops {executed:.4g}")
    ms = report(f"(a) agreement_sums K={K}, all tiles (transposition + tile kernel)",
                timed_ms(lambda: engine.agreement_sums(L, H, K, n)))
    say(f"    credited {credited / (ms * 1e-3) / 1e15:.3f} POPS = {credited / (ms * 1e-3) / I8_PEAK_OPS:.3f} of the "
        f"int8 peak; executed {executed / (ms * 1e-3) / 1e15:.3f} POPS = "
        f"{executed / (ms * 1e-3) / I8_PEAK_OPS:.3f} of the peak")
    report(f"    agreement_sums K={K}, tile range [0, 1) (transposition + one tile)",
           timed_ms(lambda: engine.agreement_sums(L, H, K, n, tile_begin=0, tile_end=1)))
    del L
torch.cuda.empty_cache()
if TRACE:
    sys.exit(0)

# (b), (c): the C2 shape, both routes
n, H, K = 10000, 500, 6
L = make(n, H, K, seed=1)
say(f"shape n={n} H={H} K={K} tiles={engine.agreement_num_tiles(H, K)}")


def torch_route():
    """The ten lines of torch: materialised one-hot, one matmul, four reductions."""
    lab = L[:, :H]
    ar = torch.arange(K, device=dev, dtype=torch.uint8)
    O = torch.cat([lab.unsqueeze(-1) == ar, (lab != 0xFF).unsqueeze(-1)], dim=-1).float().reshape(n, H * (K + 1))
    G = (O.T @ O).long().view(H, K + 1, H, K + 1)  # counts <= 10 000: exact in float32
    s0 = G[:, K, :, K]
    s2 = (G[:, :K, :, :K] ** 2).sum(dim=(1, 3))
    r2 = (G[:, :K, :, K] ** 2).sum(dim=1)
    c2 = (G[:, K, :, :K] ** 2).sum(dim=-1)
    return torch.stack([s0, s2, r2, c2], dim=-1)


S_torch = torch_route()
S_new = engine.agreement_sums(L, H, K, n)
assert bool((S_torch == S_new).all()), "the two routes disagree"
say("both routes give the same sums at the C2 shape")
del S_torch, S_new
t_ms = report("(b) torch route (float32 one-hot, O.T @ O, four reductions)", timed_ms(torch_route))
a_ms = report("(b) agreement_sums (transposition + tile kernel)", timed_ms(lambda: engine.agreement_sums(L, H, K, n)))
say(f"ratio: agreement_sums / torch route = {a_ms / t_ms:.3f}")
say(f"(c) torch route peak memory above the inputs: {peak_above(torch_route) / 2**20:.1f} MiB")
say(f"(c) agreement_sums peak memory above the inputs: "
    f"{peak_above(lambda: engine.agreement_sums(L, H, K, n)) / 2**20:.1f} MiB")
