"""Pin how a k-means fit becomes engine launches: tests/golden/engine/launch_plans.json.

Run this at commit 1323ef2 ("k-means: scheduler on a wave; compare and tol loads kept in
flight"), the last one whose Python host (consensus_clustering_amd/kmeans.py) planned its own
launches.  It cannot run later: kmeans.choose_subsets, default_seedmax and dpad_for, which it
imports, moved into the library's planner (cc_kmeans_launch_plan) and left kmeans.py.

    python tests/golden/make_launch_plans.py [OUT.json]

No GPU is needed.  For every row of ROWS it evaluates the rules of that commit's
BatchedKMeans.run, _run_wide and run_f64 (their budget loops are repeated here line for line,
with the CU count and the free device memory as inputs instead of queries) against the library's
own workspace and chunk functions, and stores the engine calls that result.  Each row also keeps
the two byte counts (budget, budget_hard) a planner needs to reproduce it:

    run       budget = workspace_budget or DEFAULT,      budget_hard = int(0.5 * free)
    _run_wide budget = wide_budget,                      budget_hard = int(0.6 * free)
    run_f64   workspace_budget None: budget = DEFAULT,   budget_hard = int(0.5 * free)
              else: budget = budget_hard = min(workspace_budget, int(0.5 * free))

tests/test_kmeans_plan.py asserts that the planner returns exactly the stored calls.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from consensus_clustering_amd import _lib, kmeans  # noqa: E402

COMMIT = "1323ef2"
GiB = 1 << 30
FREE = 240 * GiB
BIGK = [21, 24, 25, 32, 33, 54, 55, 64, 65, 96, 97, 125, 127]


def r(lo, hi):
    return list(range(lo, hi + 1))


def batched(name, d, m, nh, Ks, workspace_budget, cus=256, n_init=3, n_sub=0, seedmax=0, free=FREE):
    return dict(name=name, kind="batched", d=d, m=m, nh=nh, Ks=Ks, n_init=n_init, cus=cus,
                workspace_budget=workspace_budget, free=free, n_sub=n_sub, seedmax=seedmax, grid=0)


def wide(name, d, m, nh, Ks, wide_budget, cus=256, n_init=3, free=FREE):
    return dict(name=name, kind="wide", d=d, m=m, nh=nh, Ks=Ks, n_init=n_init, cus=cus,
                wide_budget=wide_budget, free=free, n_sub=0, seedmax=0, grid=0)


def f64(name, d, m, nh, Ks, workspace_budget, default=kmeans.DEFAULT_WORKSPACE_BUDGET, cus=256, n_init=3,
        grid=0, free=FREE):
    return dict(name=name, kind="f64", d=d, m=m, nh=nh, Ks=Ks, n_init=n_init, cus=cus,
                workspace_budget=workspace_budget, default=default, free=free, n_sub=0, seedmax=0, grid=grid)


ROWS = []
for tag, b in (("40g", 40 * GiB), ("8g", 8 * GiB), ("1b", 1)):
    ROWS += [batched(f"c3_nh1000_{tag}", 128, 40000, 1000, r(2, 20), b),
             batched(f"c3_nh125_{tag}", 128, 40000, 125, r(2, 20), b),
             batched(f"c2_nh500_{tag}", 64, 8000, 500, r(2, 15), b),
             batched(f"c5_nh256_{tag}", 32, 160000, 256, r(2, 10), b)]
ROWS += [
    batched("c3_default_budget", 128, 40000, 1000, r(2, 20), None),
    batched("c3_little_free", 128, 40000, 1000, r(2, 20), None, free=12 * GiB),
    batched("bigk_nsub1", 16, 1228, 3, BIGK, None, n_sub=1),
    batched("bigk_nsub13", 16, 1228, 3, BIGK, None, n_sub=13),
    batched("bigk_nsub13_nh64", 16, 1228, 64, BIGK, None, n_sub=13),
    batched("bigk_auto", 16, 1228, 3, BIGK, None),
    batched("c2_seedmax2", 64, 8000, 500, r(2, 15), None, seedmax=2),
    batched("c2_seedmax40", 64, 8000, 500, r(2, 15), None, seedmax=40),
    batched("k2_39_nsub1", 16, 1228, 4, r(2, 39), None, n_sub=1),
    batched("one_k_one_init", 5, 80, 2, [3], None, n_init=1),
    batched("c2_cus8", 64, 8000, 500, r(2, 15), 8 * GiB, cus=8),
    batched("c3_cus8_nh3", 100, 40000, 3, r(2, 20), None, cus=8),
    wide("c4_96g", 20000, 4000, 1000, r(2, 12), 96 * GiB),
    wide("c4_1b", 20000, 4000, 1000, r(2, 12), 1),
    wide("c4_8g", 20000, 4000, 1000, r(2, 12), 8 * GiB),
    wide("c4_little_free", 20000, 4000, 1000, r(2, 12), 96 * GiB, free=10 * GiB),
    wide("wide_bigk", 320, 819, 2, BIGK, 96 * GiB),
    wide("wide_bigk_1b", 320, 819, 2, BIGK, 1),
    wide("wide_k2_30", 320, 819, 2, r(2, 30), 96 * GiB),
    wide("wide_d300_nh7", 300, 480, 7, [2, 4, 7], 1 << 22),
    wide("wide_cus8", 320, 819, 5, r(2, 30), 96 * GiB, cus=8),
    f64("f64_c3_40g_120g", 128, 40000, 128, r(2, 20), None),
    f64("f64_c3_8g_120g", 128, 40000, 128, r(2, 20), None, default=8 * GiB),   # the two-per-CU floor
    f64("f64_c3_8g_8g", 128, 40000, 128, r(2, 20), 8 * GiB),                  # grid 87
    f64("f64_c3_1b", 128, 40000, 128, r(2, 20), 1),
    f64("f64_c3_little_free", 128, 40000, 128, r(2, 20), None, free=6 * GiB),
    f64("f64_70k", 12, 320, 6, r(2, 71), None),
    f64("f64_70k_1b", 12, 320, 6, r(2, 71), 1),
    f64("f64_grid1", 12, 320, 6, [2, 3, 6], None, grid=1),
    f64("f64_grid2", 12, 320, 6, [2, 3, 6], None, grid=2),
    f64("f64_grid2_1b", 12, 320, 6, [2, 3, 6], 1, grid=2),
    f64("f64_cus8", 128, 40000, 128, r(2, 20), None, cus=8),
    f64("f64_wide_rows", 300, 240, 5, [2, 5], None),
]


def call(engine, k0, nk, par, ws_bytes, n_sub=0, seedmax=0):
    return dict(engine=engine, k0=int(k0), nk=int(nk), par=int(par), n_sub=int(n_sub), seedmax=int(seedmax),
                ws_bytes=int(ws_bytes))


def run_batched(row, lib):
    """BatchedKMeans.run at COMMIT (d <= 128)."""
    Ks, n_init, nh, m, cus = row["Ks"], row["n_init"], row["nh"], row["m"], row["cus"]
    dpad = kmeans.dpad_for(row["d"])
    n_sub = row["n_sub"] or kmeans.choose_subsets(nh, len(Ks), cus)
    u_h = kmeans.plan(Ks, n_init, n_sub)
    nU = u_h.shape[0]
    seedmax = max(1, min(row["seedmax"] or kmeans.default_seedmax(m), 32, int(u_h[:, 0].max())))
    per = lambda g: lib.cc_kmeans_workspace_bytes(m, dpad, u_h.ctypes.data, nU, seedmax, g)
    grid = min(cus, nh * nU)
    budget = min(row["workspace_budget"] or kmeans.DEFAULT_WORKSPACE_BUDGET, int(0.5 * row["free"]))
    while grid > 1 and per(grid) > budget:
        grid //= 2
    row["budget"] = row["workspace_budget"] or kmeans.DEFAULT_WORKSPACE_BUDGET
    row["budget_hard"] = int(0.5 * row["free"])
    row["nU"] = int(nU)
    return [call("batched", 0, len(Ks), grid, per(grid), n_sub, seedmax)]


def run_f64(row, lib):
    """BatchedKMeans.run_f64 at COMMIT."""
    all_Ks, nh, m, d, cus, grid = row["Ks"], row["nh"], row["m"], row["d"], row["cus"], row["grid"]
    DEFAULT_WORKSPACE_BUDGET = row["default"]
    calls = []
    for k0 in range(0, len(all_Ks), 64):
        Ks = all_Ks[k0:k0 + 64]
        Ks_np = np.ascontiguousarray(np.asarray(Ks, dtype=np.int32))
        g = int(grid or min(4 * cus, nh * len(Ks)))
        per = lambda gg: lib.cc_kmeans_f64_workspace_bytes(m, d, Ks_np.ctypes.data, len(Ks), gg, nh)
        free_half = int(0.5 * row["free"])
        if row["workspace_budget"] is None:
            cap = min(max(DEFAULT_WORKSPACE_BUDGET, per(min(g, 2 * cus))), free_half)
        else:
            cap = min(row["workspace_budget"], free_half)
        if per(g) > cap:  # the largest grid that fits (per(g) is non-decreasing in g)
            lo, hi = 1, g
            while lo < hi:
                mid = (lo + hi + 1) // 2
                if per(mid) <= cap:
                    lo = mid
                else:
                    hi = mid - 1
            g = lo
        calls.append(call("f64", k0, len(Ks), g, per(g)))
    if row["workspace_budget"] is None:
        row["budget"], row["budget_hard"] = DEFAULT_WORKSPACE_BUDGET, free_half
    else:
        row["budget"] = row["budget_hard"] = min(row["workspace_budget"], free_half)
    return calls


def run_wide(row, lib):
    """BatchedKMeans._run_wide at COMMIT (d > 128)."""
    all_K, n_init, nh, m = row["Ks"], row["n_init"], row["nh"], row["m"]
    dpad = kmeans.dpad_for(row["d"])
    budget = min(row["wide_budget"], int(0.6 * row["free"]))
    all_Ks = np.ascontiguousarray(np.asarray(all_K, dtype=np.int32))
    calls = []
    k0 = per_call = 0
    while k0 + per_call < len(all_K):
        k0 += per_call
        per_call = lib.cc_kmeans_wide_chunk(m, dpad, all_Ks[k0:].ctypes.data, len(all_K) - k0, n_init)
        if per_call <= 0:
            _lib.check(per_call or -1, "cc_kmeans_wide_chunk")
        Ks = all_K[k0:k0 + per_call]
        Ks_np = np.ascontiguousarray(all_Ks[k0:k0 + per_call])
        ws1 = lib.cc_kmeans_wide_workspace_bytes(m, dpad, Ks_np.ctypes.data, len(Ks), n_init, 1)
        ws2 = lib.cc_kmeans_wide_workspace_bytes(m, dpad, Ks_np.ctypes.data, len(Ks), n_init, 2)
        if ws1 == 0:
            _lib.check(-1, "cc_kmeans_wide_workspace_bytes")
        per = ws2 - ws1
        cap = int(max(1, min(nh, (budget - (ws1 - per)) // per)))
        batch = -(-nh // -(-nh // cap))  # equal batches: one round-count tail per batch
        calls.append(call("wide", k0, per_call, batch, ws1 + per * (batch - 1)))
    row["budget"], row["budget_hard"] = row["wide_budget"], int(0.6 * row["free"])
    return calls


def main(out=os.path.join(HERE, "engine", "launch_plans.json")):
    lib = _lib.load()
    rows = []
    for spec in ROWS:
        row = dict(spec)
        calls = dict(batched=run_batched, wide=run_wide, f64=run_f64)[row["kind"]](row, lib)
        keep = ("name", "d", "m", "nh", "Ks", "n_init", "cus", "budget", "budget_hard", "n_sub", "seedmax", "grid")
        rows.append({**{k: row[k] for k in keep}, "precision": int(row["kind"] == "f64"),
                     "nU": row.get("nU", 0), "calls": calls})
        print(row["name"], [(c["engine"], c["k0"], c["nk"], c["par"], c["n_sub"], c["seedmax"], c["ws_bytes"])
                            for c in calls], flush=True)
    assert len({row["name"] for row in rows}) == len(rows)
    with open(out, "w") as f:
        f.write('{"commit": "%s",\n "rows": [\n' % COMMIT)
        f.write(",\n".join("  " + json.dumps(row) for row in rows))
        f.write("\n]}\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:2])
