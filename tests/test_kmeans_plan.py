"""cc_kmeans_launch_plan, the one planner behind BatchedKMeans and cc_kmeans_fit: what is launched
for a fit (engine, K values per call, grid or batch, units per resample, concurrent seeders,
workspace).  Host arithmetic only, so none of this needs a GPU.

tests/golden/engine/launch_plans.json holds the launches the Python host planned for itself
before the planner existed (tests/golden/make_launch_plans.py, run at the commit it names); the
planner must return exactly those."""
import ctypes
import json
import os

import numpy as np
import pytest

from consensus_clustering_amd import _lib, kmeans

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine", "launch_plans.json")
with open(GOLDEN) as f:
    ROWS = json.load(f)["rows"]
GiB = 1 << 30
BIGK = [21, 24, 25, 32, 33, 54, 55, 64, 65, 96, 97, 125, 127]


def plan_row(row, **over):
    a = {**row, **over}
    return kmeans.launch_plan(a["d"], a["m"], a["nh"], a["Ks"], a["n_init"], a["precision"], a["cus"],
                              a["budget"], a["budget_hard"], a["n_sub"], a["seedmax"], a["grid"])


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_planner_reproduces_the_parent_plan(row):
    got = plan_row(row)
    want = [{**c, "engine": "cc_kmeans_" + c["engine"]} for c in row["calls"]]
    assert got == want
    if got[0]["engine"] == "cc_kmeans_batched":  # the unit table whoever launches builds from n_sub
        assert kmeans.plan(row["Ks"], row["n_init"], got[0]["n_sub"]).shape[0] == row["nU"]


def test_fixture_covers_the_rules():
    """The rows the planner is pinned on, and the values worked out by hand for three of them."""
    by = {r["name"]: r for r in ROWS}
    c = by["c3_nh1000_40g"]["calls"][0]
    assert (c["n_sub"], by["c3_nh1000_40g"]["nU"], c["seedmax"], c["par"], c["ws_bytes"]) == (1, 1, 24, 256, 8718516480)
    c = by["c3_nh125_40g"]["calls"][0]
    assert (c["n_sub"], by["c3_nh125_40g"]["nU"], c["seedmax"], c["par"], c["ws_bytes"]) == (2, 2, 24, 250, 6768000256)
    c = by["c5_nh256_8g"]["calls"][0]
    assert (c["n_sub"], by["c5_nh256_8g"]["nU"], c["seedmax"], c["par"]) == (1, 1, 24, 64)
    assert by["k2_39_nsub1"]["nU"] == 2
    assert by["c2_seedmax2"]["calls"][0]["seedmax"] == 2
    assert by["bigk_nsub13"]["calls"][0]["n_sub"] == 13 and by["bigk_nsub1"]["calls"][0]["n_sub"] == 1
    assert len(by["wide_bigk"]["calls"]) >= 2 and len(by["wide_k2_30"]["calls"]) == 2
    assert by["c4_96g"]["calls"][0]["par"] == 1000 and by["c4_1b"]["calls"][0]["par"] == 1
    # float64 at the C3 shape, 256 CUs: the full grid, the two-per-CU floor above an 8 GiB budget,
    # the largest grid within a caller's 8 GiB, and one workgroup when nothing fits
    assert [by[k]["calls"][0]["par"] for k in ("f64_c3_40g_120g", "f64_c3_8g_120g", "f64_c3_8g_8g", "f64_c3_1b")] == \
        [1024, 512, 87, 1]
    assert by["f64_c3_8g_120g"]["calls"][0]["ws_bytes"] > 8 * GiB > by["f64_c3_8g_8g"]["calls"][0]["ws_bytes"]
    assert [(c["k0"], c["nk"]) for c in by["f64_70k"]["calls"]] == [(0, 64), (64, 6)]
    assert any(r["cus"] == 8 for r in ROWS)


SHAPES = [  # d, m, nh, Ks, precision
    (128, 40000, 125, list(range(2, 21)), 0),
    (16, 1228, 3, BIGK, 0),
    (16, 1228, 4, list(range(2, 40)), 0),
    (320, 819, 7, BIGK, 0),
    (20000, 4000, 1000, list(range(2, 13)), 0),
    (128, 40000, 128, list(range(2, 21)), 1),
    (12, 320, 6, list(range(2, 72)), 1),
]


@pytest.mark.parametrize("d,m,nh,Ks,precision", SHAPES)
def test_budget_extremes(d, m, nh, Ks, precision):
    """With one byte every call of every engine runs one workgroup (or one resample at a time); with
    no limit it runs the starting size: min(cus, units), min(4 cus, nh * nk), all nh resamples.
    The K values per call and the batched call's units and seeders do not depend on the budget."""
    cus = 256
    least = kmeans.launch_plan(d, m, nh, Ks, 3, precision, cus, 1, 1)
    most = kmeans.launch_plan(d, m, nh, Ks, 3, precision, cus, kmeans.UNLIMITED, kmeans.UNLIMITED)
    assert [c["par"] for c in least] == [1] * len(least)
    fixed = ("engine", "k0", "nk", "n_sub", "seedmax")
    assert [[c[k] for k in fixed] for c in least] == [[c[k] for k in fixed] for c in most]
    assert [K for c in most for K in Ks[c["k0"]:c["k0"] + c["nk"]]] == Ks
    for lo, hi in zip(least, most):
        if hi["engine"] == "cc_kmeans_batched":
            g0 = min(cus, nh * kmeans.plan(Ks, 3, hi["n_sub"]).shape[0])
        elif hi["engine"] == "cc_kmeans_f64":
            g0 = min(4 * cus, nh * hi["nk"])
        else:
            g0 = nh
        assert hi["par"] == g0
        assert lo["ws_bytes"] <= hi["ws_bytes"] and lo["ws_bytes"] % 256 == 0
    # an f64 starting grid the caller names replaces min(4 cus, nh * nk)
    if precision == 1:
        named = kmeans.launch_plan(d, m, nh, Ks, 3, precision, cus, kmeans.UNLIMITED, kmeans.UNLIMITED, grid=3)
        assert [c["par"] for c in named] == [3] * len(named)


def test_planner_errors():
    lib = _lib.load()
    Ks = np.asarray(list(range(2, 31)), dtype=np.int32)
    buf = (kmeans._Call * 4)()

    def plan(d, nK, precision, max_calls, n_init=3, nh=4):
        return lib.cc_kmeans_launch_plan(d, 819, nh, Ks.ctypes.data, nK, n_init, precision, 256, 1 << 40, 1 << 40,
                                         0, 0, 0, ctypes.addressof(buf), max_calls)

    assert plan(320, len(Ks), 0, 4) == 2  # two wide calls
    for d, precision in ((16, 0), (320, 0), (16, 1)):  # an output array too small for the calls
        assert plan(d, len(Ks), precision, 1 if d == 320 else 0) < 0
        assert "max_calls" in lib.cc_last_error().decode()
    assert plan(16, len(Ks), 0, 4, nh=0) < 0 and "bad arguments" in lib.cc_last_error().decode()
    assert plan(16, len(Ks), 2, 4) < 0 and "bad arguments" in lib.cc_last_error().decode()
    # a K that fits no wide call alone: cc_kmeans_wide_chunk's error, unchanged
    big = np.asarray([127, 2], dtype=np.int32)
    assert lib.cc_kmeans_launch_plan(320, 819, 4, big.ctypes.data, 2, 16, 0, 256, 1 << 40, 1 << 40, 0, 0, 0,
                                     ctypes.addressof(buf), 4) < 0
    msg = lib.cc_last_error().decode()
    assert "K = 127" in msg and "n_init = 16" in msg
    with pytest.raises(_lib.CCMIError, match="K = 127 with n_init = 16"):
        kmeans.launch_plan(320, 819, 4, [127, 2], 16, 0, 256, 1, 1)
    with pytest.raises(_lib.CCMIError):
        kmeans.launch_plan(16, 819, 4, [128], 3, 0, 256, 1, 1)  # cc_kmeans_plan's K <= 127


def test_dpad():
    lib = _lib.load()
    assert [lib.cc_kmeans_dpad(d) for d in (1, 32, 33, 64, 65, 128, 129, 160, 161, 20000)] == \
        [32, 32, 64, 64, 128, 128, 160, 160, 192, 20000]
    assert lib.cc_kmeans_dpad(0) < 0
