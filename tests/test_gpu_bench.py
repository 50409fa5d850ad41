"""bench.py's output contract, on the GPU: the one JSON line the driver reads (its keys, the
roofline and cpu_baseline objects), and that the timed region times the fits and nothing else
(every step's wall time equals the fit's own total); a plain run and its --dump-outputs files."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_json_contract_c2():
    steps = 2
    proc = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--config", "c2",
                           "--steps", str(steps), "--warmup", "1", "--full", "--no-consensus-roofline"],
                          cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]  # exactly one JSON line
    d = json.loads(lines[0])

    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] in ("weak", "strong")
    assert d["unit"] == "resample-clusterings/s" and "workload" in d["config"]

    # value = every clustering of the timed fits over the timed wall time
    H, (K0, K1) = d["config"]["H"], d["config"]["K_range"]
    clusterings = H * (K1 - K0 + 1)
    assert d["value"] == pytest.approx(clusterings / (d["ms_per_step"] * 1e-3), rel=1e-9)

    # the timed region is the fits: each step's wall time is its fit's own total
    assert len(d["step_ms"]) == steps == len(d["fit_total_ms"])
    for wall, fit in zip(d["step_ms"], d["fit_total_ms"]):
        assert abs(wall - fit) < 5.0, (d["step_ms"], d["fit_total_ms"])
    assert sum(d["step_ms"]) <= steps * d["ms_per_step"] + 0.05 * steps + 1e-6  # step_ms: rounded to 0.1 ms

    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert 0.0 < r["frac"] <= 1.0
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-9)
    # achieved = the kernel's credited flops per launch over its HIP-event launch time
    assert r["achieved"] == pytest.approx(r["flops_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e12, rel=1e-9)
    assert r["executed_flops_per_launch"] >= r["flops_per_launch"]  # padding slots only add work
    co = d["roofline_coassoc"]
    assert 0.0 < co["frac"] <= 1.0

    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["value"] > 0 and cb["kind"] in ("reference", "port") and cb["cores"] >= 1


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain run times its steps and nothing else (no cpu_baseline, no roofline_consensus: those
    are --full's), and --dump-outputs writes the last step's results as float .npy files."""
    import numpy as np

    steps, out = 3, tmp_path / "dump"
    proc = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--config", "smoke", "--gpus", "1",
                           "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out)],
                          cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in d, k
    assert "cpu_baseline" not in d and "roofline_consensus" not in d
    assert d["steps"] == steps == len(d["step_ms"])
    # the steps lie inside the timed region; step_ms is rounded to 0.1 ms per step, ms_per_step is not
    assert sum(d["step_ms"]) <= steps * d["ms_per_step"] + 0.05 * steps + 1e-6

    files ={p.stem: np.load(p) for p in out.glob("*.npy")}
    assert {"K_range", "hist", "cdf", "bin_edges", "pac_area", "cdf_area", "delta_k", "best_k", "pair_counts",
            "kmeans_inertia", "kmeans_n_iter", "label_rows", "labels"} <= set(files)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    H, (K0, K1), n = d["config"]["H"], d["config"]["K_range"], d["config"]["n"]
    nK = K1 - K0 + 1
    np.testing.assert_array_equal(files["K_range"], np.arange(K0, K1 + 1))
    assert files["cdf"].shape == (nK, 20) and files["kmeans_inertia"].shape == (nK, H)
    # every pair counted: the CDF ends at 1 (float32 bin widths: a few 1e-8 off)
    np.testing.assert_allclose(files["cdf"][:, -1], 1.0, rtol=0, atol=1e-6)
    assert files["pair_counts"].sum(axis=1).tolist() == [n * (n - 1) // 2] * nK
    rows, lab = files["label_rows"], files["labels"]
    assert lab.shape == (nK, len(rows), H) and np.all(np.diff(rows) > 0) and rows[-1] < n
    for k in range(nK):  # a label is a cluster of its K, or 255 where the row was not sampled
        assert np.all((lab[k] < K0 + k) | (lab[k] == 255))
    assert np.mean(lab[0] != 255) == pytest.approx(0.8, abs=0.02)  # subsampling 0.8
    assert files["best_k"][0] in files["K_range"]
