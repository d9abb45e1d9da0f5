"""CPU tier: bench.py --dump-outputs DIR writes what the timed path computed in its LAST TIMED step as float .npy files (at
most 64 MB: a seeded sample of the carriers beyond that), and --steps sets the number of timed steps.  The device is the
stand-in of tests/bench_fake_device.py, whose soft outputs carry the number of the step that made them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def _run_bench(tmp_path, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(TDM_BENCH_TEST_HOOK=os.path.join(HERE, "bench_fake_device.py"), TDM_BENCH_NO_PINNED="1", TDM_BENCH_LIVE_PMC="0",
               PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--carriers", "5", "--chunk", "4096",
           "--no-cpu-baseline", "--no-extra"] + list(extra)
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=200, cwd=str(tmp_path))


@pytest.mark.timeout(240)
def test_dump_outputs_holds_the_last_timed_step(tmp_path):
    import bench
    steps, warmup = 7, 3
    out = tmp_path / "dump"
    r = _run_bench(tmp_path, "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0
    assert d["dump_outputs"]["rows"] == 5 and d["dump_outputs"]["of_rows"] == 5
    names = {"hard", "soft", "n_soft", "best_phase", "min_margin", "rows"}
    assert {f[:-4] for f in os.listdir(out)} == names
    a = {n: np.load(out / (n + ".npy")) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) == d["dump_outputs"]["bytes"] <= 64 << 20
    ms = 34   # the stand-in's max_soft; it reports 30 soft symbols per carrier, hard symbols 0
    assert a["hard"].shape == (5, ms) and a["soft"].shape == (5, ms, 2)
    assert np.array_equal(a["n_soft"], np.full(5, 30.0)) and np.array_equal(a["rows"], np.arange(5.0))
    assert np.all(a["hard"][:, :29] == 0) and np.all(a["hard"][:, 29:] == -1)
    # every pass enqueued so far -- settling, warm-up, timed -- and none of the per-kernel pass that follows the timed one
    last_timed = max(bench.SETTLE_STEPS, warmup) + steps
    assert np.all(a["soft"][:, :30, 0] == last_timed) and np.all(a["soft"][:, :30, 1] == 0)
    assert np.all(a["soft"][:, 30:] == 0)


@pytest.mark.timeout(240)
def test_dump_outputs_is_the_same_from_run_to_run(tmp_path):
    for k in ("a", "b"):
        r = _run_bench(tmp_path, "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / k))
        assert r.returncode == 0, r.stderr[-2000:]
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


def test_dump_outputs_samples_rows_beyond_the_limit(tmp_path):
    import bench
    rows, ms = 50, 40
    rng = np.random.default_rng(3)
    hard = rng.integers(0, 4, (rows, ms)).astype(np.uint8)
    soft = (rng.standard_normal((rows, ms)) + 1j * rng.standard_normal((rows, ms))).astype(np.complex128)
    n_soft = rng.integers(0, ms + 1, rows).astype(np.int32)
    bp, mm = rng.integers(0, 10, rows).astype(np.int32), rng.random(rows)
    limit = 12 * (ms * 4 + ms * 16 + 32)
    for k in ("a", "b"):
        info = bench.dump_outputs(str(tmp_path / k), hard, soft, n_soft, bp, mm, limit=limit)
        assert info["rows"] == 12 and info["of_rows"] == rows and info["bytes"] <= limit
    sel = np.load(tmp_path / "a" / "rows.npy").astype(np.int64)
    assert np.array_equal(sel, np.load(tmp_path / "b" / "rows.npy")) and np.all(np.diff(sel) > 0)
    h, s = np.load(tmp_path / "a" / "hard.npy"), np.load(tmp_path / "a" / "soft.npy")
    for i, r in enumerate(sel):
        n = int(n_soft[r])
        assert np.array_equal(h[i, :max(n - 1, 0)], hard[r, :max(n - 1, 0)]) and np.all(h[i, max(n - 1, 0):] == -1)
        assert np.array_equal(s[i, :n, 0], soft[r, :n].real) and np.array_equal(s[i, :n, 1], soft[r, :n].imag)
        assert np.all(s[i, n:] == 0)
    assert np.array_equal(np.load(tmp_path / "a" / "best_phase.npy"), bp[sel]) and np.array_equal(np.load(tmp_path / "a" / "min_margin.npy"), mm[sel])


@pytest.mark.timeout(240)
def test_plain_run_measures_the_headline_only_and_full_adds_the_rest(tmp_path):
    """a plain run prints the headline fields and leaves the per-kernel pass, the roofline and the output check to --full"""
    headline = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
    side = {"output_check", "ms_per_step_per_kernel_pass_rank0", "stage_ms_per_launch", "roofline", "hbm_ceiling_measured"}
    r = _run_bench(tmp_path, "--steps", "3", "--warmup", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    plain = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert headline <= set(plain) and not side & set(plain) and plain["full"] is False
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["value"] > 0 and plain["dtype"] == "f64"
    r = _run_bench(tmp_path, "--steps", "3", "--warmup", "1", "--full")
    assert r.returncode == 0, r.stderr[-2000:]
    full = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert headline | side <= set(full) and full["full"] is True
    assert full["stage_ms_per_launch"]["dec_block"] == 0.5 and full["roofline"]["avg_launch_ms"] == 0.5
    assert full["output_check"]["status"] == "no pinned digest for this workload"
    assert {k: full[k] for k in ("metric", "unit", "higher_is_better", "dtype")} == {k: plain[k] for k in ("metric", "unit", "higher_is_better", "dtype")}


def test_steps_below_one_are_refused(tmp_path):
    r = _run_bench(tmp_path, "--steps", "0")
    assert r.returncode != 0 and "--steps" in r.stderr
