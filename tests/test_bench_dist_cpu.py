"""CPU tier, world size 2: bench.py's multi-rank control flow end to end -- environment of torch.distributed.run, the
librccl group (against the stub library, host memory), sharding, the three reductions, ONE JSON line on rank 0 -- with
the device replaced by a stand-in that returns fixed outputs.  Two scenarios: a clean run, and a run in which rank 1's
output check fails: BOTH ranks must stop with the failure (no rank left waiting in an all-reduce)."""
import json
import multiprocessing as mp
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STUB = os.path.join(HERE, "rccl_stub", "librccl_stub.so")


@pytest.fixture(scope="module", autouse=True)
def _build_stub():
    subprocess.run(["make", "-C", os.path.join(HERE, "rccl_stub")], check=True, capture_output=True)


class _Info:
    n_dec, dec_engine, max_soft = 410, 3, 34


class FakeBatchDemodulator:
    """what bench.main() touches of BatchDemodulator, without a device"""

    def __init__(self, rate, chunk, carriers, fmt, device=0, **kw):
        self.carriers, self.info = carriers, _Info()
        self.rank = int(os.environ.get("RANK", "0"))

    def sync(self): pass
    def wait_for(self, other): pass
    def alloc_device_io(self, shared_input=False): pass
    def upload(self, iq, freq_offsets=None, pre_shifts=None): pass
    def enqueue(self): pass
    def time_begin(self, per_stage=True): pass
    def time_end(self): return 1.0 + self.rank
    def stage_times(self): return {"dec_block": 0.5, "dec_carry": 0.01, "lpf_block": 0.3, "finish": 0.03}
    def close(self): pass

    def download(self):
        rows, ms = self.carriers, self.info.max_soft
        hard = np.full((rows, ms), self.rank, dtype=np.uint8)
        n_soft = np.full(rows, 30 + self.rank, dtype=np.int32)
        return hard, np.zeros((rows, ms), np.complex128), n_soft, np.zeros(rows, np.int32), np.zeros(rows)


class _HostMem:
    def __init__(self, device=0):
        import ctypes as C
        self.C = C
        self.buf = (C.c_byte * 16)()
        self.ptr = C.cast(self.buf, C.c_void_p)

    def upload(self, v): self.C.memmove(self.buf, self.C.byref(v), 8)
    def download(self, v): self.C.memmove(self.C.byref(v), self.buf, 8)
    def free(self): pass


def _rank(rank, world, port, bad_rank, q, strong=False):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), TORCHELASTIC_RUN_ID="benchdist", TDM_RCCL_LIB=STUB)
    sys.path.insert(0, ROOT)
    import io
    import contextlib
    import bench
    import tetraear_amd.batch as batch
    import tetraear_amd.rccl as rccl
    batch.BatchDemodulator = FakeBatchDemodulator
    rccl.DeviceMemory = _HostMem
    bench.make_batch = lambda carriers, chunk, fmt, first=0, workers=None: (np.zeros(2 * carriers * chunk, np.uint8), np.zeros(carriers))
    if bad_rank is not None:
        # a pinned digest that rank `bad_rank`'s output cannot have
        real = bench.expected_digest
        bench.expected_digest = lambda key: ("0" * 64 if f"rank{bad_rank}" in key else None)
    sys.argv = ["bench.py", "--gpus", str(world), "--steps", "2", "--warmup", "1", "--carriers", "4", "--chunk", "4096",
                "--no-cpu-baseline"]
    if bad_rank is not None or strong:
        sys.argv.append("--full")   # (the output check runs in a full run only)
    if strong:
        # BASELINE config 4's split: ONE job of 8 carriers over the ranks; the slice digests are pinned under keys that
        # name the slice (":strong{lo}-{hi}of{T}") -- here pinned to what the stand-in device returns for that rank
        sys.argv += ["--total-carriers", "8"]

        def pinned(key):
            if f":strong{4 * rank}-{4 * rank + 4}of8" not in key or f"rank{rank}" not in key:
                return None
            fake = FakeBatchDemodulator(0, 0, 4, "cu8")
            hard, _, n_soft, bp, _ = fake.download()
            return bench.output_digest(hard, n_soft, bp)
        bench.expected_digest = pinned
    out = io.StringIO()
    status = "ok"
    try:
        with contextlib.redirect_stdout(out):
            bench.main()
    except SystemExit as e:
        status = f"exit: {e}"
    q.put((rank, status, out.getvalue()))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(bad_rank, strong=False):
    ctx = mp.get_context("fork")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, bad_rank, q, strong)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    return res


@pytest.mark.timeout(180)
def test_two_rank_bench_prints_one_line_with_job_totals():
    (r0, s0, o0), (r1, s1, o1) = _run(None)
    assert s0 == "ok" and s1 == "ok"
    assert o1.strip() == ""                                    # only rank 0 prints
    lines = [l for l in o0.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["scaling"] == "weak"
    assert "librccl via ctypes" in d["config"]["collective"]
    # symbols of both ranks: 4 carriers x (29 + 30), over the slower rank's elapsed time
    assert d["value"] > 0 and d["config"]["carriers_per_gpu"] == 4
    assert "cpu_baseline" not in d and "tetra" not in d        # N = 1 only
    assert d["full"] is False and "output_check" not in d and "roofline" not in d   # a plain run: the headline only


@pytest.mark.timeout(180)
def test_failed_output_check_on_one_rank_stops_both():
    (r0, s0, o0), (r1, s1, o1) = _run(1)
    assert s0.startswith("exit:") and "1 rank" in s0, s0       # rank 0's own check passed; it learns of rank 1's failure
    assert s1.startswith("exit:") and "1 rank" in s1, s1
    assert not [l for l in o0.splitlines() if l.startswith("{")]   # no result line for a failed job


@pytest.mark.timeout(180)
def test_two_rank_strong_scaling_checks_its_slice_digests():
    """`bench.py --gpus 2 --total-carriers 8`: each rank looks its output up under the key of ITS slice of the job, and the
    line says the check ran ("matches"), not "no pinned digest" (round-3 VERDICT: the strong-scaling run had no output check)."""
    (r0, s0, o0), (r1, s1, o1) = _run(None, strong=True)
    assert s0 == "ok" and s1 == "ok", (s0, s1)
    d = json.loads([l for l in o0.strip().splitlines() if l.startswith("{")][0])
    assert d["scaling"] == "strong" and d["n_gpus"] == 2 and d["config"]["carriers_per_gpu"] == 4
    assert d["output_check"]["key"].endswith(":rank0:strong0-4of8"), d["output_check"]
    assert d["output_check"]["status"] == "matches oracle-pinned digest"


def test_pinned_digests_cover_config_4_weak_and_strong():
    """tests/golden/bench_digest.json (written on the GPU box by tools/make_bench_digest.py after 1024 oracle comparisons
    per rank) holds the headline key of every rank and every slice key of the 2-, 4- and 8-GPU strong-scaling splits."""
    sys.path.insert(0, ROOT)
    import bench
    from tetraear_amd.shard import carrier_range
    for rank in range(8):
        assert bench.expected_digest(bench.digest_key(1024, 262144, "cu8", bench.SAMPLE_RATE, rank, False)), rank
    for world in (2, 4, 8):
        for r in range(world):
            lo, hi = carrier_range(1024, r, world)
            key = bench.digest_key(hi - lo, 262144, "cu8", bench.SAMPLE_RATE, r, False) + f":strong{lo}-{hi}of1024"
            assert bench.expected_digest(key), key


@pytest.mark.timeout(240)
def test_bench_gpus_2_as_a_plain_command_spawns_its_own_ranks():
    """`python bench.py --gpus 2 ...` with NO launcher around it (round-4 VERDICT: --gpus was parsed and never read, so a driver
    calling it that way got one rank and n_gpus: 1): the command spawns two local ranks itself, they meet through RcclGroup
    (stub librccl), and rank 0 prints ONE line that says n_gpus 2 / rccl_ranks 2.  A launcher whose world size contradicts
    --gpus is refused."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(TDM_RCCL_LIB=STUB, TDM_BENCH_TEST_HOOK=os.path.join(HERE, "bench_fake_device.py"), PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--carriers", "4",
           "--chunk", "4096", "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=200, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["config"]["carriers_per_gpu"] == 4
    assert "librccl via ctypes" in d["config"]["collective"]
    # a line printed under the test hook says so itself (round-5 VERDICT: the stand-in's line looked like a measurement)
    assert d["test_hook"].endswith("bench_fake_device.py") and d["data"].startswith("test hook")
    # --gpus 2 under a launcher that started ONE rank: no line, non-zero exit
    r = subprocess.run(cmd, env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=100, cwd=ROOT)
    assert r.returncode != 0 and "refusing to report" in (r.stderr + r.stdout)
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.mark.timeout(240)
def test_bench_gpus_2_default_workload_is_config_4_as_written():
    """`python bench.py --gpus 2` with no workload flags -- the only form the driver runs: the headline is BASELINE config 4 as
    written, ONE job of 1024 carriers block-partitioned over the ranks (512 each, scaling "strong", slice digests), and the
    weak-scaling figure (every rank its own 1024) rides beside it as the side field `weak` (round-5 review).  At N = 1 the
    default stays the 1024-carrier batch on the one GPU."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(TDM_RCCL_LIB=STUB, TDM_BENCH_TEST_HOOK=os.path.join(HERE, "bench_fake_device.py"), PYTHONPATH=ROOT,
               TDM_BENCH_NO_PINNED="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--chunk", "4096", "--no-cpu-baseline",
           "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=200, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["total_carriers"] == 1024
    assert d["config"]["carriers_per_gpu"] == 512 and "strong0-512of1024" in d["output_check"]["key"]
    assert d["config"]["steps_in_flight"]["plans"] == 3
    assert d["weak"]["scaling"] == "weak" and d["weak"]["total_carriers"] == 2048 and d["weak"]["carriers_per_gpu"] == 1024
    assert d["test_hook"].endswith("bench_fake_device.py")
    # explicit --carriers keeps weak scaling, no side run
    r = subprocess.run(cmd + ["--carriers", "4"], env=env, capture_output=True, text=True, timeout=200, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["scaling"] == "weak" and d["total_carriers"] == 8 and "weak" not in d
    # a plain run (no --full): the same strong-scaling headline, without the weak-scaling side run or the output check
    r = subprocess.run(cmd[:-1], env=env, capture_output=True, text=True, timeout=200, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["scaling"] == "strong" and d["total_carriers"] == 1024 and d["config"]["carriers_per_gpu"] == 512
    assert "weak" not in d and "output_check" not in d and d["full"] is False
