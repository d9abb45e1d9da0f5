"""Host-fed rate of the persistent stream (tdm_stream_* / StreamingDemodulator) against the measured host link.

One JSON line (also written to --out):
  - h2d_ceiling_GBps: tdm_link_ceiling over 1 GiB (host->device, device->host, both at once);
  - stream: reference mode, cu8, 256 carriers x 262 144 samples per batch (128 MiB), depth 2 and 3, each
      "prefilled": every slot filled once with its own batch, then re-submitted as it is (the engine and the link alone),
      "filled":    every batch copied into the acquired page-locked slot before its submit (--fill-threads threads),
    >= 16 batches and >= 1 s after warm-up batches; Msym/s, H2D GB/s and the fraction of the measured H2D ceiling;
    and the same two with write-combined slot inputs (tdm_debug_set "stream_wc" 1) as an A/B;
  - process_stream: the same batches through tdm_process_pipelined (pageable input, 8 batches per call);
  - recording: a 10 s config-1 recording (24 M cu8 samples, tetraear_amd.synth) through iter_recording with
    overlapped=False and overlapped=True.
Every streamed batch is compared with a blocking tdm_process of the same batch (hard symbols, n_soft, best_phase,
min_margin); any mismatch exits non-zero.

    python tools/host_fed_bench.py [--quick] [--out profiles/r07_host_fed_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tetraear_amd import _lib  # noqa: E402
from tetraear_amd.batch import BatchDemodulator  # noqa: E402
from tetraear_amd.stream import StreamingDemodulator  # noqa: E402

FS = 2.4e6


def digest(hards, bp, mm):
    """what a batch's result is compared by: every row's hard symbols, n_soft (via their length), best_phase, min_margin"""
    return [h.tobytes() for h in hards], np.asarray(bp).tobytes(), np.asarray(mm).tobytes()


def run_stream(pool, refs, chunk, rows, foffs, depth, fill, min_batches, min_seconds, warmup, pool_fill):
    """-> (result dict, mismatches)"""
    sd = StreamingDemodulator(FS, chunk, rows, "cu8", depth=depth, freq_offsets=foffs)
    which = {}         # seq -> pool index of its input
    got = {}

    def collect():
        seq, hards, _, bp, mm = sd.collect()
        got[seq] = digest(hards, bp, mm)
        return seq, sum(len(h) for h in hards)

    try:
        seq = 0
        t0 = None
        timed_from = warmup
        timed_sym = 0
        while True:
            if seq == timed_from:
                while sd.in_flight:          # warm-up drained: the timed window starts on an idle device
                    collect()
                t0 = time.perf_counter()
            if t0 is not None and seq - timed_from >= min_batches and time.perf_counter() - t0 >= min_seconds:
                break
            if sd.in_flight == depth:
                s, k = collect()
                if s >= timed_from:
                    timed_sym += k
            buf = sd.input_buffer()
            if fill or seq < depth:
                idx = seq % len(pool) if fill else seq % depth
                pool_fill(buf, pool[idx])
            which[seq] = (seq % len(pool)) if fill else (seq % depth)
            sd.submit()
            seq += 1
        while sd.in_flight:
            s, k = collect()
            if s >= timed_from:
                timed_sym += k
        dt = time.perf_counter() - t0
    finally:
        sd.close()
    n_timed = seq - timed_from
    bad = [s for s in got if got[s] != refs[which[s]]]
    gb = n_timed * pool[0].nbytes / 1e9
    return {"depth": depth, "batches": n_timed, "seconds": dt, "Msym_per_s": timed_sym / dt / 1e6, "h2d_GBps": gb / dt,
            "checked_batches": len(got)}, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=262144)
    ap.add_argument("--min-batches", type=int, default=16)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--fill-threads", type=int, default=8)
    ap.add_argument("--quick", action="store_true", help="the depth-3 prefilled stream only (for a trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    rows, chunk = args.rows, args.chunk
    out = {"tool": "tools/host_fed_bench.py", "argv": sys.argv[1:],
           "workload": f"reference mode, cu8, {rows} carriers x {chunk} samples per batch ({2 * rows * chunk / 2**20:.0f} MiB)"}

    gbs = (C.c_double * 3)()
    _lib.check(lib.tdm_link_ceiling(0, 1 << 30, 10, gbs))
    ceiling = gbs[0]
    out["h2d_ceiling_GBps"] = {"h2d": gbs[0], "d2h": gbs[1], "both": gbs[2], "bytes": 1 << 30,
                               "how": "hipMemcpyAsync hipHostMalloc <-> device, 10 timed copies after 2, HIP events"}

    rng = np.random.default_rng(2026)
    pool = [rng.integers(0, 256, 2 * rows * chunk, dtype=np.uint8) for _ in range(4)]
    foffs = np.linspace(-2900.0, 2900.0, rows)
    bd = BatchDemodulator(FS, chunk, rows, "cu8")
    refs = []
    for b in pool:
        hards, _, bp, mm = bd.process(b, freq_offsets=foffs)
        refs.append(digest(hards, bp, mm))

    chunks_of = max(1, args.fill_threads)
    ex = ThreadPoolExecutor(chunks_of)

    def pool_fill(dst, src):
        step = -(-len(src) // chunks_of)
        list(ex.map(lambda i: np.copyto(dst[i:i + step], src[i:i + step]), range(0, len(src), step)))

    # host-side fill rate (what "filled" pays per batch on this host)
    dst = np.empty_like(pool[0])
    t = time.perf_counter()
    for i in range(8):
        pool_fill(dst, pool[i % 4])
    out["host_fill_GBps"] = 8 * pool[0].nbytes / (time.perf_counter() - t) / 1e9
    del dst

    mismatched = []
    runs = []
    configs = [(3, False, 0)] if args.quick else [(3, False, 0), (3, True, 0), (2, False, 0), (2, True, 0), (3, False, 1), (3, True, 1)]
    for depth, fill, wc in configs:
        with _lib.debug_option("stream_wc", wc):
            r, bad = run_stream(pool, refs, chunk, rows, foffs, depth, fill, args.min_batches, args.min_seconds, args.warmup, pool_fill)
        r.update({"inputs": "filled" if fill else "prefilled", "write_combined": bool(wc), "fraction_of_h2d_ceiling": r["h2d_GBps"] / ceiling})
        runs.append(r)
        if bad:
            mismatched.append({"run": r, "seqs": bad[:16]})
        print(json.dumps(r), file=sys.stderr, flush=True)
    out["stream"] = runs

    if not args.quick:
        # tdm_process_pipelined beside it: 8 batches per call from pageable memory
        nb = 8
        allq = np.concatenate([pool[i % 4] for i in range(nb)])
        bd.process_stream(allq, nb, foffs)
        reps, t = 0, time.perf_counter()
        while reps < 2 or time.perf_counter() - t < args.min_seconds:
            hard, soft, n_soft, bp, mm = bd.process_stream(allq, nb, foffs)
            reps += 1
        dt = time.perf_counter() - t
        for b in range(nb):
            hs = [hard[b, r, :max(int(n_soft[b, r]) - 1, 0)] for r in range(rows)]
            if digest(hs, bp[b], mm[b]) != refs[b % 4]:
                mismatched.append({"run": "process_stream", "batch": b})
        nsym = int(np.sum(np.maximum(n_soft.astype(np.int64) - 1, 0))) * reps
        out["process_stream"] = {"batches": nb * reps, "seconds": dt, "Msym_per_s": nsym / dt / 1e6,
                                 "h2d_GBps": allq.nbytes * reps / dt / 1e9,
                                 "fraction_of_h2d_ceiling": allq.nbytes * reps / dt / 1e9 / ceiling}

        # a 10 s config-1 recording through iter_recording, both paths
        from tetraear_amd import synth
        from tetraear_amd.ingest import demodulate_recording
        u8, _ = synth.dqpsk_cu8(24_000_000, FS, seed=11)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "config1.cu8")
            u8.tofile(path)
            rec = {"samples": 24_000_000, "seconds_of_signal": 24_000_000 / FS, "chunk": 262144, "rows_per_batch": 64}
            outs = {}
            for rep in range(2):       # (the second pass is the one reported: plans and page cache warm)
                for ov in (False, True):
                    t = time.perf_counter()
                    outs[ov] = demodulate_recording(path, FS, chunk=262144, freq_offset=0.0, rows_per_batch=64, overlapped=ov)
                    rec["overlapped" if ov else "default"] = {"seconds": time.perf_counter() - t, "reads": len(outs[ov])}
            t = time.perf_counter()       # (what the overlapped path pays once per recording: three plans, three pinned slots)
            StreamingDemodulator(FS, 262144, 64, "cu8", depth=3, freq_offsets=[0.0] * 64).close()
            rec["stream_create_and_close_seconds"] = time.perf_counter() - t
            same = len(outs[False]) == len(outs[True]) and all(np.array_equal(a, b) for a, b in zip(outs[False], outs[True]))
            rec["identical_yields"] = same
            if not same:
                mismatched.append({"run": "recording"})
            out["recording"] = rec
    bd.close()
    ex.shutdown()
    out["mismatches"] = mismatched
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 1 if mismatched else 0


if __name__ == "__main__":
    sys.exit(main())
