"""Stateful channeliser against the one-shot call, on the same device-resident data; prints one JSON line.

Config-5 geometry: 32 cu8 streams of 10 MS/s, M = 400, D = 125, reads of 1 Mi samples per stream.  In one process and
alternating round by round:
  one_shot   tdm_channelise_batch of one read (32 x 1 Mi), device pointers, row pitch 8400 (16-aligned)
  push       tdm_channeliser_push of the same reads, device pointers, same pitch: reset, then `reads` pushes in a row
Times are host clocks around `reads` calls that end in a device synchronise, divided by `reads`.  Every push's output is
checked against the one-shot over the whole concatenated stream: streams 0 and 31 after every round, all 32 after the
last.  The history kernel alone (k_pfb_hist) is timed by a separate `rocprofv3 --kernel-trace --stats` run of this tool.

    python tools/chan_stream_bench.py [--rounds 10] [--out profiles/r08_chan_stream_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tetraear_amd import _lib  # noqa: E402
from tetraear_amd.batch import DeviceBuffer  # noqa: E402
from tetraear_amd.channeliser import StreamingChanneliser, aligned_pitch  # noqa: E402

M, D, S, R = 400, 125, 32, 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reads", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    NR = a.reads
    N = NR * R
    n_all = -(-N // D)
    pitch = aligned_pitch(-(-R // D))
    rng = np.random.default_rng(8)
    u8 = rng.integers(0, 256, size=(NR, S, 2 * R), dtype=np.uint8)   # read r: [S][R], as a capture loop hands it over
    whole = np.ascontiguousarray(u8.transpose(1, 0, 2).reshape(S, 2 * N))
    d_reads = DeviceBuffer(0, u8.nbytes)
    d_whole = DeviceBuffer(0, whole.nbytes)
    d_one = DeviceBuffer(0, S * M * pitch * 8)                       # the timed one-shot's output
    d_ref = DeviceBuffer(0, S * M * n_all * 8)                       # one call over the whole stream: the check
    d_push = [DeviceBuffer(0, S * M * pitch * 8) for _ in range(NR)]
    try:
        d_reads.upload(u8)
        d_whole.upload(whole)
        no = C.c_int64()
        _lib.check(lib.tdm_channelise_batch(d_whole.ptr, 0, N, S, M, D, d_ref.ptr, 0, C.byref(no), 1, 0))
        assert no.value == n_all
        _lib.check(lib.tdm_dev_sync(0))
        ch = StreamingChanneliser(M, D, "cu8", streams=S, max_n_in=R)
        read_ptr = [d_reads.ptr.value + r * S * 2 * R for r in range(NR)]

        def one_shot():
            for r in range(NR):
                _lib.check(lib.tdm_channelise_batch(read_ptr[r], 0, R, S, M, D, d_one.ptr, pitch, C.byref(no), 1, 0))
            _lib.check(lib.tdm_dev_sync(0))

        def pushes():
            ch.reset()
            ns = [ch.push_device(read_ptr[r], R, d_push[r].ptr, pitch) for r in range(NR)]
            _lib.check(lib.tdm_dev_sync(0))
            return ns

        def check(streams):
            done = 0
            for r in range(NR):
                k = -(-(r + 1) * R // D) - done
                for y in streams:
                    got = np.empty((M, pitch), dtype=np.complex64)
                    ref = np.empty((M, n_all), dtype=np.complex64)
                    _lib.check(lib.tdm_dev_download(0, _lib.ptr(got), d_push[r].ptr.value + 8 * y * M * pitch, got.nbytes))
                    _lib.check(lib.tdm_dev_download(0, _lib.ptr(ref), d_ref.ptr.value + 8 * y * M * n_all, ref.nbytes))
                    if not np.array_equal(got[:, :k], ref[:, done:done + k]):
                        raise SystemExit(f"push {r} stream {y} differs from the one-shot over the whole stream")
                done += k
            return len(streams) * NR

        for _ in range(2):                                           # warm-up: code objects, tables, LDS attributes
            one_shot()
            pushes()
        t_one, t_push, checked = [], [], 0
        for i in range(a.rounds):
            t0 = time.perf_counter()
            one_shot()
            t1 = time.perf_counter()
            ns = pushes()
            t2 = time.perf_counter()
            assert sum(ns) == n_all, ns
            t_one.append((t1 - t0) * 1e3 / NR)
            t_push.append((t2 - t1) * 1e3 / NR)
            checked += check([0, S - 1] if i + 1 < a.rounds else list(range(S)))
        ch.close()
        med_one, med_push = float(np.median(t_one)), float(np.median(t_push))
        res = {"tool": "chan_stream_bench", "geometry": {"streams": S, "M": M, "D": D, "read": R, "fmt": "cu8",
                                                         "reads_per_round": NR, "pitch": pitch},
               "rounds": a.rounds, "timing": "host clock around reads_per_round calls ending in a device synchronise, per call",
               "one_shot_ms": {"median": med_one, "min": min(t_one), "max": max(t_one)},
               "push_ms": {"median": med_push, "min": min(t_push), "max": max(t_push)},
               "push_over_one_shot": med_push / med_one,
               "checked": f"{checked} (push, stream) blocks equal to one call over the whole {NR}-read stream, bit for bit"}
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        for b in [d_reads, d_whole, d_one, d_ref] + d_push:
            b.free()


if __name__ == "__main__":
    main()
