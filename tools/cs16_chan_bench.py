"""The channeliser and the wideband receiver on cu8, cs16 and cf32 input, HIP-event timed on device-resident data; prints
one JSON line.

Config-5 geometry: 32 streams of 10 MS/s, 1 Mi samples each, M = 400, D = 125, output rows at the 16-aligned pitch.  The
channeliser writes 25.6 bytes per input sample whatever the format and reads 2 / 4 / 8 (cu8 / cs16 / cf32), so from bytes
alone cs16 lies between the other two.  In one process, after untimed passes until the clocks have settled:
  channelise   `reps` tdm_channelise_batch calls (device pointers) between two events on one plan's stream, per call
  receiver     `reps` WidebandReceiver.enqueue (channeliser + feed-forward receiver) the same way
The formats alternate run by run (cu8, cs16, cf32, cu8, ...), `runs` runs each.  The fraction of the box's copy ceiling
(tdm_hbm_ceiling, measured in the same process) is bytes read + written by the channeliser over time x ceiling.

    python tools/cs16_chan_bench.py [--runs 7] [--reps 20] [--out profiles/r13_cs16_channeliser.json]
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
from tetraear_amd.batch import BatchDemodulator, DeviceBuffer  # noqa: E402
from tetraear_amd.channeliser import aligned_pitch  # noqa: E402
from tetraear_amd.wideband import WidebandReceiver  # noqa: E402

M, D, S, R, FS = 400, 125, 32, 1 << 20, 10e6
FMTS = (("cu8", 0, 2), ("cs16", 4, 4), ("cf32", 2, 8))   # name, code, bytes per sample


def _input(name, rng):
    if name == "cu8":
        return rng.integers(0, 256, size=S * R * 2, dtype=np.uint8)
    if name == "cs16":
        return rng.integers(-8192, 8192, size=S * R * 2, dtype=np.int16)
    return (0.25 * rng.standard_normal(S * R * 2)).astype(np.float32)


def _stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": [round(float(x), 5) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--settle-seconds", type=float, default=0.4)
    ap.add_argument("--no-receiver", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    n_out = -(-R // D)
    pitch = aligned_pitch(n_out)
    rng = np.random.default_rng(13)
    g = (C.c_double * 3)()
    _lib.check(lib.tdm_hbm_ceiling(0, 1 << 30, 20, g))
    ceiling = float(g[0])
    timer = BatchDemodulator(FS / D, n_out, 1, "cf32", mode=_lib.MODE_TETRA)     # its stream and event pair time the calls
    d_in = {}
    d_out = DeviceBuffer(0, S * M * pitch * 8)
    rxs = {}
    try:
        for name, code, fb in FMTS:
            d_in[name] = DeviceBuffer(0, S * R * fb)
            d_in[name].upload(_input(name, rng))
        no = C.c_int64()

        def channelise(name, code, reps):
            for _ in range(reps):
                _lib.check(lib.tdm_channelise_batch(d_in[name].ptr, code, R, S, M, D, d_out.ptr, pitch, C.byref(no), 1, 0))

        timer.make_stream_current()
        try:
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < a.settle_seconds:               # clocks settle under the load that is timed
                for name, code, _ in FMTS:
                    channelise(name, code, 10)
                timer.sync()
            chan = {name: [] for name, _, _ in FMTS}
            for _ in range(a.runs):
                for name, code, _ in FMTS:
                    timer.time_begin(per_stage=False)
                    channelise(name, code, a.reps)
                    chan[name].append(timer.time_end() / a.reps)
        finally:
            timer.release_stream()
        res = {"tool": "cs16_chan_bench",
               "geometry": {"streams": S, "M": M, "D": D, "samples_per_stream": R, "pitch": pitch},
               "timing": f"HIP events on one stream around {a.reps} calls, per call; formats alternate, {a.runs} runs each, after "
                         f"{a.settle_seconds} s of untimed passes",
               "hbm_copy_ceiling_GBps": ceiling, "channelise_ms": {}, "channelise_fraction_of_ceiling": {}}
        for name, _, fb in FMTS:
            st = _stats(chan[name])
            res["channelise_ms"][name] = st
            moved = S * R * fb + S * M * n_out * 8
            res["channelise_fraction_of_ceiling"][name] = moved / (st["median"] * 1e-3) / 1e9 / ceiling
        if not a.no_receiver:
            for name, _, _ in FMTS:
                rxs[name] = WidebandReceiver(FS, R, M, D, streams=S, fmt=name)
                rxs[name].d_in.upload(_input(name, rng))
            for _ in range(3):
                for name, _, _ in FMTS:
                    rxs[name].enqueue()
                    rxs[name].sync()
            rec = {name: [] for name, _, _ in FMTS}
            for _ in range(a.runs):
                for name, _, _ in FMTS:
                    rx = rxs[name]
                    rx.demod.time_begin(per_stage=False)
                    for _ in range(max(a.reps // 4, 2)):
                        rx.enqueue()
                    rec[name].append(rx.demod.time_end() / max(a.reps // 4, 2))
            res["receiver_enqueue_ms"] = {name: _stats(rec[name]) for name, _, _ in FMTS}
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        for rx in rxs.values():
            rx.close()
        for b in list(d_in.values()) + [d_out]:
            b.free()
        timer.close()


if __name__ == "__main__":
    main()
