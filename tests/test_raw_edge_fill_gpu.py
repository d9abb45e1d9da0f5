"""GPU: the raw-byte decimator's wide blocks with their edge lanes filled by the whole wavefront (tdm_debug_set
"raw_edge_fill" 1, the default: pz_raw_fill_edges) against the per-lane rolled loop the fill replaced ("raw_edge_fill" 0), on
the device itself.  Both hand the edge lanes the same integers, so the two settings have to agree BIT FOR BIT: soft symbols
(compared as bytes), hard symbols, counts, timing phases and margins, np.array_equal and no tolerance.

Shapes: the calls of tests/raw_edge_cases.py at every factor (three calls of the raw matrix -- odd strides, rows 2 bytes off
a dword, stride 0, two tail blocks -- and a row of one block, first and tail at once), each through the device-pointer entry
of the plan (tdm_process_device on the case's own pitched buffer) and through the host entry (tdm_process, rows back to
back); and 64 carriers x 262 144 samples at q = 10, the bench workload's row.

The switch is read at every call, so one plan serves both settings.  Every shape runs the sequence
    fill(data)  loop(other)  loop(data)  fill(other)  fill(data)
where `other` is the same layout with every byte inverted: a call that wrote nothing would leave the OTHER input's result
behind and fail the comparison, and the setting goes back and forth on the one plan with a comparison on either side.  That
the two settings run different code is not visible in the outputs, by design; tools/ab_switches.py shows it in the time.
"""
import ctypes as C

import numpy as np
import pytest

from tests import raw_edge_cases as rec
from tests import raw_matrix as rm

pytestmark = pytest.mark.gpu

CASES = rm.raw_cases()
SEQUENCE = ((1, "data"), (0, "other"), (0, "data"), (1, "other"), (1, "data"))


def _plan(rate, n, rows):
    from tetraear_amd._lib import debug_option
    from tetraear_amd.batch import BatchDemodulator
    with debug_option("raw_min_blocks", 0):
        bd = BatchDemodulator(rate, n, rows, "cu8")
    assert bd.info.dec_engine == 3, (rate, n, rows, "the plan did not take the raw-byte decimator")
    return bd


def _valid(hard, soft, n_soft, bp, mm):
    """what a call defines: per row the symbols it counted; soft symbols and margins as bytes (a NaN equals itself)"""
    out = [np.asarray(n_soft).copy(), np.asarray(bp).copy(), np.asarray(mm).view(np.uint8).copy()]
    for r in range(len(n_soft)):
        ns = int(n_soft[r])
        out.append(np.ascontiguousarray(soft[r][:ns]).view(np.uint8).copy())
        out.append(np.asarray(hard[r][:max(ns - 1, 0)]).copy())
    return out


def _equal(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _run_sequence(call, where):
    """call(which) -> _valid(...) under the setting in force; asserts the identities of the module docstring"""
    from tetraear_amd._lib import debug_option
    got = []
    for fill, which in SEQUENCE:
        with debug_option("raw_edge_fill", fill):
            got.append(call(which))
    fill_d, loop_o, loop_d, fill_o, fill_d2 = got
    assert int(fill_d[0].min()) >= 2, (where, fill_d[0])
    assert not _equal(fill_d, fill_o), f"{where}: the inverted input gave the same outputs: the comparison below would hold for a call that wrote nothing"
    assert _equal(fill_d, loop_d), f"{where}: raw_edge_fill 1 and 0 differ"
    assert _equal(fill_o, loop_o), f"{where}: raw_edge_fill 1 and 0 differ on the inverted input"
    assert _equal(fill_d, fill_d2), f"{where}: raw_edge_fill 1 after 0 differs from raw_edge_fill 1 before it"


def _device_sequence(bd, buf, n, stride, base, foffs, where):
    from tetraear_amd.batch import DeviceBuffer
    rows = bd.n_carriers
    assert 2 * (base + (rows - 1) * stride + n) == len(buf), "the last row must end with the allocation"
    bufs = {"data": buf, "other": np.bitwise_xor(buf, np.uint8(0xFF))}
    dbuf = DeviceBuffer(bd.device, len(buf))
    try:
        bd.alloc_device_io()
        bd.upload(buf[:2 * n], freq_offsets=foffs)    # (the offsets; the plan's own input buffer is not the one read)

        def call(which):
            dbuf.upload(bufs[which])
            bd.enqueue(iq_ptr=C.c_void_p(dbuf.ptr.value + 2 * base), stride=stride)
            return _valid(*bd.download())
        _run_sequence(call, where + " device entry")
    finally:
        bd.sync()
        dbuf.free()


def _host_sequence(bd, rows_bytes, foffs, where):
    bufs = {"data": rows_bytes, "other": np.bitwise_xor(rows_bytes, np.uint8(0xFF))}

    def call(which):
        hards, softs, bp, mm = bd.process(bufs[which], freq_offsets=foffs)
        return _valid(hards, softs, [len(s) for s in softs], bp, mm)
    _run_sequence(call, where + " host entry")


@pytest.mark.parametrize("q", sorted(CASES))
def test_edge_fill_on_off_bit_identical(q):
    rate = rm.RATE_OF_Q[q]
    for c in rec.cases(q):
        n, stride, base = c["n"], c["stride"], c["base"]
        bd = _plan(rate, n, rec.ROWS)
        try:
            _device_sequence(bd, c["buf"], n, stride, base, c["foffs"], c["where"])
            # the host entry takes rows back to back: the same rows, gathered
            rows_bytes = np.concatenate([rm.row_bytes(c["buf"], n, stride, base, r) for r in range(rec.ROWS)])
            _host_sequence(bd, rows_bytes, c["foffs"], c["where"])
        finally:
            bd.close()


def test_edge_fill_on_off_bit_identical_bench_row():
    """64 carriers x 262 144 samples at q = 10: 35 blocks a row, block 0 and block 34 wide"""
    from tetraear_amd import synth
    rows, n, rate = 64, 262144, rm.RATE_OF_Q[10]
    g = rm.geometry(10 * CASES[10], n)
    assert (g["nb"], g["b_tail"], g["tail"]) == (35, 34, 1), g
    u8 = synth.dqpsk_cu8_streams(n, rate, [5100 + r for r in range(rows)]).reshape(-1)
    foffs = [((r % 7) - 3) * 390.625 for r in range(rows)]
    bd = _plan(rate, n, rows)
    try:
        _device_sequence(bd, u8, n, n, 0, foffs, "64 x 262144")
        _host_sequence(bd, u8, foffs, "64 x 262144")
    finally:
        bd.close()
