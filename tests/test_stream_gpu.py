"""GPU: the persistent host-fed stream (StreamingDemodulator / tdm_stream_*) held to the oracle and to tdm_process.

Every batch and every row carries distinct data and every row its own freq_offset, so input copied from the wrong slot,
outputs read from the wrong slot or a missing wait shows up as a mismatch.
"""
import ctypes as C
import gc
import math
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SOFT_TOL = 1e-10
FS = 2.4e6
N_RAGGED = 65536 + 13
ROWS = 5
FOFFS = np.array([-2750.0, -1171.875, 0.0, 613.5, 2990.25])


def _x_of(b, r, n=N_RAGGED, salt=0):
    from tetraear_amd import synth
    return synth.noise_cu8(n, 70000 + 1000 * salt + 100 * b + r)


def _check_oracle(u8, foff, hard, soft, bp, mm, what):
    from oracle.oracle import OracleSignalProcessor
    from tetraear_amd import synth
    o = OracleSignalProcessor(FS)
    ref = o.process(synth.cu8_to_c128(u8), foff)
    np.testing.assert_array_equal(hard, ref, err_msg=what)
    if len(o.symbols) == 0:
        assert len(soft) == 0, what
        return
    assert len(soft) == len(o.symbols), what
    assert np.max(np.abs(soft - o.symbols)) <= SOFT_TOL * np.max(np.abs(o.symbols)), what
    assert int(bp) == o.best_phase, what
    assert abs(float(mm) - o.min_margin) <= 1e-9, what


def _full(bd, iq, n, fo=None, ps=None):
    """tdm_process of one batch on a lone plan, full outputs (rows x max_soft)"""
    from tetraear_amd._lib import check, ptr
    rows, ms = bd.n_carriers, bd.info.max_soft
    iq = np.ascontiguousarray(iq)
    fo = None if fo is None else np.ascontiguousarray(fo, dtype=np.float64)
    ps = None if ps is None else np.ascontiguousarray(ps, dtype=np.float64)
    hard = np.zeros((rows, ms), dtype=np.uint8)
    soft = np.zeros((rows, ms), dtype=bd.soft_dtype)
    ns, bp, mm = np.zeros(rows, np.int32), np.zeros(rows, np.int32), np.zeros(rows, np.float64)
    check(bd.lib.tdm_process(bd.handle, ptr(iq), n, ptr(ps), ptr(fo), ptr(hard), ptr(soft), ptr(ns), ptr(bp), ptr(mm)))
    return hard, soft, ns, bp, mm


def _equal(got, want, what, rows=None, soft=True):
    """a collect() result == tdm_process outputs, bit for bit, over the first `rows` rows"""
    _, hards, softs, bp, mm = got
    hard, sft, ns, wbp, wmm = want
    rows = len(hards) if rows is None else rows
    for r in range(rows):
        k = int(ns[r])
        np.testing.assert_array_equal(hards[r], hard[r, :max(k - 1, 0)], err_msg=f"{what} row {r}")
        if soft:
            np.testing.assert_array_equal(softs[r], sft[r, :k], err_msg=f"{what} row {r}")
        assert bp[r] == wbp[r] and mm[r] == wmm[r], (what, r)
    if soft:
        assert softs is not None
    else:
        assert softs is None


# ---- reference mode, cu8, against the oracle ------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [2, 3])
def test_stream_cu8_every_batch_and_row_vs_oracle(depth):
    """9 batches x 5 rows of a ragged chunk (the 8th with 3 valid inputs), then short reads of 28 and of 1 sample; depth
    steps in flight, collected late"""
    from tetraear_amd.stream import StreamingDemodulator
    nb = 9
    xs = [[_x_of(b, r) for r in range(ROWS)] for b in range(nb)]
    valid = [ROWS] * nb
    valid[7] = 3
    outs = {}
    with StreamingDemodulator(FS, N_RAGGED, ROWS, "cu8", depth=depth, soft=True, freq_offsets=FOFFS) as sd:
        for b in range(nb):
            if sd.in_flight == depth:
                got = sd.collect()
                outs[got[0]] = got
            buf = sd.input_buffer()
            buf[:] = 0
            buf[:2 * N_RAGGED * valid[b]] = np.concatenate(xs[b][:valid[b]])
            assert sd.submit(n_inputs=valid[b]) == b
        tails = []
        for b, n in ((nb, 28), (nb + 1, 1)):
            if sd.in_flight == depth:
                got = sd.collect()
                outs[got[0]] = got
            u8 = _x_of(b, 0, n=n)
            tails.append(u8)
            sd.submit_array(u8, n_samples=n)
        full = _x_of(nb + 2, 0)          # and a full read after them: the slot's plan is resized back
        while sd.in_flight == depth:
            got = sd.collect()
            outs[got[0]] = got
        sd.input_buffer()[:2 * N_RAGGED] = full
        sd.submit(n_inputs=1)
        while sd.in_flight:
            got = sd.collect()
            outs[got[0]] = got
    assert sorted(outs) == list(range(nb + 3))
    for b in range(nb):
        _, hards, softs, bp, mm = outs[b]
        for r in range(ROWS):
            if r < valid[b]:
                _check_oracle(xs[b][r], FOFFS[r], hards[r], softs[r], bp[r], mm[r], f"depth {depth} batch {b} row {r}")
            else:
                assert len(hards[r]) == 0 and len(softs[r]) == 0 and bp[r] == 0, (b, r)
    for i, u8 in enumerate(tails):
        _, hards, softs, bp, mm = outs[nb + i]
        _check_oracle(u8, FOFFS[0], hards[0], softs[0], bp[0], mm[0], f"short read {len(u8) // 2}")
        assert all(len(h) == 0 for h in hards[1:])
    assert len(outs[nb + 1][1][0]) == 0       # (the reference returns an empty array for a 1-sample read)
    _, hards, softs, bp, mm = outs[nb + 2]
    _check_oracle(full, FOFFS[0], hards[0], softs[0], bp[0], mm[0], "full read after the short ones")


# ---- other formats and modes: bit for bit against tdm_process ------------------------------------------------------------

def _batches(fmt, nb, n, rows, salt):
    from tetraear_amd import synth
    out = []
    for b in range(nb):
        rs = []
        for r in range(rows):
            u8 = _x_of(b, r, n=n, salt=salt)
            if fmt == "cu8":
                rs.append(u8)
            elif fmt == "cs8":
                rs.append(u8.view(np.int8))
            else:
                rs.append(synth.cu8_to_c128(u8).astype(np.complex64 if fmt == "cf32" else np.complex128))
        out.append(np.concatenate(rs))
    return out


def _run(sd, batches):
    """submit every batch, collecting only when the ring is full (late), return results by seq"""
    outs = {}
    for b in batches:
        if sd.in_flight == sd.depth:
            got = sd.collect()
            outs[got[0]] = got
        sd.submit_array(b)
    while sd.in_flight:
        got = sd.collect()
        outs[got[0]] = got
    return [outs[k] for k in sorted(outs)]


@pytest.mark.parametrize("fmt", ["cs8", "cf32", "cf64"])
@pytest.mark.parametrize("soft", [False, True])
def test_stream_other_formats_equal_tdm_process(fmt, soft):
    from tetraear_amd.batch import BatchDemodulator
    from tetraear_amd.stream import StreamingDemodulator
    batches = _batches(fmt, 5, N_RAGGED, ROWS, salt=1)
    with StreamingDemodulator(FS, N_RAGGED, ROWS, fmt, depth=3, soft=soft, freq_offsets=FOFFS) as sd:
        got = _run(sd, batches)
    bd = BatchDemodulator(FS, N_RAGGED, ROWS, fmt)
    for b, g in enumerate(got):
        _equal(g, _full(bd, batches[b], N_RAGGED, FOFFS), f"{fmt} soft {soft} batch {b}", soft=soft)
    bd.close()


@pytest.mark.parametrize("mode_name", ["MODE_TETRA", "MODE_TETRA_GARDNER"])
@pytest.mark.parametrize("soft", [False, True])
def test_stream_tetra_modes_equal_tdm_process(mode_name, soft):
    from tetraear_amd import _lib, synth
    from tetraear_amd.batch import BatchDemodulator
    from tetraear_amd.stream import StreamingDemodulator
    fs, n, rows, nb = 72000.0, 16384, 3, 4
    batches = []
    for b in range(nb):
        xs = []
        for r in range(rows):
            x, _ = synth.dqpsk_baseband(n, fs, 800 + 10 * b + r, timing_offset=0.1 * r - 0.15 * b)
            rng = np.random.default_rng(950 + 10 * b + r)
            xs.append((x + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64))
        batches.append(np.concatenate(xs))
    mode = getattr(_lib, mode_name)
    with StreamingDemodulator(fs, n, rows, "cf32", mode=mode, depth=2, soft=soft) as sd:
        got = _run(sd, batches)
        # a short read is refused in a TETRA mode, and the stream goes on
        sd.input_buffer()[:n - 100] = batches[0][:n - 100]
        with pytest.raises(_lib.TetraHipError) as e:
            sd.submit(n_samples=n - 100, n_inputs=1)
        assert e.value.code == _lib.TDM_ERR_UNSUPPORTED
        sd.input_buffer()[:] = batches[1]
        sd.submit()
        again = sd.collect()
    bd = BatchDemodulator(fs, n, rows, "cf32", mode=mode)
    for b, g in enumerate(got):
        _equal(g, _full(bd, batches[b], n), f"{mode_name} soft {soft} batch {b}", soft=soft)
    _equal(again, _full(bd, batches[1], n), f"{mode_name} after a refused short read", soft=soft)
    bd.close()


def test_stream_pre_shifts_rows_per_chunk_equal_tdm_process():
    """config-3 style: 3 carriers out of each of 4 reads per batch (rows_per_chunk 3), a remainder batch of 2 reads and a short
    last read, against tdm_process on a plan with the same option"""
    from tetraear_amd import synth
    from tetraear_amd.batch import BatchDemodulator
    from tetraear_amd.stream import StreamingDemodulator
    offs = np.array([-312500.0, 62500.0, 287500.0])
    reads, C3 = 4, 3
    rows = reads * C3
    pre = np.tile(offs, reads)
    fo = np.linspace(-900.0, 1300.0, rows)
    u8, _ = synth.multicarrier_cu8(11 * N_RAGGED, FS, list(offs), seed0=460)
    rd = [u8[2 * N_RAGGED * i:2 * N_RAGGED * (i + 1)] for i in range(11)]
    steps = [np.concatenate(rd[0:4]), np.concatenate(rd[4:8]), np.concatenate(rd[8:10])]
    with StreamingDemodulator(FS, N_RAGGED, rows, "cu8", soft=True, freq_offsets=fo, pre_shifts=pre, rows_per_chunk=C3) as sd:
        got = _run(sd, steps)
        tail = rd[10][:2 * 30011]
        sd.submit_array(tail, n_samples=30011)
        got_tail = sd.collect()
    bd = BatchDemodulator(FS, N_RAGGED, rows, "cu8").set_rows_per_chunk(C3)
    for b, g in enumerate(got):
        k = len(steps[b]) // (2 * N_RAGGED)
        iq = np.concatenate([steps[b], np.zeros(2 * N_RAGGED * (reads - k), np.uint8)])
        _equal(g, _full(bd, iq, N_RAGGED, fo, pre), f"rows_per_chunk batch {b}", rows=k * C3)
        assert all(len(h) == 0 for h in g[1][k * C3:])
    bd.resize(30011)
    iq = np.concatenate([tail, np.zeros(2 * 30011 * (reads - 1), np.uint8)])
    _equal(got_tail, _full(bd, iq, 30011, fo, pre), "rows_per_chunk short read", rows=C3)
    bd.close()


def test_stream_overwrite_race_collect_late():
    """Large rows (kernels take longer than a host fill): the next slots are filled and submitted while the earlier steps are
    still on the device, results collected only when the ring is full -- and a second pass collects them all at the very
    end of depth submits.  Every result equals its own batch."""
    from tetraear_amd.batch import BatchDemodulator
    from tetraear_amd.stream import StreamingDemodulator
    n, rows, nb = 262144, 48, 7
    fo = np.linspace(-2500.0, 2500.0, rows)
    batches = [np.concatenate([_x_of(b, r, n=n, salt=7) for r in range(rows)]) for b in range(nb)]
    with StreamingDemodulator(FS, n, rows, "cu8", depth=3, freq_offsets=fo) as sd:
        got = _run(sd, batches)
        late = []
        for b in range(3):
            sd.submit_array(batches[nb - 1 - b])
        for b in range(3):
            late.append(sd.collect())
    bd = BatchDemodulator(FS, n, rows, "cu8")
    want = [_full(bd, batches[b], n, fo) for b in range(nb)]
    for b, g in enumerate(got):
        _equal(g, want[b], f"race batch {b}", soft=False)
    for b, g in enumerate(late):
        _equal(g, want[nb - 1 - b], f"late batch {b}", soft=False)
    bd.close()


def test_stream_protocol_errors_leave_it_usable():
    from tetraear_amd import _lib
    from tetraear_amd.batch import BatchDemodulator
    from tetraear_amd.stream import StreamingDemodulator
    batches = _batches("cu8", 6, N_RAGGED, ROWS, salt=8)
    bd = BatchDemodulator(FS, N_RAGGED, ROWS, "cu8")
    want = [_full(bd, b, N_RAGGED, FOFFS) for b in batches]
    bd.close()
    sd = StreamingDemodulator(FS, N_RAGGED, ROWS, "cu8", depth=2, freq_offsets=FOFFS)
    L = sd.lib
    r = _lib.StreamResult()
    # collecting with nothing in flight
    assert L.tdm_stream_collect(sd.handle, 1, C.byref(r)) == _lib.TDM_ERR_INVALID
    assert "nothing in flight" in _lib.last_error()
    # n_samples > chunk
    sd.input_buffer()[:] = batches[0]
    assert L.tdm_stream_submit(sd.handle, N_RAGGED + 1, ROWS) == _lib.TDM_ERR_INVALID
    assert L.tdm_stream_submit(sd.handle, N_RAGGED, ROWS + 1) == _lib.TDM_ERR_INVALID
    sd.submit()
    sd.submit_array(batches[1])
    # acquiring a slot whose result was not collected
    p, seq = C.c_void_p(), C.c_int64()
    assert L.tdm_stream_acquire(sd.handle, C.byref(p), C.byref(seq)) == _lib.TDM_ERR_INVALID
    assert "uncollected" in _lib.last_error()
    # results come back in order, whether or not the first poll finds the oldest step finished
    first = sd.collect(wait=False) or sd.collect()
    assert first[0] == 0
    _equal(first, want[0], "after the refusals, batch 0", soft=False)
    second = sd.collect()
    assert second[0] == 1
    _equal(second, want[1], "after the refusals, batch 1", soft=False)
    got = _run(sd, batches[2:])
    for b, g in enumerate(got):
        _equal(g, want[2 + b], f"after the refusals, batch {2 + b}", soft=False)
    # destroy with steps in flight, then a fresh stream is exact
    sd.submit_array(batches[0])
    sd.submit_array(batches[1])
    sd.close()
    with pytest.raises(RuntimeError):
        sd.input_buffer()
    with StreamingDemodulator(FS, N_RAGGED, ROWS, "cu8", depth=3, freq_offsets=FOFFS) as sd2:
        got = _run(sd2, batches)
    for b, g in enumerate(got):
        _equal(g, want[b], f"fresh stream batch {b}", soft=False)


def test_stream_not_ready_is_reported_before_completion():
    """a step large enough to run for milliseconds: collect(wait=False) right after its submit says not ready; the wait then
    returns it"""
    from tetraear_amd.stream import StreamingDemodulator
    n, rows = 262144, 256
    with StreamingDemodulator(FS, n, rows, "cu8", depth=2) as sd:
        buf = sd.input_buffer()
        buf[:] = 128
        sd.submit()
        r = sd.collect(wait=False)
        if r is None:
            r = sd.collect()
        else:
            pytest.fail("a 256 x 262144 step finished before the call that submitted it returned")
        assert r[0] == 0 and len(r[1]) == rows


def test_h2d_ceiling_is_finite_and_positive():
    from tetraear_amd import _lib
    gbs = (C.c_double * 3)()
    _lib.check(_lib.load().tdm_link_ceiling(0, 256 << 20, 3, gbs))
    assert all(math.isfinite(g) and g > 0 for g in gbs), list(gbs)


# ---- iter_recording(overlapped=True) == the default path, read by read --------------------------------------------------

CHUNK, RPB, FOFF = 65536, 4, 1171.875


def _same(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, list):
            assert len(x) == len(y)
            for k, (p, q) in enumerate(zip(x, y)):
                np.testing.assert_array_equal(p, q, err_msg=f"read {i} carrier {k}")
        else:
            assert x.dtype == y.dtype == np.uint8
            np.testing.assert_array_equal(x, y, err_msg=f"read {i}")


@pytest.mark.parametrize("n", [2 * RPB * CHUNK, 6 * CHUNK, 4 * CHUNK + 1, 5 * CHUNK + 27, 3 * CHUNK + 28, 30011, 0])
@pytest.mark.parametrize("source", ["path", "fileobj", "array"])
def test_overlapped_recording_equals_the_default_path(tmp_path, n, source):
    from tetraear_amd import synth
    from tetraear_amd.ingest import demodulate_recording
    u8 = synth.noise_cu8(n, 7200 + n % 9973)
    path = tmp_path / "capture.cu8"
    u8.tofile(path)

    def src():
        return str(path) if source == "path" else (open(path, "rb") if source == "fileobj" else u8)
    s0, s1 = src(), src()
    base = demodulate_recording(s0, FS, chunk=CHUNK, freq_offset=FOFF, rows_per_batch=RPB)
    over = demodulate_recording(s1, FS, chunk=CHUNK, freq_offset=FOFF, rows_per_batch=RPB, overlapped=True)
    for s in (s0, s1):
        if hasattr(s, "close"):
            s.close()
    _same(over, base)
    assert len(base) == n // CHUNK + (1 if n % CHUNK else 0)


def test_overlapped_recording_many_carriers():
    from tetraear_amd import synth
    from tetraear_amd.ingest import iter_recording
    offs = [-312500.0, 62500.0, 287500.0]
    u8, _ = synth.multicarrier_cu8(5 * CHUNK + 4099, FS, offs, seed0=470)
    base = list(iter_recording(u8, FS, CHUNK, FOFF, rows_per_batch=RPB, pre_shifts=offs))
    over = list(iter_recording(u8, FS, CHUNK, FOFF, rows_per_batch=RPB, pre_shifts=offs, overlapped=True))
    assert all(len(o) == 3 for o in over)
    _same(over, base)


def test_overlapped_recording_consumer_stops_early_then_fresh_reader(tmp_path):
    from tetraear_amd import synth
    from tetraear_amd.ingest import demodulate_recording, iter_recording
    threads = threading.active_count()
    u8 = synth.noise_cu8(11 * CHUNK + 77, 7300)
    path = tmp_path / "first.cu8"
    u8.tofile(path)
    base = demodulate_recording(str(path), FS, CHUNK, FOFF, rows_per_batch=RPB)
    for first in iter_recording(str(path), FS, CHUNK, FOFF, rows_per_batch=RPB, overlapped=True):
        break
    gc.collect()
    np.testing.assert_array_equal(first, base[0])
    assert threading.active_count() == threads
    _same(list(iter_recording(str(path), FS, CHUNK, FOFF, rows_per_batch=RPB, overlapped=True)), base)
