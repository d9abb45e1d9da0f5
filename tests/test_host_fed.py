"""GPU: the host-fed streaming paths -- what a capture loop runs -- held to the oracle read by read.

- tdm_process_pipelined (BatchDemodulator.process_stream): n_batches batches through two device slots and three streams.
  Every batch and every row carries distinct data and every carrier its own freq_offset, so input copied into the wrong
  slot, outputs read from the wrong slot or a missing wait shows up as a mismatch.  Reference-mode cu8 (and cf64) is pinned
  to the C oracle for every (batch, row); the other wire formats and the TETRA modes are the same kernels on the same plan,
  so every batch must equal tdm_process of that batch bit for bit.
- iter_recording / demodulate_recording at the lengths where a reader goes wrong: a recording that ends on a batch
  boundary, a short last batch with blank rows, last reads of 1, 27 and 28 samples (the reference answers the first two
  with an empty array), a recording shorter than one read, an empty one, and a consumer that stops early.
"""
import ctypes as C
import gc
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SOFT_TOL = 1e-10
FS = 2.4e6
N_RAGGED = 65536 + 13          # not a multiple of any block length
ROWS = 5
FOFFS = np.array([-2750.0, -1171.875, 0.0, 613.5, 2990.25])      # a distinct freq_offset per carrier


def _x_of(b, r, n=N_RAGGED, salt=0):
    """batch b, row r: distinct uniform cu8 noise"""
    from tetraear_amd import synth
    return synth.noise_cu8(n, 50000 + 1000 * salt + 100 * b + r)


def _oracle(x, foff):
    from oracle.oracle import OracleSignalProcessor
    o = OracleSignalProcessor(FS)
    return o.process(x, foff), o


def _check_oracle(x, foff, hard, soft, ns, bp, mm, what):
    """one carrier's outputs (full rows as the C-ABI writes them) against OracleSignalProcessor.process"""
    ref, o = _oracle(x, foff)
    ns = int(ns)
    assert ns == len(ref) + 1 and ns == len(o.symbols), (what, ns, len(ref))
    np.testing.assert_array_equal(hard[:ns - 1], ref, err_msg=what)
    scale = np.max(np.abs(o.symbols))
    assert np.max(np.abs(soft[:ns] - o.symbols)) <= SOFT_TOL * scale, what
    assert int(bp) == o.best_phase, what
    assert abs(float(mm) - o.min_margin) <= 1e-9, what


def _process_full(bd, iq, fo=None):
    """tdm_process of one batch, with the full [rows][max_soft] outputs (BatchDemodulator.process trims them)"""
    from tetraear_amd._lib import check, ptr
    rows, ms = bd.n_carriers, bd.info.max_soft
    iq = np.ascontiguousarray(iq)
    fo = None if fo is None else np.ascontiguousarray(fo, dtype=np.float64)
    hard = np.zeros((rows, ms), dtype=np.uint8)
    soft = np.zeros((rows, ms), dtype=bd.soft_dtype)
    n_soft = np.zeros(rows, dtype=np.int32)
    bp = np.zeros(rows, dtype=np.int32)
    mm = np.zeros(rows, dtype=np.float64)
    check(bd.lib.tdm_process(bd.handle, ptr(iq), bd.n_samples, None, ptr(fo), ptr(hard), ptr(soft), ptr(n_soft),
                             ptr(bp), ptr(mm)))
    return hard, soft, n_soft, bp, mm


def _equal_batch(got, b, want, what):
    """batch b of process_stream's outputs == one tdm_process call's, bit for bit (soft over its valid part)"""
    hard, soft, n_soft, bp, mm = got
    np.testing.assert_array_equal(n_soft[b], want[2], err_msg=what)
    np.testing.assert_array_equal(hard[b], want[0], err_msg=what)
    np.testing.assert_array_equal(bp[b], want[3], err_msg=what)
    np.testing.assert_array_equal(mm[b], want[4], err_msg=what)
    for r in range(len(want[2])):
        k = int(want[2][r])
        assert k > 0, (what, r)
        np.testing.assert_array_equal(soft[b, r, :k], want[1][r, :k], err_msg=f"{what} row {r}")


def _check_process_vs_oracle(bd, xs, foffs, what):
    """BatchDemodulator.process of one cu8 batch (rows xs) against the oracle, row by row"""
    from tetraear_amd import synth
    hards, softs, bp, mm = bd.process(np.concatenate(xs), freq_offsets=foffs)
    for r, u8 in enumerate(xs):
        ref, o = _oracle(synth.cu8_to_c128(u8), foffs[r])
        np.testing.assert_array_equal(hards[r], ref, err_msg=f"{what} row {r}")
        assert len(softs[r]) == len(o.symbols) and bp[r] == o.best_phase, (what, r)
        assert np.max(np.abs(softs[r] - o.symbols)) <= SOFT_TOL * np.max(np.abs(o.symbols)), (what, r)


# ---- tdm_process_pipelined -------------------------------------------------------------------------------------------

def test_process_stream_cu8_every_batch_and_row_vs_oracle():
    """reference mode, cu8, 5 rows of a ragged length: 1 batch (one slot), 2 (both), 3 (a slot reused), 9 (>= 8, odd)"""
    from tetraear_amd import synth
    from tetraear_amd.batch import BatchDemodulator
    xs = [[_x_of(b, r) for r in range(ROWS)] for b in range(9)]
    bd = BatchDemodulator(FS, N_RAGGED, ROWS, "cu8")
    for nb in (1, 2, 3, 9):
        iq = np.concatenate([u8 for b in range(nb) for u8 in xs[b]])
        hard, soft, n_soft, bp, mm = bd.process_stream(iq, nb, freq_offsets=FOFFS)
        assert hard.shape[:2] == (nb, ROWS) and n_soft.shape == (nb, ROWS)
        for b in range(nb):
            for r in range(ROWS):
                _check_oracle(synth.cu8_to_c128(xs[b][r]), FOFFS[r], hard[b, r], soft[b, r], n_soft[b, r], bp[b, r],
                              mm[b, r], f"n_batches {nb} batch {b} row {r}")
    bd.close()


@pytest.mark.parametrize("fmt", ["cs8", "cf32", "cf64"])
def test_process_stream_other_formats_equal_tdm_process(fmt):
    """cs8 / cf32 / cf64 plans: every batch of a 4-batch stream == tdm_process of that batch bit for bit; cf64 (the
    reference's own complex128 input) against the oracle as well"""
    from tetraear_amd import synth
    from tetraear_amd.batch import BatchDemodulator
    nb = 4
    batches = []
    for b in range(nb):
        rows = []
        for r in range(ROWS):
            u8 = _x_of(b, r, salt=1)
            if fmt == "cs8":
                rows.append(u8.view(np.int8))
            else:
                rows.append(synth.cu8_to_c128(u8).astype(np.complex64 if fmt == "cf32" else np.complex128))
        batches.append(np.concatenate(rows))
    bd = BatchDemodulator(FS, N_RAGGED, ROWS, fmt)
    got = bd.process_stream(np.concatenate(batches), nb, freq_offsets=FOFFS)
    for b in range(nb):
        _equal_batch(got, b, _process_full(bd, batches[b], FOFFS), f"{fmt} batch {b}")
        if fmt == "cf64":
            for r in range(ROWS):
                x = batches[b][r * N_RAGGED:(r + 1) * N_RAGGED]
                _check_oracle(x, FOFFS[r], got[0][b, r], got[1][b, r], got[2][b, r], got[3][b, r], got[4][b, r],
                              f"cf64 batch {b} row {r}")
    bd.close()


@pytest.mark.parametrize("mode_name", ["MODE_TETRA", "MODE_TETRA_GARDNER"])
def test_process_stream_tetra_modes_equal_tdm_process(mode_name):
    """TETRA-mode plans: cf32 soft output (the entry sizes that buffer from the plan's mode); 3 batches x 3 rows of
    distinct pi/4-DQPSK bursts, every batch == tdm_process of that batch bit for bit"""
    from tetraear_amd import _lib, synth
    from tetraear_amd.batch import BatchDemodulator
    fs, n, rows, nb = 72000.0, 16384, 3, 3
    batches = []
    for b in range(nb):
        xs = []
        for r in range(rows):
            x, _ = synth.dqpsk_baseband(n, fs, 700 + 10 * b + r, timing_offset=0.1 * r - 0.15 * b)
            rng = np.random.default_rng(900 + 10 * b + r)
            xs.append((x + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64))
        batches.append(np.concatenate(xs))
    bd = BatchDemodulator(fs, n, rows, "cf32", mode=getattr(_lib, mode_name))
    assert bd.soft_dtype == np.complex64
    got = bd.process_stream(np.concatenate(batches), nb)
    for b in range(nb):
        _equal_batch(got, b, _process_full(bd, batches[b]), f"{mode_name} batch {b}")
    bd.close()


def _raw_stream(bd, iq, nb, fo, with_bp_mm=True):
    """tdm_process_pipelined through raw ctypes, outputs the caller's own arrays"""
    from tetraear_amd._lib import ptr
    rows, ms = bd.n_carriers, bd.info.max_soft
    out = (np.zeros((nb, rows, ms), dtype=np.uint8), np.zeros((nb, rows, ms), dtype=bd.soft_dtype),
           np.zeros((nb, rows), dtype=np.int32), np.zeros((nb, rows), dtype=np.int32), np.zeros((nb, rows), dtype=np.float64))
    rc = bd.lib.tdm_process_pipelined(bd.handle, ptr(iq), C.c_int64(nb), ptr(fo), ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                      ptr(out[3]) if with_bp_mm else None, ptr(out[4]) if with_bp_mm else None)
    return rc, out


def test_process_stream_optional_outputs_and_pinned_caller_buffers():
    """best_phase / min_margin / freq_offset NULL: hard and soft as the full call's.  Input (and one output) already
    page-locked by the caller: the entry's own hipHostRegister fails, it runs its best-effort path -- results exact, the
    caller's registrations left in place (their tdm_host_unregister still succeeds), the buffers it pinned itself released
    (registering them again succeeds)."""
    from tetraear_amd._lib import check, ptr
    from tetraear_amd.batch import BatchDemodulator
    nb = 3
    iq = np.concatenate([_x_of(b, r, salt=2) for b in range(nb) for r in range(ROWS)])
    bd = BatchDemodulator(FS, N_RAGGED, ROWS, "cu8")
    full = bd.process_stream(iq, nb)                     # freq_offsets None through the Python face
    for b in range(nb):
        _equal_batch(full, b, _process_full(bd, iq.reshape(nb, -1)[b]), f"no offsets, batch {b}")
    rc, bare = _raw_stream(bd, iq, nb, None, with_bp_mm=False)
    check(rc)
    for b in range(nb):
        _equal_batch(bare[:3] + full[3:], b, [full[i][b] for i in range(5)], f"NULL best_phase / min_margin, batch {b}")
    assert not bare[3].any() and not bare[4].any()      # (NULL outputs: the caller's arrays untouched)
    # caller-pinned input and hard output
    fo = FOFFS.copy()
    want = bd.process_stream(iq, nb, freq_offsets=fo)
    lib = bd.lib
    check(lib.tdm_host_register(0, ptr(iq), iq.nbytes))
    try:
        rows, ms = bd.n_carriers, bd.info.max_soft
        hard = np.zeros((nb, rows, ms), dtype=np.uint8)
        check(lib.tdm_host_register(0, ptr(hard), hard.nbytes))
        soft, n_soft = np.zeros((nb, rows, ms), dtype=np.complex128), np.zeros((nb, rows), dtype=np.int32)
        bp, mm = np.zeros((nb, rows), dtype=np.int32), np.zeros((nb, rows), dtype=np.float64)
        check(lib.tdm_process_pipelined(bd.handle, ptr(iq), nb, ptr(fo), ptr(hard), ptr(soft), ptr(n_soft), ptr(bp), ptr(mm)))
        for b in range(nb):
            _equal_batch((hard, soft, n_soft, bp, mm), b, [w[b] for w in want], f"caller-pinned buffers, batch {b}")
        check(lib.tdm_host_unregister(0, ptr(hard)))    # still the caller's registration
        check(lib.tdm_host_register(0, ptr(soft), soft.nbytes))    # the entry's own pin is gone
        check(lib.tdm_host_unregister(0, ptr(soft)))
    finally:
        check(lib.tdm_host_unregister(0, ptr(iq)))
    # outputs of a plain raw call: the entry pinned and released all of them
    rc, out = _raw_stream(bd, iq, nb, fo)
    check(rc)
    for b in range(nb):
        _equal_batch(out, b, [w[b] for w in want], f"raw call, batch {b}")
    for a in out[:2]:
        check(lib.tdm_host_register(0, ptr(a), a.nbytes))
        check(lib.tdm_host_unregister(0, ptr(a)))
    # and the input the entry pinned for that call is free again
    check(lib.tdm_host_register(0, ptr(iq), iq.nbytes))
    check(lib.tdm_host_unregister(0, ptr(iq)))
    bd.close()


def test_process_stream_refusals_leave_the_plan_working_and_resize():
    """n_batches 0 -> TDM_ERR_INVALID, a short input -> ValueError, a rows_per_chunk > 1 plan -> TDM_ERR_UNSUPPORTED; after
    each refusal and after a successful call, tdm_process on the same plan still gives the oracle's output; after resize to
    another length process_stream does too"""
    from tetraear_amd import _lib, synth
    from tetraear_amd.batch import BatchDemodulator
    xs0 = [_x_of(0, r, salt=3) for r in range(ROWS)]
    bd = BatchDemodulator(FS, N_RAGGED, ROWS, "cu8")
    iq = np.concatenate(xs0 + [_x_of(1, r, salt=3) for r in range(ROWS)])
    with pytest.raises(_lib.TetraHipError) as e:
        bd.process_stream(iq, 0, freq_offsets=FOFFS)
    assert e.value.code == -1        # TDM_ERR_INVALID
    _check_process_vs_oracle(bd, xs0, FOFFS, "after n_batches 0")
    with pytest.raises(ValueError):
        bd.process_stream(iq[:-2], 2, freq_offsets=FOFFS)
    _check_process_vs_oracle(bd, xs0, FOFFS, "after a short input")
    bd.process_stream(iq, 2, freq_offsets=FOFFS)
    _check_process_vs_oracle(bd, xs0, FOFFS, "after a stream")
    # another length on the same plan
    n2 = 40000 + 7
    xs = [[_x_of(b, r, n=n2, salt=4) for r in range(ROWS)] for b in range(3)]
    bd.resize(n2)
    hard, soft, n_soft, bp, mm = bd.process_stream(np.concatenate([u8 for row in xs for u8 in row]), 3, freq_offsets=FOFFS)
    for b in range(3):
        for r in range(ROWS):
            _check_oracle(synth.cu8_to_c128(xs[b][r]), FOFFS[r], hard[b, r], soft[b, r], n_soft[b, r], bp[b, r], mm[b, r],
                          f"resized: batch {b} row {r}")
    bd.close()
    # a time-batched plan (rows_per_chunk 2: 4 rows out of 2 input rows, with pre-shifts) is refused
    offs = np.array([-312500.0, 62500.0, -37500.0, 287500.0])
    u8s = [_x_of(0, r, salt=5) for r in range(2)]
    tb = BatchDemodulator(FS, N_RAGGED, 4, "cu8").set_rows_per_chunk(2)
    with pytest.raises(_lib.TetraHipError) as e:
        tb.process_stream(np.concatenate(u8s * 4), 2)
    assert e.value.code == -5        # TDM_ERR_UNSUPPORTED
    foffs = FOFFS[:4]
    hards, softs, bps, _ = tb.process(np.concatenate(u8s), freq_offsets=foffs, pre_shifts=offs)
    from oracle.oracle import OracleSignalProcessor
    for row in range(4):
        o = OracleSignalProcessor(FS)
        ref = o.process(o.frequency_shift(synth.cu8_to_c128(u8s[row // 2]), offs[row]), foffs[row])
        np.testing.assert_array_equal(hards[row], ref, err_msg=f"rows_per_chunk plan, row {row}")
        assert bps[row] == o.best_phase and len(softs[row]) == len(o.symbols)
    tb.close()


# ---- iter_recording / demodulate_recording ---------------------------------------------------------------------------

CHUNK, RPB, FOFF = 65536, 4, 1171.875


def _reads_vs_oracle(outs, u8, chunk=CHUNK, foff=FOFF, pre_shifts=None):
    """every read of a recording (the last one shorter, possibly answered with an empty array) against the oracle"""
    from oracle.oracle import OracleSignalProcessor
    from tetraear_amd import synth
    n = len(u8) // 2
    n_full, tail = divmod(n, chunk)
    assert len(outs) == n_full + (1 if tail else 0), (n, len(outs))
    x = synth.cu8_to_c128(u8)
    for i, out in enumerate(outs):
        seg = x[i * chunk:min((i + 1) * chunk, n)]
        for k, f in enumerate([None] if pre_shifts is None else pre_shifts):
            o = OracleSignalProcessor(FS)
            ref = o.process(seg if f is None else o.frequency_shift(seg, f), foff)
            got = out if f is None else out[k]
            assert got.dtype == np.uint8 and len(got) == len(ref), (i, k, len(got), len(ref))
            np.testing.assert_array_equal(got, ref, err_msg=f"read {i} carrier {k}")


@pytest.mark.parametrize("n, source", [
    (2 * RPB * CHUNK, "file"),          # ends exactly on a batch boundary
    (6 * CHUNK, "array"),               # whole reads, not whole batches: the second batch has two blank rows
    (4 * CHUNK + 1, "file"),            # a 1-sample last read, alone in its batch
    (5 * CHUNK + 27, "array"),          # a 27-sample last read: the reference's empty answer
    (3 * CHUNK + 28, "file"),           # a 28-sample last read in the same batch as three whole reads
    (30011, "array"),                   # shorter than one read
    (0, "file"),                        # empty: nothing yielded
])
def test_recording_length_edges_every_read_vs_oracle(tmp_path, n, source):
    from tetraear_amd import synth
    from tetraear_amd.ingest import demodulate_recording
    u8 = synth.noise_cu8(n, 7000 + n % 9973)
    src = u8
    if source == "file":
        src = tmp_path / "capture.cu8"
        u8.tofile(src)
        src = str(src)
    outs = demodulate_recording(src, FS, chunk=CHUNK, freq_offset=FOFF, rows_per_batch=RPB)
    if n == 0:
        assert outs == []
    _reads_vs_oracle(outs, u8)


def test_recording_many_carriers_ragged_every_read_vs_oracle():
    """pre_shifts (three carriers, rows_per_chunk 3): a ragged recording -- one whole batch, a remainder batch of one read and
    a short last read -- every read and carrier against the oracle's process(frequency_shift(read, f_k), freq_offset)"""
    from tetraear_amd import synth
    from tetraear_amd.ingest import iter_recording
    offs = [-312500.0, 62500.0, 287500.0]
    u8, _ = synth.multicarrier_cu8(5 * CHUNK + 4099, FS, offs, seed0=450)
    outs = list(iter_recording(u8, FS, CHUNK, FOFF, rows_per_batch=RPB, pre_shifts=offs))
    assert all(len(o) == 3 for o in outs)
    _reads_vs_oracle(outs, u8, pre_shifts=offs)


def test_recording_consumer_stops_early_then_a_fresh_reader_is_exact(tmp_path):
    """`break` after the first read (the reader thread is in flight on the next batch): the generator's clean-up joins it and
    releases the plan and the page-locked buffers; a second recording through a fresh generator is then exact"""
    from oracle.oracle import OracleSignalProcessor
    from tetraear_amd import synth
    from tetraear_amd.ingest import iter_recording
    threads = threading.active_count()
    u8 = synth.noise_cu8(9 * CHUNK + 77, 7100)
    path = tmp_path / "first.cu8"
    u8.tofile(path)
    for first in iter_recording(str(path), FS, CHUNK, FOFF, rows_per_batch=RPB):
        break
    gc.collect()
    ref = OracleSignalProcessor(FS).process(synth.cu8_to_c128(u8[:2 * CHUNK]), FOFF)
    np.testing.assert_array_equal(first, ref)
    assert threading.active_count() == threads
    u8b = synth.noise_cu8(6 * CHUNK + 1234, 7101)
    _reads_vs_oracle(list(iter_recording(u8b, FS, CHUNK, FOFF, rows_per_batch=RPB)), u8b)


def test_a_failed_hip_call_is_reported_once():
    """A HIP call that fails (here: unregistering a buffer that was never registered) is reported by the call that made it
    and does not surface again as a 'kernel launch' failure of the next, unrelated process call on a plan"""
    from tetraear_amd import _lib
    from tetraear_amd._lib import ptr
    from tetraear_amd.batch import BatchDemodulator
    xs = [_x_of(0, r, salt=6) for r in range(ROWS)]
    bd = BatchDemodulator(FS, N_RAGGED, ROWS, "cu8")
    never = np.zeros(1 << 16, dtype=np.uint8)
    assert bd.lib.tdm_host_unregister(0, ptr(never)) == -3          # TDM_ERR_HIP
    assert "hipHostUnregister" in _lib.last_error()
    _check_process_vs_oracle(bd, xs, FOFFS, "after a failed HIP call")
    bd.process_stream(np.concatenate(xs), 1, freq_offsets=FOFFS)
    assert bd.lib.tdm_host_unregister(0, ptr(never)) == -3
    _check_process_vs_oracle(bd, xs, FOFFS, "after a failed HIP call and a stream")
    bd.close()
