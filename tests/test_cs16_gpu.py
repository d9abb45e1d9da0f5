"""GPU: the cs16 wire format (interleaved little-endian int16 I, Q; value s / 32768) at every entry that takes a format.

The conversion is exact (fp32 and fp64) and happens where a kernel loads, so everything behind the loader sees the very
operands of the cf32 call (channeliser, TETRA modes) or the cf64 call (reference mode, spectrum gate) on the same values:
those comparisons are np.array_equal.  On top of them: the definitions (oracle/pfb_np.py, oracle/tetra_np.py) and the
oracle, with the project's bounds for the respective mode.  Shapes are the smallest at which the loaders' fast and slow
paths, the seams of a carried state and the row alignments (4-byte but not 8- or 16-byte) all occur."""
import ctypes as C

import numpy as np
import pytest

from tests import cs16_cases as cc

pytestmark = pytest.mark.gpu

SOFT_TOL = 1e-10          # reference mode (tests/test_wire_formats_gpu.py)
FOFFS = np.array([-2750.0, -1171.875, 0.0, 613.5, 2990.25])
CHAN_GEOMS = [(72, 24), (80, 27), (400, 125), (72, 300)]      # (72, 300): D > 4 M takes the direct kernel


# ---- channeliser ------------------------------------------------------------------------------------------------------

def _chan_len(M, D):
    return 12 * 3 * M + 5 * D + 11


@pytest.mark.parametrize("M, D", CHAN_GEOMS)
@pytest.mark.parametrize("streams", [1, 3])
def test_channeliser_one_shot_equals_cf32_call_and_definition(M, D, streams):
    from oracle import pfb_np
    from tetraear_amd.channeliser import channelise_batch
    N = _chan_len(M, D)
    s16 = cc.rows(N, streams, seed=2000 + M + D + streams)
    x64 = cc.c64(s16)
    n_out = -(-N // D)
    for pitch in (0, n_out | 1):                       # dense rows, and an odd output pitch
        got = channelise_batch(s16.reshape(-1), "cs16", streams, M, D, pitch=pitch)
        ref = channelise_batch(x64.reshape(-1), "cf32", streams, M, D, pitch=pitch)
        assert got.shape == (streams, M, n_out)
        np.testing.assert_array_equal(got, ref, err_msg=f"M={M} D={D} streams={streams} pitch={pitch}")
    probe = [0, 1, M // 3, M - 1]
    want = pfb_np.channelise(cc.c128(s16[-1]), M, D, channels=probe)
    scale = np.max(np.abs(want))
    for i, k in enumerate(probe):
        assert np.max(np.abs(got[-1, k] - want[i])) < 2e-5 * scale, (M, D, k)


def test_channeliser_stream_four_bytes_off_a_16_byte_boundary():
    """device pointers: the stream starts 4 bytes behind an allocation's (16-byte aligned) start, so no 4-sample unit of the
    fast path lies on a 16-byte boundary"""
    from tetraear_amd import _lib
    from tetraear_amd.batch import DeviceBuffer
    from tetraear_amd.channeliser import channelise_batch
    M, D, streams = 400, 125, 3
    N = _chan_len(M, D)
    n_out = -(-N // D)
    s16 = cc.rows(N, streams, seed=2100)
    lib = _lib.load()
    din, dout = DeviceBuffer(0, s16.nbytes + 16), DeviceBuffer(0, streams * M * n_out * 8)
    try:
        assert din.ptr.value % 16 == 0
        shifted = np.zeros(s16.size + 8, dtype=np.int16)
        shifted[2:2 + s16.size] = s16.reshape(-1)
        din.upload(shifted)
        no = C.c_int64()
        _lib.check(lib.tdm_channelise_batch(C.c_void_p(din.ptr.value + 4), _lib.FMT_CS16, N, streams, M, D, dout.ptr, 0,
                                            C.byref(no), 1, 0))
        _lib.check(lib.tdm_dev_sync(0))
        got = dout.download(np.complex64, streams * M * n_out).reshape(streams, M, n_out)
    finally:
        din.free()
        dout.free()
    np.testing.assert_array_equal(got, channelise_batch(cc.c64(s16).reshape(-1), "cf32", streams, M, D))


def _chunking(M, D, N, seed):
    from test_chan_stream_gpu import _chunking as chunking
    return chunking(M, D, N, seed)


def _push_all(ch, s16, lens):
    blocks, pos = [], 0
    for n in lens:
        y = ch.push(np.ascontiguousarray(s16[:, 2 * pos:2 * (pos + n)]))
        assert y.shape[:2] == (s16.shape[0], ch.M)
        blocks.append(y)
        pos += n
    return np.concatenate(blocks, axis=2)


@pytest.mark.parametrize("M, D", CHAN_GEOMS)
@pytest.mark.parametrize("streams", [1, 3])
def test_channeliser_carried_state_equals_one_shot(M, D, streams):
    from tetraear_amd.channeliser import StreamingChanneliser, channelise_batch
    N = _chan_len(M, D)
    s16 = cc.rows(N, streams, seed=2200 + M + D + streams)
    lens = _chunking(M, D, N, seed=M + D + 7 * streams)
    one = channelise_batch(s16.reshape(-1), "cs16", streams, M, D)
    with StreamingChanneliser(M, D, "cs16", streams=streams, max_n_in=max(lens)) as ch:
        got = _push_all(ch, s16, lens)
        assert ch.position == (N, -(-N // D))
        np.testing.assert_array_equal(got, one, err_msg=f"M={M} D={D} streams={streams}")
        ch.reset()
        assert ch.position == (0, 0)
        again = _push_all(ch, s16, [lens[-1]] + lens[:-1])
        assert ch.position == (N, -(-N // D))
    np.testing.assert_array_equal(again, one, err_msg="after reset")


def test_channeliser_carried_state_on_the_direct_kernel():
    from tetraear_amd._lib import debug_option
    from tetraear_amd.channeliser import StreamingChanneliser, channelise_batch
    M, D, streams = 400, 125, 2
    N = 9 * 3 * M + 77
    s16 = cc.rows(N, streams, seed=2300)
    lens = _chunking(M, D, N, seed=43)
    fft = channelise_batch(s16.reshape(-1), "cs16", streams, M, D)
    with debug_option("pfb_direct", 1):
        one = channelise_batch(s16.reshape(-1), "cs16", streams, M, D)
        ref = channelise_batch(cc.c64(s16).reshape(-1), "cf32", streams, M, D)
        with StreamingChanneliser(M, D, "cs16", streams=streams, max_n_in=max(lens)) as ch:
            got = _push_all(ch, s16, lens)
    np.testing.assert_array_equal(got, one)
    np.testing.assert_array_equal(one, ref)
    assert np.max(np.abs(one - fft)) < 2e-5 * np.max(np.abs(fft))


def test_iter_channels_over_a_cs16_file_equals_one_call(tmp_path):
    from tetraear_amd.channeliser import channelise
    from tetraear_amd.ingest import iter_channels
    M, D = 400, 125
    N = 3 * 20000 + 4321
    s16 = cc.row(0, N, seed=2400)
    path = tmp_path / "wide.cs16"
    s16.tofile(path)
    blocks = list(iter_channels(str(path), M, D, chunk=20000, fmt="cs16"))
    assert len(blocks) == 4
    blocks2 = list(iter_channels(s16.view(np.uint8), M, D, chunk=13333, fmt="cs16"))
    one = channelise(s16, "cs16", M, D)
    np.testing.assert_array_equal(np.concatenate(blocks, axis=2)[0], one)
    np.testing.assert_array_equal(np.concatenate(blocks2, axis=2)[0], one)


# ---- reference mode ---------------------------------------------------------------------------------------------------

def _check_oracle(fs, x, foff, hard, soft, bp, what):
    from oracle.oracle import OracleSignalProcessor
    o = OracleSignalProcessor(fs)
    ref = o.process(x, foff)
    np.testing.assert_array_equal(hard, ref, err_msg=what)
    assert len(soft) == len(o.symbols) and len(soft) > 100, what
    assert int(bp) == o.best_phase, what
    assert np.max(np.abs(soft - o.symbols)) <= SOFT_TOL * np.max(np.abs(o.symbols)), what


@pytest.mark.parametrize("fs", [2.4e6, 5.52e6])
@pytest.mark.parametrize("n", [40001, 65536 + 13])
def test_reference_mode_rows_vs_oracle_and_equal_to_cf64_plan(fs, n):
    from tetraear_amd.batch import BatchDemodulator
    rows = 5
    s16 = cc.rows(n, rows, seed=2500 + n % 13)
    xs = cc.c128(s16)
    bd = BatchDemodulator(fs, n, rows, "cs16")
    assert bd.info.in_fmt == 4 and bd.info.dec_engine in (1, 2)
    hards, softs, bp, mm = bd.process(s16.reshape(-1), freq_offsets=FOFFS)
    bd.close()
    bf = BatchDemodulator(fs, n, rows, "cf64")
    hf, sf, bpf, mmf = bf.process(xs.reshape(-1), freq_offsets=FOFFS)
    bf.close()
    for r in range(rows):
        what = f"cs16 fs {fs} n {n} row {r}"
        _check_oracle(fs, xs[r], FOFFS[r], hards[r], softs[r], bp[r], what)
        assert np.array_equal(hards[r], hf[r]) and np.array_equal(softs[r], sf[r]), what
    assert np.array_equal(bp, bpf) and np.array_equal(mm, mmf)


@pytest.mark.parametrize("fs", [2.4e6, 5.52e6])
def test_reference_mode_shared_input_with_pre_shifts(fs):
    from oracle.oracle import OracleSignalProcessor
    from tetraear_amd.batch import BatchDemodulator
    n = 50001
    s16 = cc.row(0, n, seed=2550)
    x = cc.c128(s16)
    shifts = np.array([-600000.0, -25000.0, 0.0, 37500.0, 412500.0])
    bd = BatchDemodulator(fs, n, len(shifts), "cs16")
    hards, softs, bp, mm = bd.process(s16, freq_offsets=FOFFS, pre_shifts=shifts, shared_input=True)
    bd.close()
    bf = BatchDemodulator(fs, n, len(shifts), "cf64")
    hf, sf, bpf, mmf = bf.process(x, freq_offsets=FOFFS, pre_shifts=shifts, shared_input=True)
    bf.close()
    o = OracleSignalProcessor(fs)
    for r in range(len(shifts)):
        what = f"cs16 shared fs {fs} row {r}"
        _check_oracle(fs, o.frequency_shift(x, shifts[r]), FOFFS[r], hards[r], softs[r], bp[r], what)
        assert np.array_equal(hards[r], hf[r]) and np.array_equal(softs[r], sf[r]), what


def test_signal_processor_process_cs16_equals_process():
    from tetraear_amd.signal import SignalProcessor
    n, fs = 40001, 2.4e6
    s16 = cc.row(1, n, seed=2600)
    p = SignalProcessor(fs)
    hard = p.process_cs16(s16, 1171.875)
    soft, bp, mm = p.symbols.copy(), p.best_phase, p.min_margin
    ref = p.process(cc.c128(s16), 1171.875)
    assert len(hard) > 100
    assert np.array_equal(hard, ref) and np.array_equal(soft, p.symbols) and bp == p.best_phase and mm == p.min_margin
    assert len(p.process_cs16(np.zeros(0, np.int16))) == 0 and len(p.symbols) == 0


def test_spectrum_gate_cs16_equals_cf64():
    from tetraear_amd.gate import spectrum_gate
    n, rows = 16384, 4
    s16 = cc.rows(n, rows, seed=2800)
    res, afc = spectrum_gate(s16.reshape(-1), "cs16", n, rows)
    ref, ref_afc = spectrum_gate(cc.c128(s16).reshape(-1), "cf64", n, rows)
    assert res == ref and np.array_equal(afc, ref_afc)
    assert len({d["signal_power"] for d in res}) == rows


# ---- TETRA modes ------------------------------------------------------------------------------------------------------

def _tetra_rows(fs, n, seed, toff, coff, snr, rows, scale=0.5):
    from test_tetra_mode import make_signal
    sig = [make_signal(n, fs, seed * 10 + r, toff + 0.05 * r, coff, snr) for r in range(rows)]
    s16 = np.stack([cc.quantise(s[0].astype(np.complex128), scale) for s in sig])
    return s16, [s[1] for s in sig]


def test_tetra_mode_cs16_matches_definition_and_equals_cf32_plan():
    from oracle import tetra_np
    from test_tetra_mode import CASES, best_ber
    from tetraear_amd._lib import MODE_TETRA
    from tetraear_amd.batch import BatchDemodulator
    for fs, n, seed, toff, coff, snr in CASES[:5]:
        rows = 3
        s16, dibs = _tetra_rows(fs, n, seed, toff, coff, snr, rows)
        x64 = cc.c64(s16)
        bd = BatchDemodulator(fs, n, rows, "cs16", mode=MODE_TETRA)
        hards, softs, timing, margin = bd.process(s16.reshape(-1))
        y16 = bd.rrc_filter(s16)
        bd.close()
        bf = BatchDemodulator(fs, n, rows, "cf32", mode=MODE_TETRA)
        hf, sf, tf, mf = bf.process(x64.reshape(-1))
        yf = bf.rrc_filter(x64)
        bf.close()
        assert np.array_equal(y16, yf), fs
        assert np.array_equal(timing, tf) and np.array_equal(margin, mf), fs
        for r in range(rows):
            xq = cc.c128(s16[r])
            ref_hard, _, info = tetra_np.demod(xq, fs)
            assert len(softs[r]) == info["n_sym"], (fs, r)
            np.testing.assert_array_equal(hards[r], ref_hard)
            scale = np.max(np.abs(info["sym"]))
            assert np.max(np.abs(softs[r] - info["sym"])) < 1e-5 * scale, (fs, r)
            assert best_ber(hards[r], dibs[r])[0] <= (0.0 if snr >= 20.0 else 3e-3)
            assert abs(timing[r] / 1000.0 - info["tau"][len(info["tau"]) // 2]) < 2e-3
            assert abs(margin[r] - info["margin"]) < 1e-3
            # the cf32 plan on the same values, bit for bit: hard, soft, n_soft
            assert len(softs[r]) == len(sf[r]) and np.array_equal(softs[r], sf[r]), (fs, r)
            assert np.array_equal(hards[r], hf[r]), (fs, r)
            ref_y = tetra_np.matched_filter(xq, tetra_np.rrc_taps(fs / 18000.0))
            assert np.max(np.abs(y16[r] - ref_y)) < 2e-6 * np.max(np.abs(ref_y)), (fs, r)


def test_tetra_mode_cs16_rows_that_are_not_8_byte_aligned():
    """through the C-ABI: n = 8191 at a pitch of 8193 samples, so every other row starts 4 bytes off an 8-byte boundary"""
    from oracle import tetra_np
    from tetraear_amd._lib import MODE_TETRA, check, ptr
    from tetraear_amd.batch import BatchDemodulator
    fs, n, rows, pitch = 72000.0, 8191, 3, 8193
    s16, _ = _tetra_rows(fs, n, 90, 0.1, 25.0, 22.0, rows)
    buf = np.full((rows, 2 * pitch), 0x7777, dtype=np.int16)
    buf[:, :2 * n] = s16
    bd = BatchDemodulator(fs, n, rows, "cs16", mode=MODE_TETRA)
    ms = bd.info.max_soft
    hard = np.zeros((rows, ms), np.uint8); soft = np.zeros((rows, ms), np.complex64)
    ns = np.zeros(rows, np.int32); tm = np.zeros(rows, np.int32); mm = np.zeros(rows)
    check(bd.lib.tdm_process(bd.handle, ptr(buf), pitch, None, None, ptr(hard), ptr(soft), ptr(ns), ptr(tm), ptr(mm)))
    h0, s0, t0, m0 = bd.process(s16.reshape(-1))
    bd.close()
    bf = BatchDemodulator(fs, n, rows, "cf32", mode=MODE_TETRA)
    hf, sf, tf, mf = bf.process(cc.c64(s16).reshape(-1))
    bf.close()
    for r in range(rows):
        ref_hard, _, info = tetra_np.demod(cc.c128(s16[r]), fs)
        assert ns[r] == info["n_sym"]
        np.testing.assert_array_equal(hard[r, :ns[r] - 1], ref_hard)
        for other_h, other_s in ((h0, s0), (hf, sf)):
            assert np.array_equal(hard[r, :ns[r] - 1], other_h[r]) and np.array_equal(soft[r, :ns[r]], other_s[r]), r
    assert np.array_equal(tm, tf) and np.array_equal(mm, mf)


@pytest.mark.parametrize("fs", [72000.0, 144000.0])
def test_gardner_mode_cs16_equals_cf32_three_launches(fs):
    from tetraear_amd._lib import MODE_TETRA_GARDNER, debug_option
    from tetraear_amd.batch import BatchDemodulator
    n, rows = 12000, 4
    s16, dibs = _tetra_rows(fs, n, 95, -0.1, 30.0, 22.0, rows)
    bd = BatchDemodulator(fs, n, rows, "cs16", mode=MODE_TETRA_GARDNER)
    k16 = int(bd.info.gardner_segments)
    hards, softs, timing, margin = bd.process(s16.reshape(-1))
    bd.close()
    with debug_option("gardner_fused", 0):
        bf = BatchDemodulator(fs, n, rows, "cf32", mode=MODE_TETRA_GARDNER)
        kf = int(bf.info.gardner_segments)
        hf, sf, tf, mf = bf.process(cc.c64(s16).reshape(-1))
        bf.close()
    assert k16 == kf == 1
    for r in range(rows):
        assert len(softs[r]) == len(sf[r]) > 0.9 * n / (fs / 18000.0) - 20
        assert np.array_equal(softs[r], sf[r]) and np.array_equal(hards[r], hf[r]), (fs, r)
        m = len(hards[r])
        errs = min(int(np.sum(hards[r][700:m - 8] != dibs[r][lag + 700:lag + m - 8])) for lag in range(40) if len(dibs[r]) - lag >= m)
        assert errs == 0, (fs, r, errs)
    assert np.array_equal(timing, tf) and np.array_equal(margin, mf)


@pytest.mark.parametrize("gated", [False, True])
def test_wideband_receiver_cs16_equals_cf32(gated):
    from test_tetra_mode import _wideband, best_ber
    from tetraear_amd.wideband import WidebandReceiver
    M, D, fs, n = 96, 32, 2.4e6, 65536
    ks = [[0, 5, 47, 90], [3, 49, 95]]
    s16, dibs = [], []
    for si, kk in enumerate(ks):
        x, d = _wideband(n, fs, kk, M, seed0=500 + 20 * si)
        q = np.empty(2 * n, dtype=np.int16)
        q[0::2] = np.rint(32768 * x.real / 6)
        q[1::2] = np.rint(32768 * x.imag / 6)
        s16.append(q)
        dibs.append(d)
    s16 = np.stack(s16)
    both = []
    for fmt, data in (("cs16", s16), ("cf32", cc.c64(s16))):
        rx = WidebandReceiver(fs, n, M, D, streams=2, fmt=fmt, gated=gated)
        rx.d_in.upload(data)
        rx.enqueue()
        rx.sync()
        both.append(rx.demod.download())
        rx.close()
    (hard, soft, n_soft, timing, margin), (hf, sf, nf, tf, mf) = both
    assert np.array_equal(n_soft, nf), gated
    for r in range(2 * M):                      # (a row's buffers past its symbols are never written)
        k = int(n_soft[r])
        assert np.array_equal(hard[r, :max(k - 1, 0)], hf[r, :max(k - 1, 0)]) and np.array_equal(soft[r, :k], sf[r, :k]), (gated, r)
        if k:                                   # (a gated receiver leaves the other outputs of an unlisted row alone)
            assert timing[r] == tf[r] and margin[r] == mf[r], (gated, r)
    assert not gated or np.any(n_soft == 0)
    for si, kk in enumerate(ks):
        for k in kk:
            r = si * M + k
            ber, lag = best_ber(hard[r, :n_soft[r] - 1], dibs[si][k], edge=8)
            assert n_soft[r] > 400 and ber == 0.0, (si, k, ber, lag)


# ---- refusals ---------------------------------------------------------------------------------------------------------

def test_format_5_is_still_invalid_and_partial_cs16_pushes_are_refused():
    from tetraear_amd import _lib
    from tetraear_amd.channeliser import StreamingChanneliser
    lib = _lib.load()
    h = C.c_void_p()
    buf = np.zeros(4096, dtype=np.int16)
    out = np.zeros(96 * 64 * 8, dtype=np.complex64)
    no = C.c_int64()
    for mode in (_lib.MODE_REFERENCE, _lib.MODE_TETRA, _lib.MODE_TETRA_GARDNER):
        assert lib.tdm_plan_create(72000.0, 4096, 1, 5, mode, 0, C.byref(h)) == _lib.TDM_ERR_INVALID
    for fmt in (4, 5):      # (the host-fed stream does not take cs16: include/tetrahip.h tdm_stream_create)
        assert lib.tdm_stream_create(2.4e6, 4096, 1, fmt, _lib.MODE_REFERENCE, 2, 0, None, None, 1, 0, C.byref(h)) == _lib.TDM_ERR_INVALID
    assert lib.tdm_spectrum_gate(_lib.ptr(buf), 5, 1024, 1024, 1, 2.4e6, _lib.ptr(np.zeros(8)), _lib.ptr(np.zeros(1)), 0, 0) == _lib.TDM_ERR_INVALID
    assert lib.tdm_channelise_batch(_lib.ptr(buf), 5, 512, 1, 96, 32, _lib.ptr(out), 0, C.byref(no), 0, 0) == _lib.TDM_ERR_INVALID
    assert lib.tdm_channelise(_lib.ptr(buf), 5, 512, 96, 32, _lib.ptr(out), C.byref(no), 0, 0) == _lib.TDM_ERR_INVALID
    assert lib.tdm_channeliser_create(96, 32, 5, 1, 1000, 0, C.byref(h)) == _lib.TDM_ERR_INVALID
    assert lib.tdm_channeliser_create(96, 32, 3, 1, 1000, 0, C.byref(h)) == _lib.TDM_ERR_INVALID     # (cf64: never a channeliser format)
    with StreamingChanneliser(96, 32, "cs16", streams=3, max_n_in=1000) as ch:
        for nbytes in (4 * 3 * 100 + 4, 4 * 3 * 100 + 6, 4 * 3 * 100 - 2):
            with pytest.raises(ValueError):
                ch.push(np.zeros(nbytes, dtype=np.uint8))
        assert ch.position == (0, 0)
        assert ch.push(np.zeros(4 * 3 * 100, dtype=np.uint8)).shape == (3, 96, 4)
