"""GPU: the stateful channeliser (StreamingChanneliser / tdm_channeliser_*) held to one call over the whole stream.

The definition is oracle/pfb_np.py channelise of the concatenated stream (x[n] = 0 only before the STREAM's start).  Every
output of a push is computed from its own window and phase exactly as the one-shot kernel computes it, so the pushes,
concatenated along time, must equal one channelise_batch over the concatenated input bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FMTS = {"cu8": 2, "cs8": 2, "cf32": 8}
# (M, D): every built M; D = 27 and D = 40 leave M | TB*D unmet, D = 300 > 4M takes the direct kernel
GEOMS = [(72, 24), (80, 27), (96, 32), (128, 40), (400, 125), (72, 300)]


def _stream_bytes(fmt, n, streams, seed):
    """[streams][n] samples of a wideband signal plus noise, in wire format, as bytes"""
    from tetraear_amd import synth
    rng = np.random.default_rng(seed)
    out = []
    for s in range(streams):
        x = 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        x += 0.5 * np.exp(2j * np.pi * (0.013 + 0.07 * s) * np.arange(n))
        if fmt == "cf32":
            out.append(x.astype(np.complex64).view(np.uint8))
        elif fmt == "cu8":
            out.append(synth.quantise_cu8(x, scale=0.5))
        else:
            out.append(np.clip(np.rint(np.stack([x.real, x.imag], 1).ravel() * 64), -128, 127).astype(np.int8).view(np.uint8))
    return np.stack(out)           # [streams][n * bytes]


def _as_c128(raw, fmt):
    from tetraear_amd import synth
    if fmt == "cf32":
        return raw.view(np.complex64).astype(np.complex128)
    if fmt == "cu8":
        return synth.cu8_to_c128(raw)
    s = raw.view(np.int8).astype(np.float64) / 128.0
    return s[0::2] + 1j * s[1::2]


def _chunking(M, D, N, seed):
    """chunk lengths summing to N: 1, < D, < L-1, = L-1, not multiples of D or M, long ones, in a seeded order"""
    L = 3 * M
    special = [1, max(D - 1, 1), L - 2, L - 1, 7 * D + 3, 2 * M + 1, 1, 5000, 2 * L + 17, 3]
    rng = np.random.default_rng(seed)
    lens = list(special)
    while sum(lens) < N:
        lens.append(int(rng.choice([1, D + 1, L - 1, int(rng.integers(1, 4 * L))])))
    rng.shuffle(lens)
    out, tot = [], 0
    for n in lens:
        if tot + n > N:
            n = N - tot
        if n:
            out.append(n)
            tot += n
    return out


def _push_all(ch, raw, lens, fb):
    blocks, pos = [], 0
    for n in lens:
        y = ch.push(np.ascontiguousarray(raw[:, pos * fb:(pos + n) * fb]))
        assert y.shape[:2] == (raw.shape[0], ch.M)
        blocks.append(y)
        pos += n
    return np.concatenate(blocks, axis=2)


@pytest.mark.parametrize("M, D", GEOMS)
@pytest.mark.parametrize("streams", [1, 3])
def test_random_chunkings_equal_one_call(M, D, streams):
    from oracle import pfb_np
    from tetraear_amd.channeliser import StreamingChanneliser, channelise_batch
    N = 12 * 3 * M + 5 * D + 11
    for fi, (fmt, fb) in enumerate(FMTS.items()):
        raw = _stream_bytes(fmt, N, streams, seed=1000 * M + 10 * D + fi + streams)
        lens = _chunking(M, D, N, seed=M + D + fi + 7 * streams)
        one = channelise_batch(raw.reshape(-1), fmt, streams, M, D)
        with StreamingChanneliser(M, D, fmt, streams=streams, max_n_in=max(lens)) as ch:
            got = _push_all(ch, raw, lens, fb)
            assert ch.position == (N, -(-N // D))
        assert got.shape == one.shape == (streams, M, -(-N // D)), (fmt, got.shape)
        np.testing.assert_array_equal(got, one, err_msg=f"M={M} D={D} {fmt} streams={streams}")
        if fi == 0 or streams == 1:      # the definition, on probe channels of the last stream
            probe = [0, 1, M // 3, M - 1]
            ref = pfb_np.channelise(_as_c128(raw[-1], fmt), M, D, channels=probe)
            scale = np.max(np.abs(ref))
            for i, k in enumerate(probe):
                assert np.max(np.abs(got[-1, k] - ref[i])) < 2e-5 * scale, (M, D, fmt, k)


def test_direct_kernel_chunkings_equal_one_call():
    from tetraear_amd._lib import debug_option
    from tetraear_amd.channeliser import StreamingChanneliser, channelise_batch
    M, D = 400, 125
    N = 9 * 3 * M + 77
    for fmt, fb in FMTS.items():
        raw = _stream_bytes(fmt, N, 2, seed=42)
        lens = _chunking(M, D, N, seed=43)
        with debug_option("pfb_direct", 1):
            one = channelise_batch(raw.reshape(-1), fmt, 2, M, D)
            with StreamingChanneliser(M, D, fmt, streams=2, max_n_in=max(lens)) as ch:
                got = _push_all(ch, raw, lens, fb)
        np.testing.assert_array_equal(got, one, err_msg=fmt)


def test_config5_reads_equal_one_shot_and_stateless_reads_do_not():
    """32 cu8 streams of 10 MS/s (M = 400, D = 125), 4 Mi samples each, pushed as 1 Mi-sample reads on the device; the
    channel rows land in place in one [32][400][ceil(4 Mi / 125)] array (each push writes at the columns emitted so far)."""
    from tetraear_amd import _lib
    from tetraear_amd.batch import DeviceBuffer
    from tetraear_amd.channeliser import StreamingChanneliser, channelise
    M, D, S, R, NR = 400, 125, 32, 1 << 20, 4
    N = NR * R
    n_out = -(-N // D)
    lib = _lib.load()
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, size=(S, 2 * N), dtype=np.uint8)   # [S][N] of one stream each, read r = columns r*R..
    din = DeviceBuffer(0, u8.nbytes)
    d_one = DeviceBuffer(0, S * M * n_out * 8)
    d_push = DeviceBuffer(0, S * M * n_out * 8)
    d_read = DeviceBuffer(0, S * R * 2)
    try:
        din.upload(u8)
        no = C.c_int64()
        _lib.check(lib.tdm_channelise_batch(din.ptr, 0, N, S, M, D, d_one.ptr, 0, C.byref(no), 1, 0))
        assert no.value == n_out
        emitted = []
        with StreamingChanneliser(M, D, "cu8", streams=S, max_n_in=R) as ch:
            for r in range(NR):
                d_read.upload(np.ascontiguousarray(u8[:, 2 * r * R:2 * (r + 1) * R]))
                done = ch.position[1]
                k = ch.push_device(d_read.ptr, R, d_push.ptr.value + 8 * done, n_out)
                _lib.check(lib.tdm_dev_sync(0))   # (d_read is uploaded again for the next read)
                emitted.append(k)
            assert ch.position == (N, n_out)
        assert sum(emitted) == n_out and emitted == [-(-(r + 1) * R // D) - (-(-r * R // D)) for r in range(NR)]
        per = M * n_out                                    # (compared stream by stream: 107 MB each)
        one0 = None
        for y in range(S):
            one = np.empty((M, n_out), dtype=np.complex64)
            got = np.empty((M, n_out), dtype=np.complex64)
            _lib.check(lib.tdm_dev_download(0, _lib.ptr(one), d_one.ptr.value + 8 * y * per, one.nbytes))
            _lib.check(lib.tdm_dev_download(0, _lib.ptr(got), d_push.ptr.value + 8 * y * per, got.nbytes))
            np.testing.assert_array_equal(got, one, err_msg=f"stream {y}")
            if y == 0:
                one0 = one
        # what the object fixes: a stateless channelise per read differs from the one-shot near every seam
        for r in range(1, NR):
            first = -(-r * R // D)                          # the one-shot's first output at or after the seam
            cold = channelise(np.ascontiguousarray(u8[0, 2 * r * R:2 * (r + 1) * R]), "cu8", M, D)
            ref = one0[:, first:first + 8]
            assert not np.array_equal(cold[:, :8], ref), r
            assert np.max(np.abs(cold[:, :8] - ref)) > 1e-3 * np.max(np.abs(ref)), r
    finally:
        for b in (din, d_one, d_push, d_read):
            b.free()


def test_reset_starts_a_fresh_stream():
    from tetraear_amd.channeliser import StreamingChanneliser, channelise_batch
    M, D = 96, 32
    raw = _stream_bytes("cu8", 4000, 2, seed=9)
    with StreamingChanneliser(M, D, "cu8", streams=2, max_n_in=4000) as ch:
        ch.push(raw[:, :2 * 1234].copy())
        ch.reset()
        assert ch.position == (0, 0)
        got = _push_all(ch, raw, [700, 1, 2299, 1000], 2)
    np.testing.assert_array_equal(got, channelise_batch(raw.reshape(-1), "cu8", 2, M, D))
    assert ch.handle is None
    with pytest.raises(ValueError):
        ch.push(raw)


def test_device_pushes_alternating_between_two_plan_streams_and_host_pushes_interleaved():
    """device-pointer pushes enqueued on two plans' streams in turn (tdm_set_stream), with host-form pushes in between:
    the object orders its own pushes, so the history each one reads is the previous push's"""
    from tetraear_amd import _lib
    from tetraear_amd.batch import BatchDemodulator, DeviceBuffer
    from tetraear_amd.channeliser import StreamingChanneliser, channelise_batch
    M, D, S = 400, 125, 3
    N = 40000
    raw = _stream_bytes("cf32", N, S, seed=77)
    lens = _chunking(M, D, N, seed=78)
    one = channelise_batch(raw.reshape(-1), "cf32", S, M, D)
    lib = _lib.load()
    plans = [BatchDemodulator(72000.0, 4096, 1, "cf32", mode=_lib.MODE_TETRA) for _ in range(2)]
    bufs = []
    blocks, pos = [], 0
    try:
        with StreamingChanneliser(M, D, "cf32", streams=S, max_n_in=max(lens)) as ch:
            pend = []
            for i, n in enumerate(lens):
                part = np.ascontiguousarray(raw[:, 8 * pos:8 * (pos + n)])
                pos += n
                if i % 3 == 2:
                    blocks.append(ch.push(part))
                    continue
                din, dout = DeviceBuffer(0, part.nbytes), DeviceBuffer(0, S * M * (-(-n // D)) * 8 + 8)
                bufs += [din, dout]
                din.upload(part)
                plans[i % 2].make_stream_current()
                try:
                    k = ch.push_device(din.ptr, n, dout.ptr, -(-n // D))
                finally:
                    plans[i % 2].release_stream()
                pend.append((len(blocks), dout, k, -(-n // D)))
                blocks.append(None)
            _lib.check(lib.tdm_dev_sync(0))
            for j, dout, k, pitch in pend:
                for p in plans:
                    p.sync()
                blocks[j] = dout.download(np.complex64, S * M * pitch).reshape(S, M, pitch)[:, :, :k]
        np.testing.assert_array_equal(np.concatenate(blocks, axis=2), one)
    finally:
        for b in bufs:
            b.free()
        for p in plans:
            p.close()


def test_push_refusals_and_empty_push():
    from tetraear_amd import _lib
    from tetraear_amd.channeliser import StreamingChanneliser
    lib = _lib.load()
    with StreamingChanneliser(96, 32, "cu8", streams=1, max_n_in=1000) as ch:
        no = C.c_int64(5)
        buf = np.zeros(4000, dtype=np.uint8)
        out = np.zeros(96 * 40, dtype=np.complex64)
        assert lib.tdm_channeliser_push(ch.handle, _lib.ptr(buf), 0, _lib.ptr(out), 0, C.byref(no), 0) == 0 and no.value == 0
        assert lib.tdm_channeliser_push(ch.handle, _lib.ptr(buf), 1001, _lib.ptr(out), 0, C.byref(no), 0) == _lib.TDM_ERR_INVALID
        assert lib.tdm_channeliser_push(ch.handle, _lib.ptr(buf), 100, _lib.ptr(out), 3, C.byref(no), 0) == _lib.TDM_ERR_INVALID
        assert lib.tdm_channeliser_push(ch.handle, None, 100, _lib.ptr(out), 0, C.byref(no), 0) == _lib.TDM_ERR_INVALID
        assert ch.position == (0, 0)
        y = ch.push(np.full(2 * 31, 128, dtype=np.uint8))          # instant 0 is in: one output
        assert y.shape == (1, 96, 1)
        y = ch.push(np.full(2 * 1, 128, dtype=np.uint8))           # sample 31: no instant (the next is 32)
        assert y.shape == (1, 96, 0) and ch.position == (32, 1)
        y = ch.push(np.full(2 * 32, 128, dtype=np.uint8))          # samples 32..63: instant 32
        assert y.shape == (1, 96, 1) and ch.position == (64, 2)


def test_iter_channels_over_a_file_equals_one_call(tmp_path):
    from tetraear_amd.channeliser import channelise
    from tetraear_amd.ingest import iter_channels
    M, D = 400, 125
    N = 3 * 50000 + 4321
    raw = _stream_bytes("cu8", N, 1, seed=123)[0]
    path = tmp_path / "wide.cu8"
    raw.tofile(path)
    blocks = list(iter_channels(str(path), M, D, chunk=50000))        # 50000 mod 125 = 0 ... and the 4321 tail is not
    assert len(blocks) == 4
    blocks2 = list(iter_channels(raw, M, D, chunk=33333))             # 33333 mod 125 = 83, mod 400 = 133
    one = channelise(raw, "cu8", M, D)
    np.testing.assert_array_equal(np.concatenate(blocks, axis=2)[0], one)
    np.testing.assert_array_equal(np.concatenate(blocks2, axis=2)[0], one)


def test_carrier_across_a_seam_demodulates_in_one_piece():
    """a pi/4-DQPSK carrier straddles the seams of a channel row built read by read by iter_channels; demodulated in one
    piece by a TETRA-mode plan, the row gives back the transmitted dibits across the seams"""
    from tetraear_amd import synth
    from tetraear_amd._lib import MODE_TETRA
    from tetraear_amd.batch import BatchDemodulator
    from tetraear_amd.ingest import iter_channels
    from test_tetra_mode import best_ber
    M, D, fs, n = 96, 32, 2.4e6, 131072
    ks = [3, 47, 80]
    x, dibs = synth.grid_carriers(n, fs, ks, M)
    x32 = (x / 6).astype(np.complex64)
    chunk = 10000                                                     # 13 seams; 10000 mod 32 = 16, mod 96 = 16
    rows = np.concatenate(list(iter_channels(x32.view(np.uint8), M, D, chunk, fmt="cf32")), axis=2)[0]
    n_c = rows.shape[1]
    assert n_c == -(-n // D)
    bd = BatchDemodulator(fs / D, n_c, len(ks), "cf32", mode=MODE_TETRA)
    try:
        hards, _, _, _ = bd.process(np.ascontiguousarray(rows[ks]))
    finally:
        bd.close()
    sps = (fs / D) / synth.SYMBOL_RATE
    for i, k in enumerate(ks):
        ber, lag = best_ber(hards[i], dibs[k], edge=8)
        assert len(hards[i]) > 900 and ber == 0.0, (k, ber, lag)
        # a seam falls inside the symbols that were checked
        assert (chunk / D) / sps < len(hards[i]) - 8
