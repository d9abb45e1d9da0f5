"""Tetra-mode channeliser (oversampled polyphase DFT filter bank) -- host face of tdm_channelise and tdm_channeliser.

`channelise` / `channelise_batch` start every call cold (samples before the call read as zero, output instants count from
its first sample).  `StreamingChanneliser` carries each stream's state from one push to the next, so that a capture read
chunk after chunk gives exactly what one call over the whole capture gives.
"""
import ctypes as C

import numpy as np

from tetraear_amd import _lib
from tetraear_amd._lib import FMT_BYTES, check, ptr

ACCEPTS = _lib.wire_codes("cu8", "cs8", "cf32", "cs16")


def channelise(iq, fmt, M, D, device=0):
    """One wideband stream -> complex64 [M][ceil(n/D)]; channel k is centred on k*fs/M."""
    f = ACCEPTS[fmt]
    iq = np.ascontiguousarray(iq)
    n_in = iq.nbytes // FMT_BYTES[f]
    n_out = (n_in + D - 1) // D
    out = np.zeros((M, n_out), dtype=np.complex64)
    no = C.c_int64()
    check(_lib.load().tdm_channelise(ptr(iq), f, n_in, M, D, ptr(out), C.byref(no), 0, device))
    assert no.value == n_out
    return out


def aligned_pitch(n_out):
    """Row pitch (complex samples) that keeps the kernel's 128-byte stores inside one cache line."""
    return (n_out + 15) // 16 * 16


def channelise_batch(iq, fmt, n_streams, M, D, device=0, pitch=0):
    """n_streams wideband streams back to back -> complex64 [n_streams][M][ceil(n/D)] in one launch
    (a view of a [n_streams][M][pitch] array when a row pitch is given)."""
    f = ACCEPTS[fmt]
    iq = np.ascontiguousarray(iq)
    n_in = iq.nbytes // FMT_BYTES[f] // n_streams
    n_out = (n_in + D - 1) // D
    out = np.zeros((n_streams, M, pitch or n_out), dtype=np.complex64)
    no = C.c_int64()
    check(_lib.load().tdm_channelise_batch(ptr(iq), f, n_in, n_streams, M, D, ptr(out), pitch, C.byref(no), 0, device))
    assert no.value == n_out
    return out[:, :, :n_out]


class StreamingChanneliser:
    """Stateful channeliser (include/tetrahip.h tdm_channeliser_*): `streams` wideband streams that advance together.

        with StreamingChanneliser(400, 125, "cu8", streams=32, max_n_in=1 << 20) as ch:
            for read in reads:                 # uint8 [streams][2 * n] (or flat, streams back to back)
                y = ch.push(read)              # complex64 [streams][M][n_out], n_out may be 0

    Concatenated along time, the pushes' outputs equal one channelise_batch over the concatenated input, bit for bit."""

    def __init__(self, M, D, fmt="cu8", streams=1, max_n_in=1 << 20, device=0):
        self.lib = _lib.load()
        self.handle = None
        self.M, self.D, self.streams, self.max_n_in = int(M), int(D), int(streams), int(max_n_in)
        self.fmt = ACCEPTS[fmt] if isinstance(fmt, str) else int(fmt)
        h = C.c_void_p()
        check(self.lib.tdm_channeliser_create(self.M, self.D, self.fmt, self.streams, self.max_n_in, int(device), C.byref(h)))
        self.handle = h

    @property
    def position(self):
        """(samples pushed, outputs emitted) per stream since create / reset"""
        si, so = C.c_int64(), C.c_int64()
        check(self.lib.tdm_channeliser_position(self._h(), C.byref(si), C.byref(so)))
        return si.value, so.value

    def _h(self):
        if self.handle is None:
            raise ValueError("StreamingChanneliser is closed")
        return self.handle

    def push(self, iq):
        """host samples of every stream, [streams][n] back to back in the wire format -> complex64 [streams][M][n_out]"""
        h = self._h()
        iq = np.ascontiguousarray(iq)
        n_in = iq.nbytes // FMT_BYTES[self.fmt] // self.streams
        if n_in * FMT_BYTES[self.fmt] * self.streams != iq.nbytes:
            raise ValueError(f"push: {iq.nbytes} bytes are not {self.streams} streams of whole samples")
        pos = self.position[0]
        n_exp = -(-(pos + n_in) // self.D) - (-(-pos // self.D))
        out = np.empty((self.streams, self.M, n_exp), dtype=np.complex64)
        no = C.c_int64()
        check(self.lib.tdm_channeliser_push(h, ptr(iq), n_in, ptr(out), 0, C.byref(no), 0))
        assert no.value == n_exp, (no.value, n_exp)
        return out

    def push_device(self, d_in, n_in, d_out, pitch):
        """device pointers: d_in [streams][n_in], d_out [streams][M][pitch] cf32 (pitch >= ceil(n_in / D)); enqueued on the
        current stream (tdm_set_stream).  Returns n_out."""
        no = C.c_int64()
        check(self.lib.tdm_channeliser_push(self._h(), d_in, int(n_in), d_out, int(pitch), C.byref(no), 1))
        return no.value

    def reset(self):
        """back to a fresh stream"""
        check(self.lib.tdm_channeliser_reset(self._h()))

    def close(self):
        if self.handle is not None:
            self.lib.tdm_channeliser_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass
