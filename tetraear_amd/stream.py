"""Persistent, overlapped host-fed stream: the capture loop (include/tetrahip.h tdm_stream_*).

The reference reads a chunk, demodulates it and reads the next one (decrypt_capture.py:101-107, ui/modern.py:1908-1912).
`StreamingDemodulator` is that loop for batches of reads with everything made once: `depth` plans of one batch geometry and
a ring of `depth` slots, each with a library-owned page-locked input that the caller fills in place.  Step k runs on slot
k % depth; its host->device copy overlaps the kernels of the steps before it, its outputs come back behind its kernels.

    with StreamingDemodulator(2.4e6, chunk, rows, freq_offsets=f) as sd:
        for ...:
            buf = sd.input_buffer()            # the next slot's page-locked input (waits for nothing on the device)
            n = f.readinto(buf)                # filled in place
            sd.submit(n_inputs=...)            # H2D -> kernels -> D2H, queued; returns at once
            if sd.in_flight == sd.depth:
                seq, hards, softs, bp, mm = sd.collect()     # the oldest step, in order

Results are collected in submission order; a slot is handed out again only after its result was collected.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FMT_BYTES, FMT_CF32, FMT_CF64, FMT_CS8, FMT_CU8, MODE_REFERENCE, check

ACCEPTS = _lib.wire_codes("cu8", "cs8", "cf32", "cf64")   # (tdm_stream_create does not take cs16)


class StreamingDemodulator:
    """sample_rate, chunk (samples per input row), rows (plan rows per batch), fmt, mode: as BatchDemodulator.
    depth: slots = plans = steps that can be outstanding (3: four streams).  soft: copy the soft symbols back too.
    freq_offsets / pre_shifts: per plan row, or None (pre_shifts: reference mode).  rows_per_chunk = C: one input row feeds
    C consecutive plan rows (C carriers of one wideband read; rows must be a multiple of C)."""

    def __init__(self, sample_rate, chunk, rows, fmt="cu8", mode=MODE_REFERENCE, depth=3, soft=False, freq_offsets=None,
                 pre_shifts=None, rows_per_chunk=1, device=0):
        self.lib = _lib.load()
        self.handle = None
        self.fmt = ACCEPTS[fmt] if isinstance(fmt, str) else int(fmt)
        self.chunk, self.rows, self.depth, self.device = int(chunk), int(rows), int(depth), device
        self.rows_per_chunk = int(rows_per_chunk)
        self.in_rows = self.rows // max(self.rows_per_chunk, 1)
        self.mode, self.soft = mode, bool(soft)
        self.soft_dtype = np.complex128 if mode == MODE_REFERENCE else np.complex64
        fo = None if freq_offsets is None else np.ascontiguousarray(freq_offsets, dtype=np.float64)
        ps = None if pre_shifts is None else np.ascontiguousarray(pre_shifts, dtype=np.float64)
        for name, a in (("freq_offsets", fo), ("pre_shifts", ps)):
            if a is not None and a.shape != (self.rows,):
                raise ValueError(f"{name}: one entry per plan row ({self.rows}), got shape {a.shape}")
        h = C.c_void_p()
        check(self.lib.tdm_stream_create(float(sample_rate), self.chunk, self.rows, self.fmt, int(mode), self.depth,
                                         _lib.STREAM_SOFT if self.soft else 0, _lib.ptr(fo), _lib.ptr(ps),
                                         self.rows_per_chunk, int(device), C.byref(h)))
        self.handle = h
        self._acquired = None      # (seq, view) of the slot being filled
        self._views = []           # every view handed out (emptied on close)
        self.in_flight = 0

    # ---- the loop ----------------------------------------------------------------------------------------------------
    def _live(self):
        if not self.handle:
            raise RuntimeError("StreamingDemodulator is closed")

    def input_buffer(self):
        """numpy view of the next slot's page-locked input (acquired now; the same view until it is submitted): in_rows x
        chunk samples, flat -- bytes for cu8 / cs8 (two per sample), complex samples for cf32 / cf64.  Rows of a submit with
        n_samples < chunk lie n_samples apart.  Valid until the slot's step is submitted; never use it after close()."""
        self._live()
        if self._acquired is None:
            p, seq = C.c_void_p(), C.c_int64()
            check(self.lib.tdm_stream_acquire(self.handle, C.byref(p), C.byref(seq)))
            # the numpy view of an input slot: cu8 / cs8 as interleaved bytes, cf32 / cf64 as complex samples
            dt = np.dtype(_lib.FMT_VIEW_DTYPE[self.fmt])
            count = self.in_rows * self.chunk * FMT_BYTES[self.fmt] // dt.itemsize
            view = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(count * dt.itemsize,)).view(dt)
            self._views.append(view)
            self._acquired = (seq.value, view)
        return self._acquired[1]

    def submit(self, n_samples=None, n_inputs=None):
        """enqueue the acquired slot: n_inputs input rows (default all) of n_samples (default the chunk; shorter:
        reference mode only) back to back at the start of its input.  Returns the step's sequence number."""
        self._live()
        if self._acquired is None:
            raise RuntimeError("submit without an acquired input (call input_buffer() first)")
        n = self.chunk if n_samples is None else int(n_samples)
        k = self.in_rows if n_inputs is None else int(n_inputs)
        check(self.lib.tdm_stream_submit(self.handle, n, k))
        seq = self._acquired[0]
        self._acquired = None
        self.in_flight += 1
        return seq

    def submit_array(self, arr, n_samples=None):
        """copy `arr` (whole input rows of n_samples, default the chunk, in the stream's format) into the next slot and
        submit it"""
        n = self.chunk if n_samples is None else int(n_samples)
        src = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        row_bytes = n * FMT_BYTES[self.fmt]
        if src.nbytes % row_bytes or not 0 < src.nbytes <= self.in_rows * row_bytes:
            raise ValueError(f"{src.nbytes} bytes are not 1..{self.in_rows} rows of {row_bytes} bytes")
        buf = self.input_buffer().view(np.uint8)
        buf[:src.nbytes] = src
        return self.submit(n, src.nbytes // row_bytes)

    def collect(self, wait=True):
        """the oldest uncollected step: (seq, hards, softs or None, best_phase, min_margin), hards / softs one array per plan
        row trimmed to its symbols (rows without input: empty) and copied out of the slot; with wait=False None when that
        step has not finished yet"""
        self._live()
        r = _lib.StreamResult()
        rc = self.lib.tdm_stream_collect(self.handle, 1 if wait else 0, C.byref(r))
        if rc == _lib.TDM_NOT_READY:
            return None
        check(rc)
        self.in_flight -= 1
        rows, ms = r.n_rows, r.max_soft

        def arr(p, ctype, count, dtype):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(count,)).view(dtype).copy()
        n_soft = arr(r.n_soft, C.c_int32, rows, np.int32)
        hard = np.ctypeslib.as_array(C.cast(r.hard, C.POINTER(C.c_uint8)), shape=(rows, ms))
        hards = [hard[i, :max(int(n_soft[i]) - 1, 0)].copy() for i in range(rows)]
        softs = None
        if r.soft:
            soft = np.ctypeslib.as_array(C.cast(r.soft, C.POINTER(C.c_uint8)), shape=(rows, ms * r.soft_bytes)).view(self.soft_dtype)
            softs = [soft[i, :int(n_soft[i])].copy() for i in range(rows)]
        bp = arr(r.best_phase, C.c_int32, rows, np.int32)
        mm = arr(r.min_margin, C.c_double, rows, np.float64)
        return r.seq, hards, softs, bp, mm

    # ---- lifetime ----------------------------------------------------------------------------------------------------
    def close(self):
        """drain and free everything; the stream and every view it handed out are unusable afterwards"""
        if getattr(self, "handle", None):
            self._views.clear()
            self._acquired = None
            self.lib.tdm_stream_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
