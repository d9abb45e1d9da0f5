"""`SignalProcessor` with the reference's interface, computed on an MI355X.

Mirrors `tetraear/signal/processor.py:18-273` (syrex1013/TetraEar v2.2): same constructor,
attributes, method names, argument meaning, return types and "log and carry on" error behaviour,
so `tetraear.ui.modern.CaptureThread`, the capture scripts and `TetraSignalDetector` can use it
unchanged.  Every method is one call into libtetrahip.so (hand-written HIP kernels); nothing is
computed in numpy here beyond dtype plumbing, and a missing library / GPU raises.
"""
import ctypes as C
import logging
import threading
from collections import OrderedDict

import numpy as np

from tetraear_amd import _lib
from tetraear_amd._lib import FMT_CF32, FMT_CF64, FMT_CS16, FMT_CU8, check, ptr
from tetraear_amd.batch import BatchDemodulator

logger = logging.getLogger(__name__)

# One plan per (device, sample rate, wire format), shared by every SignalProcessor of the process: the reference's
# callers make a new SignalProcessor per call (signal/scanner.py:164) and read whatever length they like
# (scanner.py:347, rtl_auto_capture.py:182), so neither the instance nor the length may key the expensive state.
# A plan serves any chunk length (tdm_plan_resize keeps the per-length tables of the lengths it has seen).
_PLAN_CACHE_SIZE = 8
_PLANS = OrderedDict()
_PLANS_LOCK = threading.Lock()


def _shared_plan(device, sample_rate, n, fmt):
    key = (int(device), float(sample_rate), fmt)
    with _PLANS_LOCK:
        p = _PLANS.get(key)
        if p is None:
            p = BatchDemodulator(sample_rate, n, 1, fmt, device)
            p.lock = threading.Lock()
            _PLANS[key] = p
            while len(_PLANS) > _PLAN_CACHE_SIZE:
                _, old = _PLANS.popitem(last=False)
                with old.lock:
                    old.close()
        else:
            _PLANS.move_to_end(key)
    return p


def close_plans():
    """Release every cached plan (device memory, streams)."""
    with _PLANS_LOCK:
        while _PLANS:
            _, old = _PLANS.popitem()
            with old.lock:
                old.close()


def _as_c128(samples):
    a = np.asarray(samples)
    return np.ascontiguousarray(a, dtype=np.complex128), np.iscomplexobj(a)


class SignalProcessor:
    """Processes raw IQ samples for TETRA demodulation (GPU implementation)."""

    def __init__(self, sample_rate=2.4e6, device=0):
        # processor.py:21-33
        self.sample_rate = sample_rate
        self.symbol_rate = 18000
        self.samples_per_symbol = int(sample_rate / self.symbol_rate)
        self.symbols = None
        # extras (not in the reference): diagnostics of the last process() call
        self.best_phase = None
        self.min_margin = None
        self.device = device

    # ------------------------------------------------------------------ processor.py:35-49
    def resample(self, samples, target_rate):
        x, _ = _as_c128(samples)
        num = int(len(x) * target_rate / self.sample_rate)
        y = np.empty(num, dtype=np.complex128)
        check(_lib.load().tdm_resample(ptr(x), len(x), num, ptr(y), self.device))
        return y

    # ------------------------------------------------------------------ processor.py:51-83
    def filter_signal(self, samples, bandwidth=25000, sample_rate=None):
        if len(samples) == 0:
            return samples
        fs = sample_rate if sample_rate is not None else self.sample_rate
        x, was_complex = _as_c128(samples)
        y = np.empty_like(x)
        applied = C.c_int32()
        check(_lib.load().tdm_filter_signal(ptr(x), len(x), float(bandwidth), float(fs), ptr(y),
                                            C.byref(applied), self.device))
        if not applied.value:
            # the reference catches filtfilt's ValueError and returns its input (processor.py:81-83)
            logger.warning("Filter design failed, using unfiltered samples: The length of the input "
                           "vector x must be greater than padlen, which is 15.")
            return samples
        return y if was_complex else y.real.copy()

    # ------------------------------------------------------------------ processor.py:85-100
    def frequency_shift(self, samples, freq_offset, sample_rate=None):
        fs = sample_rate if sample_rate is not None else self.sample_rate
        x, _ = _as_c128(samples)
        y = np.empty_like(x)
        check(_lib.load().tdm_frequency_shift(ptr(x), len(x), float(freq_offset), float(fs), ptr(y), self.device))
        return y

    # ------------------------------------------------------------------ processor.py:102-166
    def demodulate_dqpsk(self, samples):
        if len(samples) < 2:
            return np.array([], dtype=np.uint8)
        x, _ = _as_c128(samples)
        out = np.empty(len(x) - 1, dtype=np.uint8)
        n_out = C.c_int64()
        mm = C.c_double()
        check(_lib.load().tdm_demodulate_dqpsk(ptr(x), len(x), ptr(out), C.byref(n_out), C.byref(mm), self.device))
        self.min_margin = mm.value
        return out[:n_out.value]

    # ------------------------------------------------------------------ processor.py:168-219
    def extract_symbols(self, samples, sample_rate=None):
        if len(samples) == 0:
            return np.array([], dtype=complex)
        fs = sample_rate if sample_rate is not None else self.sample_rate
        if int(fs / self.symbol_rate) <= 1:
            return samples  # processor.py:216-217
        x, was_complex = _as_c128(samples)
        y = np.empty_like(x)
        n_out = C.c_int64()
        bp = C.c_int32()
        check(_lib.load().tdm_extract_symbols(ptr(x), len(x), float(fs), float(self.symbol_rate), ptr(y),
                                              C.byref(n_out), C.byref(bp), self.device))
        self.best_phase = bp.value
        y = y[:n_out.value]
        return y if was_complex else y.real.copy()

    # ------------------------------------------------------------------ processor.py:221-273
    def process(self, samples, freq_offset=0):
        if len(samples) == 0:
            self.symbols = np.array([], dtype=complex)
            return np.array([], dtype=np.uint8)
        # Input dtypes (the reference follows its input's dtype through scipy.signal.decimate, processor.py:254, which casts
        # the SOS to x.dtype): complex128 -- what pyrtlsdr hands over -- is the reference's own arithmetic, term for term.
        # complex64 / float32 input the reference decimates in SINGLE precision (everything behind the decimator is double
        # again); here every dtype is computed in fp64: the result is the reference's result for the same samples handed
        # over as complex128, which its own single-precision pass approximates to 1e-5 (hard decisions equal on the
        # goldens of tests/golden/dtypes.npz, soft within 5e-5).  A REAL array stays real in the reference when
        # freq_offset == 0: `symbols` is then a float64 array here too.
        a = np.asarray(samples)
        if a.dtype == np.complex64:
            fmt, x = FMT_CF32, np.ascontiguousarray(a)
        else:
            fmt, x = FMT_CF64, np.ascontiguousarray(a, dtype=np.complex128)
        hard = self._run(x, fmt, len(x), freq_offset)
        if not np.iscomplexobj(a) and freq_offset == 0:
            self.symbols = np.ascontiguousarray(self.symbols.real)
        return hard

    def process_cu8(self, iq_bytes, freq_offset=0):
        """process() fed with raw RTL-SDR bytes (interleaved uint8 I,Q) instead of the complex128
        array pyrtlsdr would have made from them; identical results, 8x less host->device traffic."""
        u8 = np.ascontiguousarray(iq_bytes, dtype=np.uint8)
        n = len(u8) // 2
        if n == 0:
            self.symbols = np.array([], dtype=complex)
            return np.array([], dtype=np.uint8)
        return self._run(u8, FMT_CU8, n, freq_offset)

    def process_cs16(self, iq_int16, freq_offset=0):
        """process() fed with the interleaved int16 I,Q of a 16-bit radio (sc16 / CS16) instead of the complex128 array
        s / 32768 made from them; identical results, 4x less host->device traffic."""
        s16 = np.ascontiguousarray(iq_int16, dtype=np.int16)
        n = len(s16) // 2
        if n == 0:
            self.symbols = np.array([], dtype=complex)
            return np.array([], dtype=np.uint8)
        return self._run(s16, FMT_CS16, n, freq_offset)

    def _run(self, x, fmt, n, freq_offset):
        plan = _shared_plan(self.device, self.sample_rate, n, fmt)
        with plan.lock:
            if plan.handle is None:   # (evicted between the look-up and the lock)
                return self._run(x, fmt, n, freq_offset)
            return self._run_locked(plan.resize(n), x, freq_offset)

    def _run_locked(self, plan, x, freq_offset):
        info = plan.info
        if info.q == 1 and self.sample_rate > 480000 and int(self.sample_rate / 240000) > 1:
            logger.warning("Decimation failed: The length of the input vector x must be greater than "
                           "padlen, which is 27.")
        if not info.lpf_applied:
            logger.warning("Filter design failed, using unfiltered samples: The length of the input "
                           "vector x must be greater than padlen, which is 15.")
        hards, softs, bp, mm = plan.process(x, freq_offsets=[float(freq_offset)])
        self.symbols = softs[0]
        self.best_phase = int(bp[0])
        self.min_margin = float(mm[0])
        return hards[0]

    def close(self):
        """Kept for callers of earlier versions: plans are shared by all instances now (see close_plans)."""
