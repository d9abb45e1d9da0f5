"""Shared input builders of the cs16 tests (tests/test_cs16_cpu.py, tests/test_cs16_gpu.py).

A cs16 row is interleaved int16 I, Q (little-endian); the value it means is s / 32768 exactly.  Every row has distinct
I and Q content, so a swapped pair or swapped bytes cannot pass:
  0  noise at roughly a quarter of full scale plus a tone at a positive, non-symmetric frequency
  1  the same kind of row, holding both -32768 and 32767
  2  values in {-1, 0, 1} only (low byte / sign extension)
  3  I at 0x0100 scale, Q at 0x0001 scale (byte order)
"""
import ctypes as C

import numpy as np

FMT_CS16 = 4
KINDS = 4


def row(kind, n, seed):
    """interleaved int16 [2 n] of row kind `kind` (kind % 4), from a seeded default_rng"""
    rng = np.random.default_rng(seed)
    kind %= KINDS
    out = np.empty(2 * n, dtype=np.int16)
    if kind in (0, 1):
        x = 0.17 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        x += 0.12 * np.exp(2j * np.pi * (0.0137 + 0.003 * (seed % 5)) * np.arange(n))
        out[0::2] = np.clip(np.rint(32768 * x.real), -32768, 32767)
        out[1::2] = np.clip(np.rint(32768 * x.imag), -32768, 32767)
        if kind == 1:
            at = rng.choice(n, size=4, replace=False)
            out[2 * at[0]], out[2 * at[1] + 1] = -32768, 32767
            out[2 * at[2]], out[2 * at[3] + 1] = 32767, -32768
    elif kind == 2:
        out[:] = rng.integers(-1, 2, size=2 * n)
    else:
        out[0::2] = rng.integers(-127, 128, size=n) * 256
        out[1::2] = rng.integers(-127, 128, size=n)
    return out


def rows(n, count, seed):
    """[count][2 n] int16: row r is of kind r % 4"""
    return np.stack([row(r, n, seed + 17 * r) for r in range(count)])


def c128(s16):
    """the reference value of interleaved int16 (last axis): s / 32768 as complex128"""
    s = np.asarray(s16).astype(np.float64) / 32768.0
    return s[..., 0::2] + 1j * s[..., 1::2]


def c64(s16):
    return c128(s16).astype(np.complex64)


def quantise(x, scale=0.5):
    """a complex signal brought to `scale` of full scale, as interleaved int16"""
    x = np.asarray(x) * (scale / np.max(np.abs(np.concatenate([x.real, x.imag]))))
    out = np.empty(2 * len(x), dtype=np.int16)
    out[0::2] = np.clip(np.rint(32768 * x.real), -32768, 32767)
    out[1::2] = np.clip(np.rint(32768 * x.imag), -32768, 32767)
    return out


def emu_process(sample_rate, iq, fmt, n, rows=1, stride=None, pre_shift=None, freq_offset=None):
    """tests/emul/emul.py process() with the wire format as its integer code (that module's name table stops at cf64; the
    library passes the code straight into run_ref)"""
    from tests.emul import emul
    L = emul.lib()
    L.emu_rows_per_chunk(1)
    ms = C.c_int32()
    L.emu_process(C.c_double(sample_rate), C.c_int64(n), rows, int(fmt), None, C.c_int64(0), None, None,
                  None, None, None, None, None, C.byref(ms))
    ms = ms.value
    hard = np.zeros((rows, ms), dtype=np.uint8)
    soft = np.zeros((rows, ms), dtype=np.complex128)
    n_soft = np.zeros(rows, dtype=np.int32)
    bp = np.zeros(rows, dtype=np.int32)
    mm = np.zeros(rows, dtype=np.float64)
    iq = np.ascontiguousarray(iq)
    ps = None if pre_shift is None else np.ascontiguousarray(pre_shift, dtype=np.float64)
    fo = None if freq_offset is None else np.ascontiguousarray(freq_offset, dtype=np.float64)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    L.emu_process(C.c_double(sample_rate), C.c_int64(n), rows, int(fmt), vp(iq), C.c_int64(n if stride is None else stride),
                  vp(ps), vp(fo), vp(hard), vp(soft), vp(n_soft), vp(bp), vp(mm), None)
    return hard, soft, n_soft, bp, mm


def emu_gate(iq, fmt, n, rows, fs):
    from tests.emul import emul
    L = emul.lib()
    iq = np.ascontiguousarray(iq)
    out = np.zeros((rows, 8))
    afc = np.zeros(rows)
    L.emu_gate(iq.ctypes.data_as(C.c_void_p), C.c_int64(n), rows, int(fmt), C.c_double(fs),
               out.ctypes.data_as(C.c_void_p), afc.ctypes.data_as(C.c_void_p))
    return out, afc
