"""Shared input builders of the cs16 tests (tests/test_cs16_cpu.py, tests/test_cs16_gpu.py).

A cs16 row is interleaved int16 I, Q (little-endian); the value it means is s / 32768 exactly.  Every row has distinct
I and Q content, so a swapped pair or swapped bytes cannot pass:
  0  noise at roughly a quarter of full scale plus a tone at a positive, non-symmetric frequency
  1  the same kind of row, holding both -32768 and 32767
  2  values in {-1, 0, 1} only (low byte / sign extension)
  3  I at 0x0100 scale, Q at 0x0001 scale (byte order)
"""
import numpy as np

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
