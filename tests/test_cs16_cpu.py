"""CPU: the cs16 wire format (interleaved little-endian int16 I, Q; value s / 32768) in the lock-step emulation of the
kernel bodies and in the Python plumbing that needs no device.

s / 32768 is exact in fp64, and the loaders convert where they load, so a cs16 call is the cf64 call on the same values
behind another loader: the outputs are compared bit for bit with the emulation fed those values as cf64, and against the
oracle's process() on them.  Rates: 2.4 MS/s (q = 10, parallel-form decimator) and 5.52 MS/s (cascade engine)."""
import os

import numpy as np
import pytest

from tests import cs16_cases as cc
from tests.emul import emul

SOFT_TOL = 1e-10          # the project's reference-mode bound (tests/test_wire_formats_gpu.py SOFT_TOL)
FOFFS = np.array([-2750.0, -1171.875, 0.0, 613.5])
RATES = [2.4e6, 5.52e6]
LENGTHS = [40001, 65536 + 13]
_oracle_cache = {}


def _oracle(fs, x, foff, shift=None):
    """the oracle's process() on reference values; computed once per (input, offsets) and shared"""
    from oracle.oracle import OracleSignalProcessor
    key = (fs, len(x), float(x[:64].sum().real), float(x[-64:].sum().imag), float(foff), shift)
    if key not in _oracle_cache:
        o = OracleSignalProcessor(fs)
        hard = o.process(x if shift is None else o.frequency_shift(x, shift), foff)
        _oracle_cache[key] = (hard, o.symbols, o.best_phase)
    return _oracle_cache[key]


def _check_rows_vs_oracle(fs, xs, foffs, out, what, shifts=None):
    hard, soft, n_soft, bp, mm = out
    for r in range(len(foffs)):
        x = xs[r] if shifts is None else xs
        ref_hard, ref_soft, ref_bp = _oracle(fs, x, foffs[r], None if shifts is None else float(shifts[r]))
        k = int(n_soft[r])
        assert k == len(ref_soft) and k > 100, (what, r)
        np.testing.assert_array_equal(hard[r, :k - 1], ref_hard, err_msg=f"{what} row {r}")
        assert int(bp[r]) == ref_bp, (what, r)
        assert np.max(np.abs(soft[r, :k] - ref_soft)) <= SOFT_TOL * np.max(np.abs(ref_soft)), (what, r)


def _equal_all_five(a, b, what):
    for name, u, v in zip(("hard", "soft", "n_soft", "best_phase", "min_margin"), a, b):
        assert np.array_equal(u, v), (what, name)


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("n", LENGTHS)
def test_emul_cs16_rows_vs_oracle_and_equal_to_cf64(fs, n):
    s16 = cc.rows(n, 4, seed=1600 + n % 11)
    xs = cc.c128(s16)
    got = emul.process(fs, s16, "cs16", n, rows=4, freq_offset=FOFFS)
    _check_rows_vs_oracle(fs, xs, FOFFS, got, f"cs16 fs {fs} n {n}")
    same = emul.process(fs, xs, "cf64", n, rows=4, freq_offset=FOFFS)
    _equal_all_five(got, same, f"cs16 against cf64, fs {fs} n {n}")


@pytest.mark.parametrize("fs", RATES)
def test_emul_cs16_shared_input_with_pre_shifts(fs):
    """one cs16 stream, five carriers shifted out of it: row r is process(frequency_shift(s / 32768, shift_r), foff_r)"""
    n = 40001
    s16 = cc.row(0, n, seed=1650)
    x = cc.c128(s16)
    shifts = np.array([-600000.0, -25000.0, 0.0, 37500.0, 412500.0])
    foffs = np.array([-2750.0, -1171.875, 0.0, 613.5, 2990.25])
    got = emul.process(fs, s16, "cs16", n, rows=5, stride=0, pre_shift=shifts, freq_offset=foffs)
    _check_rows_vs_oracle(fs, x, foffs, got, f"cs16 shared fs {fs}", shifts=shifts)
    same = emul.process(fs, x, "cf64", n, rows=5, stride=0, pre_shift=shifts, freq_offset=foffs)
    _equal_all_five(got, same, f"cs16 shared against cf64, fs {fs}")


@pytest.mark.parametrize("fs", RATES)
def test_emul_cs16_row_stride_of_n_plus_one(fs):
    """rows n + 1 samples apart: every other row starts 4 bytes off an 8-byte boundary; the pad sample is never read"""
    n = 40001
    s16 = cc.rows(n, 4, seed=1660)
    padded = np.full((4, 2 * (n + 1)), 0x7abc, dtype=np.int16)
    padded[:, :2 * n] = s16
    got = emul.process(fs, padded, "cs16", n, rows=4, stride=n + 1, freq_offset=FOFFS)
    dense = emul.process(fs, s16, "cs16", n, rows=4, freq_offset=FOFFS)
    _equal_all_five(got, dense, f"stride n + 1, fs {fs}")
    _check_rows_vs_oracle(fs, cc.c128(s16), FOFFS, got, f"cs16 stride n + 1 fs {fs}")


def test_emul_gate_cs16_equals_cf64():
    n, fs = 16384, 2.4e6
    s16 = cc.rows(n, 4, seed=1670)
    out, afc = emul.gate(s16, "cs16", n, 4, fs)
    ref_out, ref_afc = emul.gate(cc.c128(s16), "cf64", n, 4, fs)
    assert np.array_equal(out, ref_out) and np.array_equal(afc, ref_afc)
    assert np.all(np.isfinite(out)) and len(np.unique(out[:, 0])) == 4      # (the rows are different signals)


def test_python_tables_and_header_know_cs16():
    from tetraear_amd import _lib, batch, channeliser, gate, stream, wideband
    assert _lib.WIRE_FORMATS["cs16"][:2] == (4, 4) and _lib.FMT_CS16 == 4 and _lib.FMT_BYTES[_lib.FMT_CS16] == 4
    for mod in (batch, channeliser, wideband, gate):
        assert mod.ACCEPTS["cs16"] == 4, mod.__name__
    assert "cs16" not in stream.ACCEPTS      # (tdm_stream_create does not take it: include/tetrahip.h)
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tetrahip.h")
    import re
    text = open(header).read()
    enum = re.search(r"typedef enum tdm_fmt \{(.*?)\} tdm_fmt;", text, re.S).group(1)
    enum = re.sub(r"/\*.*?\*/", "", enum, flags=re.S)
    values = {k: int(v) for k, v in re.findall(r"(TDM_\w+)\s*=\s*(\d+)", enum)}
    assert values == {"TDM_CU8": 0, "TDM_CS8": 1, "TDM_CF32": 2, "TDM_CF64": 3, "TDM_CS16": 4}
    assert _lib.header_version(header) == _lib.ABI_VERSION


def test_cs16_builder_rows_are_what_they_claim():
    s = cc.rows(5000, 4, seed=1)
    assert s[1].min() == -32768 and s[1].max() == 32767
    assert set(np.unique(s[2])) == {-1, 0, 1}
    assert np.all(s[3, 0::2] % 256 == 0) and np.max(np.abs(s[3, 1::2])) < 128
    for r in range(4):
        assert not np.array_equal(s[r, 0::2], s[r, 1::2])
    x = cc.c128(s)
    assert x.dtype == np.complex128 and x[1].real.min() == -1.0
    # s / 32768 survives the two-term bf16 split of the fused receiver exactly: 16 significant bits in two 8-bit halves
    v = np.arange(-32768, 32768).astype(np.float32) / np.float32(32768)
    hi = (v.view(np.uint32) + 0x7fff + ((v.view(np.uint32) >> 16) & 1)) & 0xffff0000
    hi = hi.astype(np.uint32).view(np.float32)
    lo = v - hi
    lo_b = ((lo.view(np.uint32) + 0x7fff + ((lo.view(np.uint32) >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)
    assert np.array_equal(hi + lo_b, v)
