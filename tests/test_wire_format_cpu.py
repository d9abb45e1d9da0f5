"""CPU: csrc/wire_format.hpp, the one definition of the IQ wire formats, as the host compiler builds it for tests/emul
(-ffp-contract=off), exhaustively over the integer codes, and held against the Python table (tetraear_amd/_lib.py
WIRE_FORMATS) and the header's enum.

fp64 must be, bit for bit, what the reference stack computes: cu8 as pyrtlsdr does, (u_I + 1j u_Q) / 127.5 - (1 + 1j) in
complex128 -- numpy divides a complex array by a real scalar by multiplying with fl(1 / 127.5), two roundings --, cs8 as
s / 128 and cs16 as s / 32768 (both exact).

fp32 must be the uncontracted float32 evaluation of the same expressions.  For cu8 that pins the HOST form only: a device
compiler may fuse u * fl(1/127.5f) - 1 into one fma, which gives other bits in 158 of the 256 codes.  The device form is
held by the instruction-for-instruction comparison of every kernel against the parent commit
(profiles/r13_wire_format_isa.txt)."""
import ctypes as C
import os
import re

import numpy as np

from tests.emul import emul
from tetraear_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decode(fmt, packed):
    """(complex128, complex64) of the packed samples through emu_wire_decode"""
    packed = np.ascontiguousarray(packed)
    n = packed.nbytes // _lib.WIRE_FORMATS[fmt][1]
    o64, o32 = np.zeros(2 * n, dtype=np.float64), np.zeros(2 * n, dtype=np.float32)
    rc = emul.lib().emu_wire_decode(emul.FMT[fmt], packed.ctypes.data_as(C.c_void_p), C.c_int64(n),
                                    o64.ctypes.data_as(C.c_void_p), o32.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return o64.view(np.complex128), o32.view(np.complex64)


def _bits_equal(a, b):
    return a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _byte_pairs(dtype):
    """all 65 536 (I, Q) byte pairs, interleaved"""
    i, q = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return np.stack([i.ravel(), q.ravel()], axis=1).astype(np.uint8).view(dtype).ravel()


def _int16_pairs():
    """all 65 536 int16 values in I with Q = ~I, then the same with I and Q swapped"""
    v = np.arange(-32768, 32768, dtype=np.int16)
    a = np.stack([v, ~v], axis=1)
    return np.concatenate([a, a[:, ::-1]]).ravel()


def test_cu8_every_byte_pair():
    u = _byte_pairs(np.uint8)
    got64, got32 = _decode("cu8", u)
    ref = u.astype(np.float64).view(np.complex128)   # pyrtlsdr read_samples / packed_bytes_to_iq
    ref /= 127.5
    ref -= (1 + 1j)
    assert _bits_equal(got64, ref)
    # host form only (see the module docstring): float32 multiply by fl32(1 / 127.5), rounded, then the subtraction
    ref32 = u.astype(np.float32) * (np.float32(1) / np.float32(127.5)) - np.float32(1)
    assert ref32.dtype == np.float32 and _bits_equal(got32, ref32.view(np.complex64))


def test_cs8_every_byte_pair():
    s = _byte_pairs(np.int8)
    got64, got32 = _decode("cs8", s)
    assert _bits_equal(got64, (s.astype(np.float64) / 128).view(np.complex128))
    assert _bits_equal(got32, (s.astype(np.float32) / np.float32(128)).view(np.complex64))


def test_cs16_every_int16_in_i_and_in_q():
    s = _int16_pairs()
    assert len(s) == 4 * 65536 and not np.array_equal(s[0::2], s[1::2])
    got64, got32 = _decode("cs16", s)
    assert _bits_equal(got64, (s.astype(np.float64) / 32768).view(np.complex128))
    assert _bits_equal(got32, (s.astype(np.float32) / np.float32(32768)).view(np.complex64))


def test_wire_bytes_equals_the_python_table():
    L = emul.lib()
    for name, (code, nbytes, dtype) in _lib.WIRE_FORMATS.items():
        assert L.emu_wire_bytes(code) == nbytes == _lib.FMT_BYTES[code], name
        assert nbytes % np.dtype(dtype).itemsize == 0, name
    codes = sorted(c for c, _, _ in _lib.WIRE_FORMATS.values())
    assert codes == list(range(len(codes)))
    assert L.emu_wire_bytes(-1) == -1 and L.emu_wire_bytes(len(codes)) == -1
    for name in ("cf32", "cf64"):      # (values, not codes: nothing to decode)
        assert L.emu_wire_decode(emul.FMT[name], None, C.c_int64(0), None, None) == -1


def test_format_codes_equal_the_header_enum():
    text = open(os.path.join(REPO, "include", "tetrahip.h")).read()
    enum = re.search(r"typedef enum tdm_fmt \{(.*?)\} tdm_fmt;", text, re.S).group(1)
    enum = re.sub(r"/\*.*?\*/", "", enum, flags=re.S)
    values = {k[len("TDM_"):].lower(): int(v) for k, v in re.findall(r"(TDM_\w+)\s*=\s*(\d+)", enum)}
    assert values == {name: code for name, (code, _, _) in _lib.WIRE_FORMATS.items()}
    assert values == emul.FMT
    for name, code in values.items():
        assert getattr(_lib, "FMT_" + name.upper()) == code
