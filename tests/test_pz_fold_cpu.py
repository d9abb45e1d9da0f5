"""CPU: the raw-byte decimator's narrow blocks in the folded block-sum form (pz_raw_fold_lane: what the kernel ships at
q = 10) and in the per-sample form of the same body, both lock-step emulated and held against the oracle on the same rows.

tests/emul/emul.cpp reaches only the shipped form, so the per-sample figures -- the yardstick beside the folded ones -- come
from a harness of this test's own (tests/emul/pz_fold_harness.cpp: the same chain with FOLD = false, compiled here with g++),
which also hands out the decimator's finished output.

Conditions:
  * modulated rows: hard symbols, symbol count and timing phase equal the oracle's; soft symbols within 1e-12 of max|soft|
    (the kernel's own figure, pz_kernels.hpp on the permute conversion); the per-sample form has to meet that bound with a
    factor 3 to spare on every such row (a row on which it did not would be replaced by another seed and named here: none
    was), and the folded form's soft error may be at most 10 times the per-sample form's;
  * every row, the constant-pattern ones included: decimator output within 1e-12 of max|y_oracle|.  The bound is the soft
    symbols' -- they are samples of a unit-passband-gain filter of this output --, not a figure taken from either form.
    (On a constant input the reference's own phase pick is rounding noise, tests/golden_cases.py TIMING_DEGENERATE: those
    rows are held to this condition only.)
The rows: lengths that give narrow blocks between a first block and one or two tail blocks (block = 64 lanes x 120 samples).
The byte patterns are all-0x00, all-0xFF and alternating 0x00/0xFF (I = 0x00, Q = 0xFF throughout); one more row alternates
the SAMPLES (0x00,0x00 / 0xFF,0xFF: the largest window differences d_j = +-255, input at the Nyquist rate, output almost
nothing), held to 1e-12 of the input's full scale 1.0, which is what sets its error.

Figures of this test at the commit that added it (worst over the rows; folded / per-sample):
  decimator output error / max|y_oracle| : 6.4e-13 / 3.4e-13 (modulated), 1.0e-13 / 1.0e-13 (constant patterns)
  soft symbol error / max|soft|          : 2.7e-13 / 2.1e-13
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import OracleSignalProcessor
from tetraear_amd import synth

FS = 2.4e6
Q = 10
SOFT_BOUND = 1e-12
DEC_BOUND = 1e-12
_EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul")
_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tetraear_amd", "csrc")

# (name, length, kind, seed, freq_offset)
MODULATED = [
    ("dqpsk_262144_s11", 262144, "dqpsk", 11, 1171.875),
    ("dqpsk_262144_s12", 262144, "dqpsk", 12, -390.625),
    ("dqpsk_46157_s13", 46157, "dqpsk", 13, 0.0),
    ("dqpsk_24001_s14", 24001, "dqpsk", 14, 781.25),
    ("noise_38270_s15", 38270, "noise", 15, 0.0),   # (two tail blocks: the extension crosses a block boundary),
]
# (the largest window sums s_j come from all_ff, the largest differences d_j = +-255 from NYQUIST's sample-wise alternation:
#  bytes_00_ff, the byte-wise alternation, is I = 0x00, Q = 0xFF throughout and has d_j = 0 -- the two rows together are the
#  "largest s and d, worst cancellation" case)
CONSTANT = [
    ("all_00", 46157, "b00", 0, 0.0),
    ("all_ff", 46157, "bff", 0, 0.0),
    ("bytes_00_ff", 46157, "b00ff", 0, 0.0),
]
NYQUIST = [("samples_00_ff", 46157, "s00ff", 0, 0.0)]


def _row(kind, n, seed):
    if kind == "dqpsk":
        return synth.dqpsk_cu8(n, FS, seed=seed)[0]
    if kind == "noise":
        return synth.noise_cu8(n, seed)
    if kind == "b00":
        return np.zeros(2 * n, dtype=np.uint8)
    if kind == "bff":
        return np.full(2 * n, 255, dtype=np.uint8)
    if kind == "b00ff":
        return np.tile(np.array([0, 255], dtype=np.uint8), n)
    if kind == "s00ff":
        return np.tile(np.array([0, 0, 255, 255], dtype=np.uint8), (n + 1) // 2)[: 2 * n]
    raise KeyError(kind)


@pytest.fixture(scope="module")
def harness():
    src = os.path.join(_EMUL, "pz_fold_harness.cpp")
    out = os.path.join(_EMUL, "libpz_fold_harness.so")
    deps = [src, os.path.join(_EMUL, "emul.cpp")] + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-fPIC", "-std=c++20", "-ffp-contract=off", "-Wall",
                        "-Wno-unknown-pragmas", "-pthread", "-shared", "-o", out, src], check=True, cwd=_EMUL)
    return C.CDLL(out)


def _run(lib, fold, u8, n, foff):
    n_dec, ms, narrow = C.c_int64(), C.c_int32(), C.c_int32()
    rc = lib.pzf_run(int(fold), C.c_double(FS), C.c_int64(n), None, C.c_double(foff), None, None, None, None, None,
                     C.byref(n_dec), C.byref(ms), C.byref(narrow))
    assert rc == 0, "this length does not take the raw-byte decimator"
    y = np.zeros(n_dec.value, dtype=np.complex128)
    hard = np.zeros(ms.value, dtype=np.uint8)
    soft = np.zeros(ms.value, dtype=np.complex128)
    ns, bp = C.c_int32(), C.c_int32()
    u8 = np.ascontiguousarray(u8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.pzf_run(int(fold), C.c_double(FS), C.c_int64(n), vp(u8), C.c_double(foff), vp(y), vp(hard), vp(soft),
                     C.byref(ns), C.byref(bp), C.byref(n_dec), C.byref(ms), C.byref(narrow))
    assert rc == 0
    return dict(y=y, hard=hard[:max(ns.value - 1, 0)], soft=soft[:ns.value], bp=bp.value, narrow=narrow.value)


def _oracle(u8, foff):
    o = OracleSignalProcessor(FS)
    x = synth.cu8_to_c128(u8)
    hard = o.process(x, foff)
    return dict(y=o.decimate(x, Q), hard=hard, soft=o.symbols, bp=o.best_phase)


def _dec_err(got, ref, floor=0.0):
    assert len(got["y"]) == len(ref["y"])
    return np.max(np.abs(got["y"] - ref["y"])) / max(np.max(np.abs(ref["y"])), floor)


def _soft_err(got, ref):
    assert len(got["soft"]) == len(ref["soft"])
    return np.max(np.abs(got["soft"] - ref["soft"])) / np.max(np.abs(ref["soft"]))


@pytest.mark.parametrize("name,n,kind,seed,foff", MODULATED, ids=[c[0] for c in MODULATED])
def test_fold_modulated_rows(harness, name, n, kind, seed, foff):
    u8 = _row(kind, n, seed)
    ref = _oracle(u8, foff)
    per = _run(harness, 0, u8, n, foff)
    fold = _run(harness, 1, u8, n, foff)
    assert fold["narrow"] >= 1, "the length has no narrow block"
    d_fold, d_per = _dec_err(fold, ref), _dec_err(per, ref)
    s_fold, s_per = _soft_err(fold, ref), _soft_err(per, ref)
    print(f"\n{name}: narrow blocks {fold['narrow']}  decimator error folded {d_fold:.3e} per-sample {d_per:.3e}  "
          f"soft error folded {s_fold:.3e} per-sample {s_per:.3e}")
    # the yardstick has to be one the per-sample form passes alone, with room
    assert s_per <= SOFT_BOUND / 3, f"per-sample form {s_per:.3e}: replace this row's seed"
    for got in (fold, per):
        assert got["bp"] == ref["bp"]
        np.testing.assert_array_equal(got["hard"], ref["hard"])
    assert d_per <= DEC_BOUND and d_fold <= DEC_BOUND
    assert s_fold <= SOFT_BOUND
    assert s_fold <= 10 * s_per, "folded form spends more than ten times the per-sample form's error: shorten the segments"


@pytest.mark.parametrize("name,n,kind,seed,foff", CONSTANT + NYQUIST, ids=[c[0] for c in CONSTANT + NYQUIST])
def test_fold_constant_pattern_rows(harness, name, n, kind, seed, foff):
    u8 = _row(kind, n, seed)
    x = synth.cu8_to_c128(u8)
    ref = dict(y=OracleSignalProcessor(FS).decimate(x, Q))
    per = _run(harness, 0, u8, n, foff)
    fold = _run(harness, 1, u8, n, foff)
    assert fold["narrow"] >= 1
    floor = 1.0 if kind == "s00ff" else 0.0   # (Nyquist-rate row: against the input's full scale, see the module docstring)
    d_fold, d_per = _dec_err(fold, ref, floor), _dec_err(per, ref, floor)
    print(f"\n{name}: max|y_oracle| {np.max(np.abs(ref['y'])):.3e}  decimator error folded {d_fold:.3e} per-sample {d_per:.3e}")
    assert d_per <= DEC_BOUND and d_fold <= DEC_BOUND


def test_shipped_form_is_the_folded_one(harness):
    """tests/emul/emul.py (the emulation every other CPU test goes through) gives the folded harness run's symbols bit for bit."""
    from tests.emul import emul
    name, n, kind, seed, foff = MODULATED[2]
    u8 = _row(kind, n, seed)
    fold = _run(harness, 1, u8, n, foff)
    per = _run(harness, 0, u8, n, foff)
    hard, soft, n_soft, bp, mm = emul.process(FS, u8, "cu8", n, freq_offset=[foff])
    ns = int(n_soft[0])
    assert ns == len(fold["soft"])
    np.testing.assert_array_equal(soft[0, :ns], fold["soft"])
    assert not np.array_equal(fold["soft"], per["soft"]), "the two forms should differ in the last bits"
