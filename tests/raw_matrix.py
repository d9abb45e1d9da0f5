"""Shared by tests/test_raw_matrix_cpu.py and tests/test_raw_matrix_gpu.py: the raw-byte decimator (pz_raw_body, k_pz_raw)
at every decimation factor it is instantiated for, in calls of several rows -- the factors' sample rates, the block
geometry, the length classes, the row kinds, the comparisons with the oracle and the per-factor error table.

Geometry (pz_tables.hpp build_pz_tables, ref_pipeline.hpp run_pz_raw): a lane holds L = Q * S samples, a block B = 64 * L;
the padded row is P0 + n + 2 * 27 positions long with P0 = (L - 27 % L) % L.  Block 0 and the blocks from b_tail (the block
of the first position past the signal) on run the wide body, the blocks between them the narrow one (folded at q = 10).
"""
import os
import re

import numpy as np

from oracle.oracle import OracleSignalProcessor
from tetraear_amd import synth

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tetraear_amd", "csrc")
EDGE = 27            # ref_plan.hpp kEdgeSos
SOFT_TOL = 1e-10     # the project's bar for soft symbols on the device (tests/test_gpu_parity.py)
GPU_MARGIN = 8       # the device build contracts multiply-adds and orders its sums differently from the emulation

# one sample rate per factor: int(rate / 240 000) is the factor (design.hpp decimation_factor)
RATE_OF_Q = {3: 900e3, 4: 1.024e6, 6: 1.536e6, 7: 1.8e6, 8: 2.048e6, 10: 2.4e6, 12: 2.88e6, 13: 3.2e6, 41: 10e6}

# Worst soft-symbol error of the CPU emulation against the ORACLE over the matrix of tests/test_raw_matrix_cpu.py, per
# factor, as a fraction of max|soft| (the Nyquist rows: of the input's full scale), measured when the tests were written and
# rounded up to two digits.  The CPU test holds its own figure between a tenth of the entry and the entry, the GPU test
# holds the device to GPU_MARGIN times the entry (and to SOFT_TOL).
RAW_SOFT_WORST = {
    3: 6.2e-13, 4: 1.6e-13, 6: 2.1e-13, 7: 1.6e-13, 8: 1.5e-13, 10: 2.6e-13, 12: 3.2e-13, 13: 1.4e-13, 41: 3.8e-12,
}

KINDS = ("noise", "rand0255", "b00", "bff", "b00ff", "s00ff")
STRICT_KINDS = ("noise", "rand0255")          # the oracle's timing pick is well defined: everything has to be equal
PATTERN_KINDS = ("b00", "bff", "b00ff", "s00ff")   # run with freq_offset 0; the first three are timing-degenerate (check_row)
LENGTH_CLASSES = ("B-1", "B+1", "2B+3", "3B-5", "3B+L+1", "5B+7", "B/2+1", "two_tail")


def _cases(macro):
    with open(os.path.join(_CSRC, "ref_plan.hpp")) as f:
        text = f.read()
    m = re.search(r"#define\s+%s\(X\)(.*)" % macro, text)
    assert m, macro
    return {int(q): int(s) for q, s in re.findall(r"X\((\d+),\s*(\d+)\)", m.group(1))}


def raw_cases():
    """{Q: S} of the raw-byte decimator's instantiations (TDM_PZR_CASES_A / _B of ref_plan.hpp)"""
    out = _cases("TDM_PZR_CASES_A")
    out.update(_cases("TDM_PZR_CASES_B"))
    return out


def pz_cases():
    """{Q: S} of the double-based parallel-form decimator (TDM_PZ_CASES)"""
    return _cases("TDM_PZ_CASES")


def geometry(L, n):
    """The launch of a parallel-form decimator with lanes of L samples on rows of n: blocks nb, first tail block b_tail,
    narrow blocks (1 .. b_tail - 1) and tail blocks (b_tail .. nb - 1)."""
    B = 64 * L
    P0 = (L - EDGE % L) % L
    nb = (P0 + n + 2 * EDGE + B - 1) // B
    b_tail = min((P0 + EDGE + n) // B, nb - 1)
    return dict(L=L, B=B, nb=nb, b_tail=b_tail, narrow=max(b_tail - 1, 0), tail=nb - b_tail)


def two_tail_length(L, m=3, even=False):
    """A length whose tail extension crosses the boundary between blocks m - 1 and m: the signal ends in block m - 1, the
    extension in block m.  Found by walking down from the boundary, not by formula, so that the search and the geometry
    above have to agree."""
    B = 64 * L
    for n in range(m * B, (m - 1) * B, -1):
        g = geometry(L, n)
        if g["tail"] == 2 and g["nb"] == m + 1 and (n % 2 == 0) == even and geometry(L, n + 6)["tail"] == 2 and geometry(L, n - 6)["tail"] == 2:
            return n
    raise AssertionError("no two-tail-block length")


def class_lengths(q, S):
    """{class name: n}"""
    L = q * S
    B = 64 * L
    return {"B-1": B - 1, "B+1": B + 1, "2B+3": 2 * B + 3, "3B-5": 3 * B - 5, "3B+L+1": 3 * B + L + 1, "5B+7": 5 * B + 7,
            "B/2+1": B // 2 + 1, "two_tail": two_tail_length(L, 3, even=True)}


def check_class(name, g):
    """the class holds what its name says (g = geometry of its length)"""
    want = {"B-1": (2, 0, 1), "B+1": (2, 0, 1), "2B+3": (3, 1, 1), "3B-5": (4, 2, 1), "3B+L+1": (4, 2, 1), "5B+7": (6, 4, 1),
            "B/2+1": (1, 0, 1), "two_tail": (4, 1, 2)}[name]
    assert (g["nb"], g["narrow"], g["tail"]) == want, (name, g)


def make_row(kind, n, seed):
    """2 n bytes, I and Q interleaved"""
    if kind == "noise":
        return synth.noise_cu8(n, seed)
    if kind == "rand0255":
        return (np.random.default_rng(seed).integers(0, 2, size=2 * n, dtype=np.uint8) * 255).astype(np.uint8)
    if kind == "b00":
        return np.zeros(2 * n, dtype=np.uint8)
    if kind == "bff":
        return np.full(2 * n, 255, dtype=np.uint8)
    if kind == "b00ff":   # byte-wise alternation: I = 0x00, Q = 0xFF throughout
        return np.tile(np.array([0, 255], dtype=np.uint8), n)
    if kind == "s00ff":   # Nyquist: the SAMPLES alternate (0x00, 0x00) / (0xFF, 0xFF)
        return np.tile(np.array([0, 0, 255, 255], dtype=np.uint8), (n + 1) // 2)[: 2 * n]
    raise KeyError(kind)


def row_offset(kind, i, rate_dec):
    """every row its own freq_offset; the constant patterns run with none (see check_row)"""
    if kind in PATTERN_KINDS:
        return 0.0
    return ((i * 5) % 11 - 5) * rate_dec / 2048.0 + (i + 1) * 7.8125


def layout(rows, n, stride, base, kinds, seed):
    """The input of one call: `rows` rows of n samples, `stride` samples apart (0: every row reads the same samples), the
    first `base` samples in front of row 0; row r is of kind kinds[r % len(kinds)].  Returns (bytes, per-row kinds): the
    buffer ends with the last row's last byte, and what lies between pitched rows is filler no row may read."""
    total = base + (rows - 1) * stride + n
    buf = np.random.default_rng(seed ^ 0x5EED).integers(0, 256, size=2 * total, dtype=np.uint8)
    out = []
    for r in range(rows if stride else 1):
        k = kinds[r % len(kinds)]
        o = 2 * (base + r * stride)
        buf[o:o + 2 * n] = make_row(k, n, seed + 101 * r)
        out.append(k)
    if not stride:
        out = out * rows
    return buf, out


MATRIX_ROWS = 6
MATRIX_STRIDES = ("n", "other_parity", "pitched", "zero")
_MATRIX_BASES = (0, 1, 3, 0, 3, 1, 0, 1)


def matrix_cases(q):
    """The matrix of one factor: one call of MATRIX_ROWS rows per length class.  Stride kind and the first row's offset into
    its buffer move against the classes from factor to factor (each factor sees every stride kind twice) instead of being
    crossed with them.  Strided calls hold one row of each kind, at a position that moves with the class; a stride-0 call
    is one noise or random row read by every plan row, each with its own freq_offset.
    Yields dicts: cname, n, skind, stride, base, buf (the bytes), kinds and foffs (per row), where."""
    S = raw_cases()[q]
    fi = sorted(raw_cases()).index(q)
    lengths = class_lengths(q, S)
    for ci, cname in enumerate(LENGTH_CLASSES):
        n = lengths[cname]
        skind = MATRIX_STRIDES[(ci + fi) % 4]
        stride = {"n": n, "other_parity": n + 1, "pitched": n + 4 + (n // 64) % 3, "zero": 0}[skind]
        base = _MATRIX_BASES[(ci + 3 * fi) % 8]
        kinds = tuple(KINDS[(k + ci) % 6] for k in range(6)) if stride else (STRICT_KINDS[(ci + fi) % 2],)
        buf, rkinds = layout(MATRIX_ROWS, n, stride, base, kinds, seed=1000 * q + ci)
        foffs = [row_offset(rkinds[r], r + ci, RATE_OF_Q[q] / q) for r in range(MATRIX_ROWS)]
        yield dict(cname=cname, n=n, skind=skind, stride=stride, base=base, buf=buf, kinds=rkinds, foffs=foffs,
                   where=f"q={q} {cname} n={n} stride={skind}({stride}) base={base}")


def row_bytes(buf, n, stride, base, r):
    """exactly the bytes row r was given"""
    o = 2 * (base + r * stride)
    return buf[o:o + 2 * n]


def oracle_row(rate, u8, foff):
    o = OracleSignalProcessor(rate)
    hard = o.process(synth.cu8_to_c128(u8), foff)
    return dict(hard=hard, soft=o.symbols, bp=o.best_phase)


def check_row(kind, hard, soft, bp, ref, where):
    """One row against the oracle's result for its bytes; returns the soft error the bound is held against.
    noise / random rows: count, hard symbols and timing phase equal, soft error as a fraction of max|soft|.
    constant patterns (freq_offset 0): the oracle's timing pick is rounding noise, so the count may differ by one and the
    hard symbols are compared over the common length; every soft symbol is held to the oracle's -- flat -- value.
    Nyquist row (freq_offset 0): its oracle output is NOT flat and its timing pick is NOT degenerate -- the odd extension of
    an alternating row is a 27-sample pedestal at each end, which the filters pass: the first symbol is 1.4, the ones
    behind it decay to the interior's rounding residue of 1e-17.  So the row is held index by index: count and timing phase
    equal, soft error against the input's full scale 1.0 (tests/test_pz_fold_cpu.py), and the hard symbols equal wherever
    the oracle's own decision is DEFINED, i.e. could not be moved over a threshold by a soft error the SOFT_TOL bar admits
    (decision k, between symbols k and k + 1: angular margin above 2 (eps / |s_k| + eps / |s_k+1|), eps = 1e-10): in the
    interior both sides decide on their own rounding residue and no implementation could equal the oracle's there.  At
    least the 4 decisions at the start are asserted to be defined, so the comparison never goes empty."""
    if kind in STRICT_KINDS:
        assert len(soft) == len(ref["soft"]) and len(soft) >= 2, (where, len(soft), len(ref["soft"]))
        assert bp == ref["bp"], (where, bp, ref["bp"])
        np.testing.assert_array_equal(hard, ref["hard"], err_msg=str(where))
        return float(np.max(np.abs(soft - ref["soft"])) / np.max(np.abs(ref["soft"])))
    assert kind in PATTERN_KINDS
    if kind == "s00ff":
        s = ref["soft"]
        assert len(soft) == len(s) and len(soft) >= 5, (where, len(soft), len(s))
        assert bp == ref["bp"], (where, bp, ref["bp"])
        ph = np.angle(s[1:] * np.conj(s[:-1]))
        thr = np.array([-5 * np.pi / 8, -3 * np.pi / 8, 3 * np.pi / 8, 5 * np.pi / 8])
        margin = np.min(np.abs(ph[:, None] - thr[None, :]), axis=1)
        mag = np.maximum(np.abs(s), 1e-300)
        defined = margin > 2 * (SOFT_TOL / mag[1:] + SOFT_TOL / mag[:-1])
        assert np.all(defined[:4]), (where, "the end transient's decisions should be defined", margin[:4], mag[:5])
        np.testing.assert_array_equal(hard[defined], ref["hard"][defined], err_msg=str(where))
        return float(np.max(np.abs(soft - s)))
    assert abs(len(soft) - len(ref["soft"])) <= 1 and len(soft) >= 2, (where, len(soft), len(ref["soft"]))
    m = min(len(hard), len(ref["hard"]))
    np.testing.assert_array_equal(hard[:m], ref["hard"][:m], err_msg=str(where))
    flat = np.mean(ref["soft"])
    scale = 1.0 if kind == "s00ff" else float(np.max(np.abs(ref["soft"])))
    spread = float(np.max(np.abs(ref["soft"] - flat)) / scale)
    # (the reference's own departure from flat, part of the figure returned: it has to stay far below the bar -- 5e-13 at
    #  the factors up to 13, 1e-12 at q = 41)
    assert spread <= SOFT_TOL / 10, (where, "the oracle's own output is not flat", spread)
    return float(np.max(np.abs(soft - flat)) / scale)
