"""CPU: the scan terms the raw-byte decimator leaves out (pz_tables.hpp PzScanKeep, pz_kernels.hpp pz_block_finish).

A lane's end state reaches the lane d lanes away through C^(L d), which decays like |p|^(L d), p the pole of the pair and L
the lane length.  The five terms of a pair are the Kogge-Stone steps d = 1, 2, 4, 8 and the multiply by C^(16 L) in the
second row-total step; a term whose bound |p|^(L d) is under 1e-24 (kPzScanNegligible, the constant of the low-rate
kernel's scan_rows) is compiled out, per factor, by a constexpr table.

Part 1, test_compiled_table_is_the_rule: for all nine (Q, S) of the raw-byte kernel, every compiled-out (pair, term) has its
long-double bound under the constant and every kept one is at or above it (the row-total steps are not in the table: they
always stay).  The pair order is not assumed: the |p|^2 the tables hold per pair are held against the oracle's own design
(oracle/design.py, scipy's section order) pair by pair, and the bounds are formed a second time here, in numpy's long
double, from that design.  The plan's own check (pz_scan_keep_is_safe, which decides whether a plan may run the pruned
kernel) says yes for the shipped tables and no for a table that drops one more term of the slowest pair.

Part 2, test_pruned_equals_every_term: the emulation runs what ships, which is pruned (tests/emul/emul.cpp); a harness of
this test's own (tests/emul/scan_prune_harness.cpp, compiled here with g++) runs the same chain with every term.  Soft
symbols, hard symbols, n_soft and best_phase are np.array_equal for q = 10 and for q = 3 (a factor whose table drops the
most: seven of twenty terms), at 3B - 5 (wide first block, two narrow blocks, wide tail) and 5B + 7, six rows a call: noise,
random 0x00 / 0xFF bytes, all-0x00, the Nyquist alternation, two blocks of 0x00 followed by 0xFF to the end (the largest
jump between distant and local states) and the same reversed.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import design as odesign
from tests import raw_matrix as rm

_EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul")
_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tetraear_amd", "csrc")
CONSTANT = 1e-24
TERMS = 5
DISTANCE = (1, 2, 4, 8, 16)   # lanes: four Kogge-Stone steps, the far multiply
CASES = rm.raw_cases()
ROW_KINDS = ("noise", "rand0255", "b00", "s00ff", "step_up", "step_down")


def make_row(kind, n, seed, B):
    """2 n bytes; the step rows: two blocks of one byte value, the other to the end"""
    if kind == "step_up":
        return np.concatenate([np.zeros(4 * B, dtype=np.uint8), np.full(2 * n - 4 * B, 255, dtype=np.uint8)])
    if kind == "step_down":
        return np.concatenate([np.full(4 * B, 255, dtype=np.uint8), np.zeros(2 * n - 4 * B, dtype=np.uint8)])
    return rm.make_row(kind, n, seed)


def six_rows(q, n, seed):
    B = 64 * q * CASES[q]
    assert n > 2 * B
    return np.concatenate([make_row(k, n, seed + 101 * r, B) for r, k in enumerate(ROW_KINDS)])


def row_offsets(q):
    return [0.0 if k in ("b00", "s00ff", "step_up", "step_down") else rm.row_offset(k, r, rm.RATE_OF_Q[q] / q) for r, k in enumerate(ROW_KINDS)]


@pytest.fixture(scope="module")
def harness():
    src = os.path.join(_EMUL, "scan_prune_harness.cpp")
    out = os.path.join(_EMUL, "libscan_prune_harness.so")
    deps = [src, os.path.join(_EMUL, "emul.cpp")] + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-fPIC", "-std=c++20", "-ffp-contract=off", "-Wall",
                        "-Wno-unknown-pragmas", "-pthread", "-shared", "-o", out, src], check=True, cwd=_EMUL)
    return C.CDLL(out)


def _table(lib, q):
    geom = (C.c_int32 * 4)()
    kept = (C.c_int32 * 4)()
    a2 = (C.c_double * 4)()
    below = (C.c_int32 * (4 * TERMS))()
    bound = (C.c_double * (4 * TERMS))()
    const, ok = C.c_double(), C.c_int32()
    rc = lib.spr_table(C.c_double(rm.RATE_OF_Q[q]), geom, kept, a2, below, bound, C.byref(const), C.byref(ok))
    assert rc == 0, q
    return dict(geom=list(geom), kept=list(kept), a2=np.array(a2), below=np.array(below).reshape(4, TERMS),
                bound=np.array(bound).reshape(4, TERMS), constant=const.value, plan_ok=ok.value)


@pytest.mark.parametrize("q", sorted(CASES))
def test_compiled_table_is_the_rule(harness, q):
    t = _table(harness, q)
    S = CASES[q]
    L = q * S
    assert t["geom"] == [q, S, L, TERMS]
    assert t["constant"] == CONSTANT
    # ---- the pair order: the tables' |p|^2 against the oracle's design, section by section
    sos = odesign.cheby1_lowpass_sos(8, 0.05, 0.8 / q)
    np.testing.assert_allclose(t["a2"], sos[:, 5], rtol=1e-12, atol=0, err_msg=f"q={q}: the tables' pairs are not the design's sections in order")
    assert np.all(np.diff(sos[:, 5]) > 0), "scipy's order: the pair closest to the unit circle last"
    # ---- the bounds once more, from the oracle's design, in numpy's long double
    p2 = sos[:, 5].astype(np.longdouble)
    for s in range(4):
        kept = t["kept"][s]
        assert 1 <= kept <= TERMS, (q, s, kept)
        for term, d in enumerate(DISTANCE):
            b = np.power(p2[s], np.longdouble(L * d) / 2)
            assert abs(float(b) - t["bound"][s, term]) <= 1e-9 * float(b), (q, s, term, float(b), t["bound"][s, term])
            under = bool(b < np.longdouble(CONSTANT))
            assert under == bool(t["below"][s, term]), (q, s, term, float(b))
            if term >= kept:
                assert under, f"q={q} pair {s} term d={d}: compiled out at bound {float(b):.3e}, not under {CONSTANT}"
            else:
                assert not under, f"q={q} pair {s} term d={d}: kept at bound {float(b):.3e}, under {CONSTANT}"
    print(f"\nSCAN_PRUNE q={q} S={S} L={L} kept per pair (design order) {t['kept']}  dropped terms {4 * TERMS - sum(t['kept'])}")
    # ---- the plan's own check
    assert t["plan_ok"] == 1
    assert harness.spr_table_is_safe(C.c_double(rm.RATE_OF_Q[q]), (C.c_int32 * 4)(*t["kept"])) == 1
    if t["kept"][3] > 1:
        worse = list(t["kept"])
        worse[3] -= 1   # (one more term of the slowest pair)
        while worse[3] > 0 and t["below"][3, worse[3]]:
            worse[3] -= 1
        assert harness.spr_table_is_safe(C.c_double(rm.RATE_OF_Q[q]), (C.c_int32 * 4)(*worse)) == 0


def test_q3_drops_the_most():
    """the factor part 2 takes beside q = 10 is one whose table drops the most terms"""
    with open(os.path.join(_CSRC, "pz_tables.hpp")) as f:
        import re
        rows = re.findall(r"^TDM_PZ_SCAN_KEEP\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)", f.read(), re.M)
    dropped = {int(r[0]): 4 * TERMS - sum(int(x) for x in r[2:]) for r in rows}
    assert dropped[3] == max(dropped.values()) and dropped[10] > 0, dropped


def _run(lib, prune, q, n, u8, foffs):
    rows = len(ROW_KINDS)
    rate = rm.RATE_OF_Q[q]
    ms = C.c_int32()
    rc = lib.spr_run(int(prune), C.c_double(rate), C.c_int64(n), rows, None, C.c_int64(n), None, None, None, None, None, C.byref(ms))
    assert rc == 0, "this length does not take the raw-byte decimator"
    hard = np.zeros((rows, ms.value), dtype=np.uint8)
    soft = np.zeros((rows, ms.value), dtype=np.complex128)
    ns = np.zeros(rows, dtype=np.int32)
    bp = np.zeros(rows, dtype=np.int32)
    fo = np.asarray(foffs, dtype=np.float64)
    u8 = np.ascontiguousarray(u8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.spr_run(int(prune), C.c_double(rate), C.c_int64(n), rows, vp(u8), C.c_int64(n), vp(fo), vp(hard), vp(soft), vp(ns), vp(bp),
                     C.byref(ms))
    assert rc == 0
    return hard, soft, ns, bp


@pytest.mark.parametrize("q,cname", [(10, "3B-5"), (10, "5B+7"), (3, "3B-5"), (3, "5B+7")])
def test_pruned_equals_every_term(harness, q, cname):
    n = rm.class_lengths(q, CASES[q])[cname]
    rm.check_class(cname, rm.geometry(q * CASES[q], n))
    u8 = six_rows(q, n, seed=7000 + q)
    foffs = row_offsets(q)
    pruned = _run(harness, 1, q, n, u8, foffs)
    every = _run(harness, 0, q, n, u8, foffs)
    assert np.all(pruned[2] >= 2)
    for name, a, b in zip(("hard", "soft", "n_soft", "best_phase"), pruned, every):
        if name == "soft":
            a, b = a.view(np.float64), b.view(np.float64)
        assert np.array_equal(a, b), f"q={q} {cname} n={n}: {name} of the pruned scans differs from the scans with every term"
    if cname == "3B-5":
        # (the harness' pruned run is the emulation every other CPU test goes through)
        from tests.emul import emul
        hard, soft, n_soft, bp, mm = emul.process(rm.RATE_OF_Q[q], u8, "cu8", n, rows=len(ROW_KINDS), freq_offset=foffs)
        assert np.array_equal(n_soft, pruned[2]) and np.array_equal(bp, pruned[3])
        for r in range(len(ROW_KINDS)):
            assert np.array_equal(soft[r, :n_soft[r]].view(np.float64), pruned[1][r, :n_soft[r]].view(np.float64))
