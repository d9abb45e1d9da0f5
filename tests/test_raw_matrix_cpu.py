"""CPU: the raw-byte decimator's body (pz_raw_body) lock-step emulated at EVERY factor it is instantiated for, in calls of six
rows, against the oracle run on exactly the bytes each row was given.

Until this file the emulation reached the raw body with one row per call only (every multi-row cu8 case carried pre-shifts,
which switch the raw body off), so nothing indexed by `row` in it -- rowp, Ef / Eb, Elast, flast, Hb, y0 -- was ever seen
at row > 0, and the extreme byte patterns were held at q = 10 and one length.

The matrix, per factor (tests/raw_matrix.py):
  * lengths B-1, B+1, 2B+3, 3B-5, 3B+L+1, 5B+7, B/2+1 (L = Q S samples per lane, B = 64 L per block) and one length whose
    tail extension crosses a block boundary (two tail blocks); each class is asserted to hold the blocks its name says, and
    the plan is asserted to be one tdm_plan_get_info would report as dec_engine 3 (emul.dec_engine);
  * six rows per call, one of each kind -- noise, random 0x00/0xFF bytes, all-0x00, all-0xFF, the byte-wise alternation, the
    Nyquist sample alternation -- at a row position that moves with the length class; every row its own freq_offset;
  * row strides n (odd for seven of the classes: every second row starts 2 bytes off a dword and takes the uint16 pair
    loads), n + 1, a pitched stride and 0 (all rows share one input), and the first row 0, 1 or 3 samples into its buffer;
    stride and start move against the length classes from factor to factor instead of being crossed with them.
Conditions (raw_matrix.check_row): noise and random rows equal the oracle's count, hard symbols and timing phase, soft
symbols within the bound; the constant patterns run with freq_offset 0 and are compared phase-agnostically (the oracle's
timing pick on them is rounding noise: count within one, hard symbols over the common length, every soft symbol against
the oracle's flat value).  The Nyquist row turned out to be neither flat nor timing-degenerate -- its odd extension is a
pedestal at each end, the first symbol is 1.4 and the oracle picks phase 0 at every shape here -- so it is held index by
index like a noise row (count, phase, soft error against the input's full scale 1.0), except that hard symbols are
compared only where the oracle's own decision is defined: in the interior both sides slice 1e-17 of rounding residue.
The bound: the factor's worst error has to lie between a tenth of RAW_SOFT_WORST[q] and RAW_SOFT_WORST[q] (a stale entry
hides drift in neither direction), and below the 1e-10 bar of the device tests.

Figures at the commit that added the file (worst over the matrix, fraction of max|soft|; strict rows / pattern rows):
  q = 3   6.1e-13 / 4.5e-13      q = 7   1.5e-13 / 1.2e-13      q = 12  3.2e-13 / 1.1e-13
  q = 4   1.6e-13 / 1.5e-13      q = 8   1.3e-13 / 1.5e-13      q = 13  1.4e-13 / 5.4e-14
  q = 6   1.3e-13 / 2.1e-13      q = 10  2.6e-13 / 1.2e-13      q = 41  3.3e-12 / 3.7e-12
At q = 41 the worst noise row is the half-block class (2625 samples: 5 symbols to normalise by), the worst pattern row
all-0xFF at 5B+7; the oracle's own constant-row output there is flat to 1e-12 only.  Lengths of 28, 29 and 161 samples
(n_dec <= 15: no channel filter) never take the raw-byte decimator and are no part of the matrix.

What the matrix catches (each change made alone on a scratch copy; test_raw_matrix_emulated then fails at the factors named;
"before": whether tests/test_emul_parity.py and tests/test_pz_fold_cpu.py noticed):
  flast row offset dropped (row * 2 -> 0) in the raw body's store      all nine (NaN from the unwritten slots)    before: no
  ... where the carry reads it                                          eight: 2.7e-6 at q = 3 down to 2.7e-10 at q = 12,
      13; at q = 41 the last extended sample weighs less than the rows' spread (3.4e-12) -- the code is one function for
      all factors                                                                                                   before: 2 tests
  Elast row offset dropped, store or read                               all nine                                   before: 3 tests
  first tail block one too large                                        all nine                                   before: 1 test
  first tail block one too small (same result, narrow blocks run wide)  all nine, by the geometry assertion        before: no
  PzRawBias off by one on the extension path                            all nine                                   before: yes
  halves of the uint16 pair load swapped                                all nine (rows 2 bytes off a dword)        before: no
"""
import time

import pytest

from tests import raw_matrix as rm
from tests.emul import emul

ROWS = rm.MATRIX_ROWS
CASES = rm.raw_cases()


def test_every_raw_factor_has_a_matrix_row():
    """a factor added to TDM_PZR_CASES without a rate and a bound here fails"""
    assert len(CASES) >= 9, CASES
    assert set(CASES) == set(rm.RATE_OF_Q), "a raw-byte instantiation without a sample rate in tests/raw_matrix.py"
    assert set(CASES) == set(rm.RAW_SOFT_WORST), "a raw-byte instantiation without an entry in RAW_SOFT_WORST"
    for q, S in CASES.items():
        assert int(rm.RATE_OF_Q[q] / 240000.0) == q
        assert (q * S) % 2 == 0


@pytest.mark.parametrize("q", sorted(CASES))
def test_raw_matrix_emulated(q):
    S, rate = CASES[q], rm.RATE_OF_Q[q]
    worst = {"strict": (0.0, None), "pattern": (0.0, None)}
    seen_strides, seen_classes = set(), set()
    t0 = time.time()
    for c in rm.matrix_cases(q):
        n, stride, base = c["n"], c["stride"], c["base"]
        engine, g = emul.dec_engine(rate, n, "cu8", ROWS)
        assert engine == 3, (c["where"], engine)
        mine = rm.geometry(q * S, n)
        assert (g["L"], g["nb"], g["b_tail"]) == (mine["L"], mine["nb"], mine["b_tail"]), (g, mine)
        rm.check_class(c["cname"], mine)
        seen_strides.add(c["skind"])
        seen_classes.add(c["cname"])
        hard, soft, n_soft, bp, mm = emul.process(rate, c["buf"][2 * base:], "cu8", n, rows=ROWS, stride=stride, freq_offset=c["foffs"])
        for r in range(ROWS):
            ns = int(n_soft[r])
            ref = rm.oracle_row(rate, rm.row_bytes(c["buf"], n, stride, base, r), c["foffs"][r])
            where = f"{c['where']} row={r} {c['kinds'][r]}"
            e = rm.check_row(c["kinds"][r], hard[r, :max(ns - 1, 0)], soft[r, :ns], int(bp[r]), ref, where)
            grp = "strict" if c["kinds"][r] in rm.STRICT_KINDS else "pattern"
            if e > worst[grp][0]:
                worst[grp] = (e, where)
    assert seen_strides == set(rm.MATRIX_STRIDES) and seen_classes == set(rm.LENGTH_CLASSES)
    w = max(worst["strict"][0], worst["pattern"][0])
    print(f"\nRAW_MATRIX_CPU q={q} worst {w:.2e}  strict {worst['strict'][0]:.2e} [{worst['strict'][1]}]  "
          f"pattern {worst['pattern'][0]:.2e} [{worst['pattern'][1]}]  ({time.time() - t0:.1f} s)")
    assert w <= rm.SOFT_TOL
    assert w <= rm.RAW_SOFT_WORST[q], f"q={q}: {w:.3e} above the table's {rm.RAW_SOFT_WORST[q]:.3e}"
    assert w >= rm.RAW_SOFT_WORST[q] / 10, f"q={q}: {w:.3e} below a tenth of the table's {rm.RAW_SOFT_WORST[q]:.3e}: renew the entry"
