"""GPU: k_pz_raw with the negligible scan terms compiled out (tdm_debug_set "scan_prune" 1, the default; pz_tables.hpp
PzScanKeep) against the same kernel with every term ("scan_prune" 0, the plan made after the switch) and against the oracle.

Factors q = 10 (block B = 64 x 120 = 7680 samples) and q = 3 (B = 3072: a table that drops the most terms); lengths 3B - 5
(wide first block, narrow middle, wide tail) and 5B + 7; six rows a call, the rows of tests/test_scan_prune_cpu.py: noise,
random 0x00 / 0xFF bytes, all-0x00, the Nyquist alternation, two blocks of 0x00 followed by 0xFF to the end and the same
reversed.
  * pruned against every term: hard symbols, soft symbols, n_soft and best_phase np.array_equal;
  * pruned against the oracle: tests/raw_matrix.py check_row per row, the worst soft error within the bound
    tests/test_raw_matrix_gpu.py holds that factor to (GPU_MARGIN x RAW_SOFT_WORST[q], and SOFT_TOL).  The two step rows
    are held the way the Nyquist row is: index by index, count and timing phase equal, soft error against the input's
    full scale 1.0 (their max|soft| is 1.41, so that is the stricter figure), hard symbols equal wherever the oracle's
    decision is defined.
"""
import numpy as np
import pytest

from tests import raw_matrix as rm
from tests.test_scan_prune_cpu import CASES, ROW_KINDS, row_offsets, six_rows

pytestmark = pytest.mark.gpu


def _run(q, n, u8, foffs, prune):
    from tetraear_amd._lib import debug_option
    from tetraear_amd.batch import BatchDemodulator
    with debug_option("scan_prune", prune), debug_option("raw_min_blocks", 0):
        bd = BatchDemodulator(rm.RATE_OF_Q[q], n, len(ROW_KINDS), "cu8")
    try:
        assert bd.info.dec_engine == 3, (q, n, "the plan did not take the raw-byte decimator")
        bd.alloc_device_io()
        bd.upload(u8, freq_offsets=foffs)
        bd.enqueue()
        hard, soft, n_soft, bp, mm = bd.download()
    finally:
        bd.sync()
        bd.close()
    return hard, soft, n_soft, bp


@pytest.mark.parametrize("q,cname", [(10, "3B-5"), (10, "5B+7"), (3, "3B-5"), (3, "5B+7")])
def test_pruned_scans_on_device(q, cname):
    n = rm.class_lengths(q, CASES[q])[cname]
    rm.check_class(cname, rm.geometry(q * CASES[q], n))
    u8 = six_rows(q, n, seed=7000 + q)
    foffs = row_offsets(q)
    pruned = _run(q, n, u8, foffs, 1)
    every = _run(q, n, u8, foffs, 0)
    hard, soft, n_soft, bp = pruned
    where = f"q={q} {cname} n={n}: %s of the pruned scans differs from the scans with every term"
    assert np.array_equal(n_soft, every[2]), where % "n_soft"
    assert np.array_equal(bp, every[3]), where % "best_phase"
    assert np.all(n_soft >= 2)
    for r in range(len(ROW_KINDS)):   # (what a call writes of a row: n_soft soft symbols, one decision fewer)
        ns = int(n_soft[r])
        assert np.array_equal(hard[r, :ns - 1], every[0][r, :ns - 1]), where % f"row {r}: hard"
        assert np.array_equal(soft[r, :ns].view(np.float64), every[1][r, :ns].view(np.float64)), where % f"row {r}: soft"
    worst = (0.0, None)
    for r, kind in enumerate(ROW_KINDS):
        ref = rm.oracle_row(rm.RATE_OF_Q[q], rm.row_bytes(u8, n, n, 0, r), foffs[r])
        ns = int(n_soft[r])
        where = f"q={q} {cname} n={n} row={r} {kind}"
        e = rm.check_row(kind if kind in rm.KINDS else "s00ff", hard[r, :max(ns - 1, 0)], soft[r, :ns], int(bp[r]), ref, where)
        print(f"\nSCAN_PRUNE_GPU {where}: soft error {e:.2e}")
        worst = max(worst, (e, where), key=lambda t: t[0])
    print(f"\nSCAN_PRUNE_GPU q={q} {cname} worst {worst[0]:.2e} [{worst[1]}]  table {rm.RAW_SOFT_WORST[q]:.2e}")
    assert worst[0] <= rm.SOFT_TOL, worst
    assert worst[0] <= rm.GPU_MARGIN * rm.RAW_SOFT_WORST[q], (worst, rm.RAW_SOFT_WORST[q])
