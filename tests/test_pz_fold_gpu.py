"""GPU: the raw-byte decimator's interior blocks in the folded block-sum form (tdm_debug_set "raw_fold" 1, the default)
against the per-sample form of the same kernel ("raw_fold" 0) on 64 carriers x 262 144 samples, and both against the CPU
oracle on 8 of the rows.  Equal decisions, counts and timing phases; soft symbols within the parity tests' tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SOFT_TOL = 1e-10   # tests/test_gpu_parity.py
ROWS, N = 64, 262144
ORACLE_ROWS = (0, 7, 13, 22, 31, 40, 52, 63)


def _run(u8, foffs, fold):
    from tetraear_amd._lib import debug_option
    from tetraear_amd.batch import BatchDemodulator
    with debug_option("raw_fold", fold), debug_option("raw_min_blocks", 0):
        bd = BatchDemodulator(2.4e6, N, ROWS, "cu8")
    try:
        assert bd.info.dec_engine == 3, "the batch did not take the raw-byte decimator"
        return bd.process(u8, freq_offsets=foffs)
    finally:
        bd.close()


def test_raw_fold_on_off_and_oracle():
    from oracle.oracle import OracleSignalProcessor
    from tetraear_amd import synth
    u8 = synth.dqpsk_cu8_streams(N, 2.4e6, [4100 + r for r in range(ROWS)]).reshape(-1)
    foffs = [((r % 7) - 3) * 390.625 for r in range(ROWS)]
    hard1, soft1, bp1, mm1 = _run(u8, foffs, 1)
    hard0, soft0, bp0, mm0 = _run(u8, foffs, 0)
    worst = 0.0
    for r in range(ROWS):
        assert len(soft1[r]) == len(soft0[r]) and len(soft1[r]) > 1000, r
        np.testing.assert_array_equal(hard1[r], hard0[r])
        assert bp1[r] == bp0[r], r
        worst = max(worst, np.max(np.abs(soft1[r] - soft0[r])) / np.max(np.abs(soft0[r])))
    print(f"folded against per-sample: worst soft difference {worst:.3e} of max|soft|")
    assert worst <= SOFT_TOL
    assert worst > 0.0, "both settings gave the same bits: the plan ignored the raw_fold switch"
    for name, hards, softs, bps in (("folded", hard1, soft1, bp1), ("per-sample", hard0, soft0, bp0)):
        worst = 0.0
        for r in ORACLE_ROWS:
            o = OracleSignalProcessor(2.4e6)
            ref = o.process(synth.cu8_to_c128(u8[2 * N * r: 2 * N * (r + 1)]), foffs[r])
            assert len(softs[r]) == len(o.symbols), (name, r)
            assert bps[r] == o.best_phase, (name, r)
            np.testing.assert_array_equal(hards[r], ref)
            worst = max(worst, np.max(np.abs(softs[r] - o.symbols)) / np.max(np.abs(o.symbols)))
        print(f"{name} against the oracle: worst soft error {worst:.3e} of max|soft|")
        assert worst <= SOFT_TOL, name
