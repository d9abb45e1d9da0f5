"""CPU: the raw-byte decimator's wide blocks hand their edge lanes the same integers as before the whole wavefront filled
them (pz_raw_fill_edges: every lane builds a share of the head extension 2 u[0] - u[27 - e], the row's last samples, the tail
extension 2 u[n-1] - u[n-2-k] and the zeros behind it; the edge lanes then read their L dwords).

The integers are unchanged, so every output is: tests/golden/raw_edge_bits.npz holds the SHA-256 of the emulation's soft /
hard / n_soft / best_phase bytes from the commit before the change (tests/golden/make_golden_raw_edge.py), for the calls of
tests/raw_edge_cases.py at every factor -- three calls of the raw matrix (among them two tail blocks) and a row that fits
one block, which is first and tail block at once.  The emulation runs what ships (a zeroed ZpParams::raw_edge_loop), the
fixture is the rolled loop's.  Equal digests, nothing less: a tolerance would admit a changed extension sample, which moves
a soft symbol by 1e-6 (tests/test_raw_matrix_cpu.py: PzRawBias off by one)."""
import os

import numpy as np
import pytest

from tests import raw_edge_cases as rec
from tests import raw_matrix as rm

CASES = rm.raw_cases()
_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raw_edge_bits.npz")


def test_fixture_covers_every_factor_and_call():
    gold = np.load(_GOLD)
    want = {rec.key(q, c) for q in CASES for c in rec.MATRIX_CLASSES + ("nb1",)}
    assert set(gold.files) == want, set(gold.files) ^ want
    assert len(CASES) >= 9


@pytest.mark.parametrize("q", sorted(CASES))
def test_edge_fill_keeps_every_bit(q):
    gold = np.load(_GOLD)
    seen = []
    for c in rec.cases(q):
        hard, soft, n_soft, bp = rec.emulate(q, c)
        got = rec.digest(hard, soft, n_soft, bp)
        assert int(n_soft.min()) >= 2, c["where"]
        assert np.array_equal(got, gold[rec.key(q, c["cname"])]), f"{c['where']}: the emulation's output bytes differ from the fixture's"
        seen.append(c["cname"])
    assert seen == list(rec.MATRIX_CLASSES) + ["nb1"], seen
