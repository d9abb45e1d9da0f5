"""Fixture of tests/test_raw_edge_fill_cpu.py: per decimation factor of the raw-byte decimator and per call of
tests/raw_edge_cases.cases(q), the SHA-256 of the CPU emulation's soft / hard / n_soft / best_phase bytes.

Written at the commit BEFORE the wide blocks' edge lanes were filled by the whole wavefront, i.e. by the emulation of the
per-lane rolled loop: the test holds the new fill to the same bits.  It is renewed only by a change that means to move the
decimator's output, and then from a tree whose tests/test_raw_matrix_cpu.py passes.
CPU only:  python tests/golden/make_golden_raw_edge.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from tests import raw_edge_cases as rec   # noqa: E402
from tests import raw_matrix as rm        # noqa: E402

out = {}
for q in sorted(rm.raw_cases()):
    for c in rec.cases(q):
        hard, soft, n_soft, bp = rec.emulate(q, c)
        assert int(n_soft.min()) >= 2, c["where"]
        out[rec.key(q, c["cname"])] = rec.digest(hard, soft, n_soft, bp)
        print(c["where"], "symbols", n_soft.tolist(), out[rec.key(q, c["cname"])].tobytes().hex()[:16], flush=True)
np.savez(os.path.join(HERE, "raw_edge_bits.npz"), **out)
print("written:", len(out), "digests")
