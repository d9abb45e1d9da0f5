"""Shared by tests/test_raw_edge_fill_cpu.py, tests/test_raw_edge_fill_gpu.py and tests/golden/make_golden_raw_edge.py: the
calls that pin what the raw-byte decimator's WIDE blocks (block 0 and the blocks from b_tail on, pz_raw_body<..., true>)
hand their edge lanes -- the lanes holding the odd extension at either end of a row and the zero pad behind it.

Per factor: three calls of tests/raw_matrix.matrix_cases (six rows each, the matrix's own strides and base offsets) and one
added call on a row that fits ONE block, which is then both the first and the tail block:
  B+1        the signal ends one sample into block 1: the tail block is two edge lanes and 62 lanes of zeros
  3B+L+1     the tail extension starts in lane 1 of the tail block, behind an interior lane
  two_tail   the tail extension crosses a block boundary: two tail blocks, each filling the slots of its own lanes only
  nb1        n = B - P0 - 2 * 27 - L + 10: lanes 62 and 63 of block 0 hold the tail extension (the last ten extended
             samples in lane 63, zeros behind them), lane 0 holds the head extension
Every stride kind of the matrix comes up over the nine factors; the added call runs on the odd pitch n + 1 or n + 2 from a
base of one sample, so that every second row starts 2 bytes off a dword.
"""
import hashlib

import numpy as np

from tests import raw_matrix as rm

MATRIX_CLASSES = ("B+1", "3B+L+1", "two_tail")
ROWS = rm.MATRIX_ROWS


def nb1_length(q, S):
    L = q * S
    P0 = (L - rm.EDGE % L) % L
    return 64 * L - P0 - 2 * rm.EDGE - L + 10


def cases(q):
    """dicts as tests/raw_matrix.matrix_cases yields them: cname, n, stride, base, buf, kinds, foffs, where"""
    for c in rm.matrix_cases(q):
        if c["cname"] in MATRIX_CLASSES:
            yield c
    S = rm.raw_cases()[q]
    n = nb1_length(q, S)
    g = rm.geometry(q * S, n)
    assert (g["nb"], g["b_tail"], g["narrow"], g["tail"]) == (1, 0, 0, 1), g
    stride = n + 1 + (n % 2)          # odd
    base = 1
    kinds = tuple(rm.KINDS[(k + q) % 6] for k in range(6))
    buf, rkinds = rm.layout(ROWS, n, stride, base, kinds, seed=7000 + q)
    foffs = [rm.row_offset(rkinds[r], r + q, rm.RATE_OF_Q[q] / q) for r in range(ROWS)]
    yield dict(cname="nb1", n=n, skind="odd", stride=stride, base=base, buf=buf, kinds=rkinds, foffs=foffs,
               where=f"q={q} nb1 n={n} stride=odd({stride}) base={base}")


def key(q, cname):
    return f"q{q}_{cname.replace('+', 'p').replace('-', 'm').replace('/', 'd')}"


def digest(hard, soft, n_soft, best_phase):
    """SHA-256 over the bytes of the four outputs of one call, as 32 uint8"""
    h = hashlib.sha256()
    for a, dt in ((soft, np.complex128), (hard, np.uint8), (n_soft, np.int32), (best_phase, np.int32)):
        a = np.ascontiguousarray(a)
        assert a.dtype == dt, (a.dtype, dt)
        h.update(a.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def emulate(q, c):
    """(hard, soft, n_soft, best_phase) of the CPU lock-step emulation for one case"""
    from tests.emul import emul
    rate = rm.RATE_OF_Q[q]
    engine, g = emul.dec_engine(rate, c["n"], "cu8", ROWS)
    assert engine == 3, (c["where"], engine)
    hard, soft, n_soft, bp, mm = emul.process(rate, c["buf"][2 * c["base"]:], "cu8", c["n"], rows=ROWS, stride=c["stride"],
                                              freq_offset=c["foffs"])
    return hard, soft, n_soft, bp
