"""GPU: k_pz_raw at every factor it is instantiated for, in launches of several rows, against the oracle run on exactly the
bytes each row was given (the device half of tests/test_raw_matrix_cpu.py; shapes, row kinds and comparisons are those of
tests/raw_matrix.py).

What reached the raw-byte kernel with more than one row before this file: 2.4 MS/s (q = 10), 262 144 samples, even stride,
dword-aligned rows -- test_c4_full_batch_every_carrier_vs_oracle (1024 rows), test_pz_fold_gpu.py (64), and, by their size
alone (rows x blocks >= 8 per CU), the 64 x 262 144 plans of test_pipelined_batch.py and the 256 x 262 144 stream of
test_stream_gpu.py; the other host-fed and stream tests (5 or 9 rows of 46 157 / 65 536) stay on the double-based kernel.
Every other factor had only ever run row 0 (the cu8_engine="raw" cases of test_gpu_parity.py).  No case here has that
shape.

  a. test_raw_matrix_on_device: per factor, every length class, six rows a launch (one of each row kind): first the CPU
     matrix's own eight calls byte for byte (raw_matrix.matrix_cases) through the device-pointer entry, then the host entry
     (BatchDemodulator.process, stride n) at the class lengths -- seven odd, one even -- and at two more even ones; the
     device-pointer entry (alloc_device_io / upload / enqueue(iq_ptr=, stride=)) with odd and even pitched strides, stride
     0 and the stride n, the base pointer 0, 1 or 3 whole samples into a larger allocation: with an even stride and an odd
     offset every row, row 0 included, starts 2 bytes off a dword (the uint16 pair loads in the wide and in the narrow
     body), with an odd stride every second row does.  Every buffer ends with the last row's last byte.
  b. the six byte patterns are rows of every launch of (a); q = 10 runs the matrix under both raw_fold settings.
  c. test_default_threshold: no raw_min_blocks switch -- the row count at which a batch of an odd length at q = 8 crosses
     8 blocks per CU by itself reports engine 3, one row less engine 2; 16 rows of each are held to the oracle.
  d. test_resize_under_the_raw_engine: one plan of 5 rows walked through lengths with and without narrow blocks, with one
     and two tail blocks, shorter and longer than it was made for, and back.
  e. two of the shapes per factor are run again on the same plan and buffers: bit-identical.
  f. test_dec_engine_of_time_batched_plans: a plan with rows_per_chunk > 1 reports engine 2, without the option 3.

Bound per factor: GPU_MARGIN (8) x RAW_SOFT_WORST[q], and the project's 1e-10.
Figures on an MI355X at the commit that added the file (worst soft error per factor over (a), fraction of max|soft|):
  factor              3        4        6        7        8        10       12       13       41
  whole of (a)        6.5e-13  2.0e-13  2.3e-13  1.6e-13  1.7e-13  2.8e-13  3.3e-13  3.8e-13  8.9e-12
  CPU matrix's calls  6.5e-13  1.6e-13  2.3e-13  1.4e-13  1.6e-13  2.8e-13  2.7e-13  1.3e-13  4.0e-12
  RAW_SOFT_WORST      6.2e-13  1.6e-13  2.1e-13  1.6e-13  1.5e-13  2.6e-13  3.2e-13  1.4e-13  3.8e-12
q = 10 with raw_fold 0: 2.8e-13 (the same row).  On the CPU matrix's own bytes the device is within 1.1 x the emulation at
every factor: contraction and summation order cost next to nothing, the margin of 8 is spent on OTHER inputs -- the largest
ratio to the table is 2.7 at q = 13 (3B+L+1, even pitched stride, base + 1 sample, row 1, noise) and 2.4 at q = 41 (2B+3,
even pitched stride, base + 3, row 3, noise), which is the spread of the oracle's own rounding from row to row (the
emulation on those same extra rows gives 2.1 x and 1.4 x the table at q = 13 and 41).  Resize walks: 1.5e-13 (q = 12),
4.0e-12 (q = 41).  Threshold, q = 8, 65 537 samples, 256 CUs: 63 rows engine 3 (1.7e-13), 62 rows engine 2 (1.3e-13).
"""
import ctypes as C

import numpy as np
import pytest

from tests import raw_matrix as rm

pytestmark = pytest.mark.gpu

ROWS = 6
CASES = rm.raw_cases()
# (stride kind, base offset in samples) of the device-pointer launches; each length class takes two, moving with the factor
DEVICE_LAYOUTS = (("pitch_odd", 0), ("pitch_even", 1), ("zero", 3), ("n", 1), ("pitch_odd", 3), ("pitch_even", 3), ("zero", 0))


def _stride(kind, n):
    odd = n + 4 + (n % 2 == 0)
    return {"n": n, "pitch_odd": odd, "pitch_even": odd + 3, "zero": 0}[kind]


def _kinds(ci, stride):
    return tuple(rm.KINDS[(k + ci) % 6] for k in range(6)) if stride else (rm.STRICT_KINDS[ci % 2],)


def _plan(rate, n, rows, fold=1):
    from tetraear_amd._lib import debug_option
    from tetraear_amd.batch import BatchDemodulator
    with debug_option("raw_fold", fold), debug_option("raw_min_blocks", 0):
        bd = BatchDemodulator(rate, n, rows, "cu8")
    assert bd.info.dec_engine == 3, (rate, n, rows, "the plan did not take the raw-byte decimator")
    return bd


def _check_rows(rate, buf, n, stride, base, rkinds, foffs, got, where, rows=None):
    """got = (hards, softs, bp) as lists per row; returns the worst soft error"""
    hards, softs, bp = got
    worst = (0.0, None)
    for r in (range(len(rkinds)) if rows is None else rows):
        ref = rm.oracle_row(rate, rm.row_bytes(buf, n, stride, base, r), foffs[r])
        w = f"{where} row={r} {rkinds[r]}"
        e = rm.check_row(rkinds[r], hards[r], softs[r], int(bp[r]), ref, w)
        if e > worst[0]:
            worst = (e, w)
    return worst


def _host_call(bd, buf, foffs):
    hards, softs, bp, mm = bd.process(buf, freq_offsets=foffs)
    return hards, softs, bp


def _device_call(bd, dbuf, buf, n, stride, base, foffs, again=False):
    """the rows of `buf` (uploaded to dbuf, a DeviceBuffer of exactly len(buf) bytes) through the device-pointer entry"""
    assert 2 * (base + (bd.n_carriers - 1) * stride + n) == len(buf) == dbuf.nbytes, "the last row must end with the allocation"
    if not again:
        dbuf.upload(buf)
        bd.upload(buf[:2 * n], freq_offsets=foffs)    # (the plan's own input buffer is not the one read)
    bd.enqueue(iq_ptr=C.c_void_p(dbuf.ptr.value + 2 * base), stride=stride)
    hard, soft, n_soft, bp, mm = bd.download()
    hards = [hard[r, :max(int(n_soft[r]) - 1, 0)].copy() for r in range(bd.n_carriers)]
    softs = [soft[r, :int(n_soft[r])].copy() for r in range(bd.n_carriers)]
    return hards, softs, bp


def _same(a, b, where):
    for r in range(len(a[0])):
        np.testing.assert_array_equal(a[0][r], b[0][r], err_msg=f"{where}: hard symbols of row {r} on the second call")
        assert np.array_equal(a[1][r].view(np.float64), b[1][r].view(np.float64)), f"{where}: soft symbols of row {r} on the second call"
    np.testing.assert_array_equal(a[2], b[2])


def _compute_units():
    """compute units of the (first) GPU, from the driver's own listing and not from the library under test: rocminfo's first
    GPU agent, else the KFD topology (SIMDs over SIMDs per CU of the first node that has any)"""
    import glob
    import re
    import shutil
    import subprocess
    exe = shutil.which("rocminfo") or "/opt/rocm/bin/rocminfo"
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError):
        out = ""
    for agent in re.split(r"\n\*+\s*\nAgent \d+", out)[1:]:
        m = re.search(r"Compute Unit:\s+(\d+)", agent)
        if re.search(r"Device Type:\s+GPU", agent) and m:
            return int(m.group(1))
    for path in sorted(glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"), key=lambda p: int(p.split("/")[-2])):
        with open(path) as f:
            props = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
        if int(props.get("simd_count", 0)) > 0 and int(props.get("simd_per_cu", 0)) > 0:
            return int(props["simd_count"]) // int(props["simd_per_cu"])
    raise RuntimeError("no GPU agent in rocminfo's output or the KFD topology")


def _matrix(q, fold):
    from tetraear_amd.batch import DeviceBuffer
    S, rate = CASES[q], rm.RATE_OF_Q[q]
    fi = sorted(CASES).index(q)
    L, B = q * S, 64 * q * S
    lengths = [(c, n) for c, n in rm.class_lengths(q, S).items()]
    lengths += [("2B+4 (even)", 2 * B + 4), ("3B+L+2 (even)", 3 * B + L + 2)]
    worst = (0.0, None)
    # ---- the CPU matrix's own calls, byte for byte, through the device-pointer entry: the device against the emulation's
    # figure on the same rows
    for c in rm.matrix_cases(q):
        n, stride, base = c["n"], c["stride"], c["base"]
        bd = _plan(rate, n, ROWS, fold)
        dbuf = DeviceBuffer(bd.device, len(c["buf"]))
        try:
            bd.alloc_device_io()
            got = _device_call(bd, dbuf, c["buf"], n, stride, base, c["foffs"])
            w = _check_rows(rate, c["buf"], n, stride, base, c["kinds"], c["foffs"], got, f"fold={fold} {c['where']} device")
            worst = max(worst, w, key=lambda t: t[0])
        finally:
            bd.sync()
            dbuf.free()
            bd.close()
    shared = worst
    # ---- more of the same classes: the host entry at every length, other strides and offsets
    seen = set()
    for ci, (cname, n) in enumerate(lengths):
        g = rm.geometry(L, n)
        if cname in rm.LENGTH_CLASSES:
            rm.check_class(cname, g)
        bd = _plan(rate, n, ROWS, fold)
        try:
            assert (bd.info.q, bd.info.n_samples) == (q, n)
            # ---- host entry, stride n
            buf, rkinds = rm.layout(ROWS, n, n, 0, _kinds(ci, n), seed=2000 * q + ci)
            foffs = [rm.row_offset(rkinds[r], r + ci, rate / q) for r in range(ROWS)]
            where = f"q={q} fold={fold} {cname} n={n} host"
            got = _host_call(bd, buf, foffs)
            w = _check_rows(rate, buf, n, n, 0, rkinds, foffs, got, where)
            worst = max(worst, w, key=lambda t: t[0])
            if ci == 2:
                _same(got, _host_call(bd, buf, foffs), where)
            # ---- device-pointer entry
            if cname not in rm.LENGTH_CLASSES:
                continue
            bd.alloc_device_io()
            for k in range(2):
                skind, base = DEVICE_LAYOUTS[(2 * ci + k + fi) % len(DEVICE_LAYOUTS)]
                seen.add((skind, base))
                stride = _stride(skind, n)
                buf, rkinds = rm.layout(ROWS, n, stride, base, _kinds(ci + k + 1, stride), seed=3000 * q + 2 * ci + k)
                foffs = [rm.row_offset(rkinds[r], r + ci + k, rate / q) for r in range(ROWS)]
                where = f"q={q} fold={fold} {cname} n={n} device stride={skind}({stride}) base={base}"
                dbuf = DeviceBuffer(bd.device, len(buf))
                try:
                    got = _device_call(bd, dbuf, buf, n, stride, base, foffs)
                    w = _check_rows(rate, buf, n, stride, base, rkinds, foffs, got, where)
                    worst = max(worst, w, key=lambda t: t[0])
                    if ci == 4 and k == 0:
                        _same(got, _device_call(bd, dbuf, buf, n, stride, base, foffs, again=True), where)
                finally:
                    bd.sync()
                    dbuf.free()
        finally:
            bd.close()
    assert seen == set(DEVICE_LAYOUTS), seen
    print(f"\nRAW_MATRIX_GPU q={q} fold={fold} worst {worst[0]:.2e} [{worst[1]}]  on the CPU matrix's own calls {shared[0]:.2e} "
          f"[{shared[1]}]  table {rm.RAW_SOFT_WORST[q]:.2e}  ratio {worst[0] / rm.RAW_SOFT_WORST[q]:.2f}")
    assert worst[0] <= rm.SOFT_TOL, worst
    assert worst[0] <= rm.GPU_MARGIN * rm.RAW_SOFT_WORST[q], (worst, rm.RAW_SOFT_WORST[q])


@pytest.mark.parametrize("q", sorted(CASES))
def test_raw_matrix_on_device(q):
    _matrix(q, 1)


def test_raw_matrix_on_device_per_sample_form():
    """q = 10 with the narrow blocks sample by sample (raw_fold 0, the folded form's A/B partner): the same matrix"""
    _matrix(10, 0)


def test_default_threshold():
    """Without the raw_min_blocks switch: the plan takes the raw-byte kernel from rows x blocks >= 8 per CU on (blocks: the
    double-based decimator's, lanes of Q x S(TDM_PZ_CASES) samples -- tdm_plan_create)."""
    from tetraear_amd.batch import BatchDemodulator
    q, n = 8, 65537
    rate = rm.RATE_OF_Q[q]
    cus = _compute_units()
    nb = rm.geometry(q * rm.pz_cases()[q], n)["nb"]
    rows_raw = -(-8 * cus // nb)
    assert rows_raw >= 17 and (rows_raw - 1) * nb < 8 * cus <= rows_raw * nb
    for rows, engine in ((rows_raw, 3), (rows_raw - 1, 2)):
        bd = BatchDemodulator(rate, n, rows, "cu8")
        try:
            assert (bd.info.q, bd.info.n_samples, bd.info.n_carriers) == (q, n, rows)
            assert bd.info.dec_engine == engine, (rows, nb, cus, bd.info.dec_engine)
            kinds = ("noise", "rand0255", "noise", "s00ff", "rand0255", "bff", "noise")
            buf, rkinds = rm.layout(rows, n, n, 0, kinds, seed=8000 + rows)
            foffs = [rm.row_offset(rkinds[r], r, rate / q) for r in range(rows)]
            got = _host_call(bd, buf, foffs)
            sample = sorted(set(range(0, rows, max(rows // 8, 1))[:8]) | set(range(1, rows, max(rows // 7, 1))[:7]) | {0, 1, rows - 2, rows - 1})
            assert len(sample) >= 16 and any(r % 2 for r in sample) and any(r % 2 == 0 for r in sample)
            w = _check_rows(rate, buf, n, n, 0, rkinds, foffs, got, f"q={q} n={n} rows={rows} engine={engine}", rows=sample)
            print(f"\nRAW_MATRIX_GPU threshold rows={rows} engine={engine} ({cus} CUs, {nb} blocks a row) worst {w[0]:.2e} [{w[1]}]")
            assert w[0] <= rm.SOFT_TOL
            if engine == 3:
                assert w[0] <= rm.GPU_MARGIN * rm.RAW_SOFT_WORST[q], w
        finally:
            bd.close()


@pytest.mark.parametrize("q", [12, 41])
def test_resize_under_the_raw_engine(q):
    S, rate, rows = CASES[q], rm.RATE_OF_Q[q], 5
    ln = rm.class_lengths(q, S)
    walk = ["3B+L+1", "B-1", "two_tail", "5B+7", "B/2+1", "3B+L+1", "2B+3", "two_tail", "B-1", "5B+7"]
    g = [rm.geometry(q * S, ln[c]) for c in walk]
    assert {x["tail"] for x in g} == {1, 2} and any(x["narrow"] == 0 for x in g) and any(x["narrow"] >= 2 for x in g)
    assert min(ln[c] for c in walk) < ln[walk[0]] < max(ln[c] for c in walk)
    bd = _plan(rate, ln[walk[0]], rows)
    worst = (0.0, None)
    try:
        for step, cname in enumerate(walk):
            n = ln[cname]
            bd.resize(n)
            assert bd.info.n_samples == n and bd.info.dec_engine == 3, (cname, bd.info.dec_engine)
            buf, rkinds = rm.layout(rows, n, n, 0, _kinds(step, n), seed=5000 * q + step)
            foffs = [rm.row_offset(rkinds[r], r + step, rate / q) for r in range(rows)]
            got = _host_call(bd, buf, foffs)
            w = _check_rows(rate, buf, n, n, 0, rkinds, foffs, got, f"q={q} resize step {step} {cname} n={n}")
            worst = max(worst, w, key=lambda t: t[0])
    finally:
        bd.close()
    print(f"\nRAW_MATRIX_GPU resize q={q} worst {worst[0]:.2e} [{worst[1]}]")
    assert worst[0] <= rm.SOFT_TOL
    assert worst[0] <= rm.GPU_MARGIN * rm.RAW_SOFT_WORST[q], worst


def test_dec_engine_of_time_batched_plans():
    """a plan whose rows share input rows (rows_per_chunk > 1) never takes the raw-byte kernel (run_ref_fmt), and says so"""
    n, rows = 23161, 6
    bd = _plan(2.4e6, n, rows)
    try:
        bd.set_rows_per_chunk(2)
        assert bd.info.dec_engine == 2
        bd.set_rows_per_chunk(1)
        assert bd.info.dec_engine == 3
    finally:
        bd.close()
