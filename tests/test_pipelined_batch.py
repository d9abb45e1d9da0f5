"""PipelinedBatchDemodulator (tetraear_amd/batch.py): plans of the same batch geometry taking the steps in turn -- each plan's
outputs are a lone plan's bit for bit, chunk k can be fed to plan k % depth, per-stage timing orders the steps on the device
(tdm_plan_wait_for)."""
import numpy as np
import pytest


def _valid_equal(a, b):
    """outputs (hard, soft, n_soft, best_phase, min_margin) equal over their valid parts"""
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[3], b[3])
    np.testing.assert_array_equal(a[4], b[4])
    for r in range(len(a[2])):
        k = int(a[2][r])
        np.testing.assert_array_equal(a[0][r, :max(k - 1, 0)], b[0][r, :max(k - 1, 0)])
        np.testing.assert_array_equal(a[1][r, :k], b[1][r, :k])


@pytest.mark.gpu
def test_pipelined_plans_equal_a_lone_plan_and_take_chunks_in_turn():
    from tetraear_amd import synth
    from tetraear_amd.batch import BatchDemodulator, PipelinedBatchDemodulator, batch_demodulator
    n, rows = 65536, 9
    chunks = [np.concatenate([synth.noise_cu8(n, 8100 + 50 * c + r) for r in range(rows)]) for c in range(5)]
    foffs = np.linspace(-3000.0, 3000.0, rows)
    one = BatchDemodulator(2.4e6, n, rows, "cu8")
    one.alloc_device_io()
    refs = []
    for u8 in chunks:
        one.upload(u8, freq_offsets=foffs)
        one.enqueue()
        refs.append(one.download())
    one.close()
    for depth in (2, 3):
        pl = PipelinedBatchDemodulator(2.4e6, n, rows, "cu8", depth=depth)
        assert pl.depth == depth
        pl.alloc_device_io()
        # one resident batch, many steps: every plan ends with the lone plan's outputs
        pl.upload(chunks[0], freq_offsets=foffs)
        for _ in range(2 * depth + 1):
            pl.enqueue()
        for o in pl.download_all():
            _valid_equal(refs[0], o)
        _valid_equal(refs[0], pl.download())
        # a capture loop: chunk k to plan k % depth, `depth` chunks in flight, outputs collected a round later
        got = {}
        for k, u8 in enumerate(chunks):
            if k >= depth:
                got[k - depth] = pl.download(slot=k)     # (the plan about to be reused: its previous chunk's outputs)
            pl.upload(u8, freq_offsets=foffs, slot=k)
            pl.enqueue(slot=k)
        for k in range(len(chunks) - depth, len(chunks)):
            got[k] = pl.download(slot=k)
        for k in range(len(chunks)):
            _valid_equal(refs[k], got[k])
        # the per-stage pass: steps one after the other on the device, same outputs
        pl.upload(chunks[1], freq_offsets=foffs)
        pl.time_begin(per_stage=True)
        for _ in range(depth):
            pl.enqueue()
        ms = pl.time_end()
        st = pl.stage_times()
        assert ms > 0 and st["dec_block"] > 0
        for o in pl.download_all():
            _valid_equal(refs[1], o)
        pl.close()
    assert isinstance(batch_demodulator(2.4e6, n, 4, "cu8", depth=1), BatchDemodulator)
    auto = batch_demodulator(2.4e6, n, 4, "cu8")
    assert isinstance(auto, PipelinedBatchDemodulator) and auto.depth == 3
    auto.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_capture_loop_recipe_vs_a_lone_plan_and_the_oracle(depth):
    """The class docstring's capture loop, literally and through public calls only: 12 distinct chunks of 9 rows x 65536 cu8
    samples, chunk k uploaded to and enqueued on slot k, collected with download(slot=k) one round later, while `depth`
    steps are in flight.  Every chunk's valid outputs equal a lone plan's bit for bit, every fourth chunk's the oracle's."""
    from oracle.oracle import OracleSignalProcessor
    from tetraear_amd import synth
    from tetraear_amd.batch import BatchDemodulator, PipelinedBatchDemodulator
    n, rows, n_chunks = 65536, 9, 12
    chunks = [np.concatenate([synth.noise_cu8(n, 8400 + 20 * c + r) for r in range(rows)]) for c in range(n_chunks)]
    f = np.linspace(-2900.0, 3100.0, rows)
    one = BatchDemodulator(2.4e6, n, rows, "cu8")
    one.alloc_device_io()
    refs = []
    for u8 in chunks:
        one.upload(u8, freq_offsets=f)
        one.enqueue()
        refs.append(one.download())
    one.close()
    outs = {}
    pl = PipelinedBatchDemodulator(2.4e6, n, rows, "cu8", depth=depth)
    pl.alloc_device_io()
    for k, chunk in enumerate(chunks):
        if k >= pl.depth:
            outs[k - pl.depth] = pl.download(slot=k)
        pl.upload(chunk, freq_offsets=f, slot=k)
        pl.enqueue(slot=k)
    for k in range(max(len(chunks) - pl.depth, 0), len(chunks)):
        outs[k] = pl.download(slot=k)
    pl.close()
    assert sorted(outs) == list(range(n_chunks))
    for k in range(n_chunks):
        _valid_equal(refs[k], outs[k])
    for k in range(0, n_chunks, 4):
        hard, soft, n_soft, bp, mm = outs[k]
        for r in range(rows):
            o = OracleSignalProcessor(2.4e6)
            ref = o.process(synth.cu8_to_c128(chunks[k][2 * n * r:2 * n * (r + 1)]), f[r])
            ns = int(n_soft[r])
            assert ns == len(ref) + 1 and bp[r] == o.best_phase, (k, r)
            np.testing.assert_array_equal(hard[r, :ns - 1], ref, err_msg=f"chunk {k} row {r}")
            assert np.max(np.abs(soft[r, :ns] - o.symbols)) <= 1e-10 * np.max(np.abs(o.symbols)), (k, r)


@pytest.mark.gpu
def test_plan_wait_for_orders_two_plans_on_the_device():
    """tdm_plan_wait_for: plan B's pass enqueued behind plan A's with the wait runs alone (its own event span is a lone pass's),
    without it the two share the device and B's span grows."""
    from tetraear_amd import _lib, synth
    from tetraear_amd.batch import BatchDemodulator
    n, rows = 262144, 64
    u8 = synth.noise_cu8(n * rows, 8200)
    a = BatchDemodulator(2.4e6, n, rows, "cu8")
    b = BatchDemodulator(2.4e6, n, rows, "cu8")
    for p in (a, b):
        p.alloc_device_io()
        p.upload(u8)
        for _ in range(20):
            p.enqueue()
        p.sync()
    a.time_begin(per_stage=False); a.enqueue(); t_alone = a.time_end()
    a.enqueue()
    b.wait_for(a)
    b.time_begin(per_stage=False); b.enqueue(); t_ordered = b.time_end()
    a.sync()
    a.enqueue()
    b.time_begin(per_stage=False); b.enqueue(); t_beside = b.time_end()
    a.sync()
    print(f"one pass alone {t_alone:.4f} ms, behind the other plan's pass (tdm_plan_wait_for) {t_ordered:.4f} ms, beside it {t_beside:.4f} ms")
    assert t_ordered < 1.25 * t_alone
    with pytest.raises(_lib.TetraHipError):
        _lib.check(_lib.load().tdm_plan_wait_for(None, a.handle))
    a.close(); b.close()


def test_pipelined_host_logic_with_stand_in_plans(monkeypatch):
    """CPU tier: the turn-taking logic of PipelinedBatchDemodulator on stand-in plans (no device): step k goes to plan k % depth,
    `upload(slot=k)` feeds that plan only, `download` returns the last step's plan, per-stage timing orders every step behind the
    previous one (wait_for) and plain timing does not."""
    import tetraear_amd.batch as batch
    log = []

    class Plan:
        count = 0

        def __init__(self, *a, **k):
            self.idx = Plan.count
            Plan.count += 1
            self.info, self.soft_dtype, self.data = "info", np.complex128, None

        def alloc_device_io(self, shared_input=False): log.append(("alloc", self.idx, shared_input))
        def upload(self, iq, fo=None, ps=None): self.data = iq; log.append(("upload", self.idx))
        def enqueue(self): log.append(("enqueue", self.idx))
        def wait_for(self, other): log.append(("wait", self.idx, other.idx))
        def sync(self): log.append(("sync", self.idx))
        def download(self): log.append(("download", self.idx)); return ("out", self.idx, self.data)
        def time_begin(self, per_stage=True): log.append(("begin", self.idx, per_stage))
        def time_end(self): return 1.0 + self.idx
        def stage_times(self): return {"dec_block": 0.1 * (self.idx + 1)}
        def close(self): log.append(("close", self.idx))

    monkeypatch.setattr(batch, "BatchDemodulator", Plan)
    pl = batch.PipelinedBatchDemodulator(2.4e6, 4096, 4, "cu8", depth=3)
    assert pl.depth == 3
    pl.alloc_device_io()
    pl.upload("all")
    assert [p.data for p in pl.plans] == ["all"] * 3
    for k in range(5):
        pl.upload(f"chunk{k}", slot=k)
        pl.enqueue()
    assert [e[1] for e in log if e[0] == "enqueue"] == [0, 1, 2, 0, 1]
    assert not [e for e in log if e[0] == "wait"]                  # steps overlap unless a per-stage pass is on
    assert pl.download() == ("out", 1, "chunk4") and [o[2] for o in pl.download_all()] == ["chunk3", "chunk4", "chunk2"]
    pl.time_begin(per_stage=True)
    pl.enqueue(); pl.enqueue()
    assert [e for e in log if e[0] == "wait"] == [("wait", 2, 1), ("wait", 0, 2)]
    assert pl.time_end() == 3.0 and abs(pl.stage_times()["dec_block"] - 0.2) < 1e-12
    keep = Plan.stage_times
    Plan.stage_times = lambda self: {} if self.idx == 1 else keep(self)      # (a plan that took no step of a short per-stage pass)
    assert abs(pl.stage_times()["dec_block"] - 0.2) < 1e-12
    Plan.stage_times = keep
    pl.enqueue()
    assert len([e for e in log if e[0] == "wait"]) == 2             # (back to overlapping steps after time_end)
    pl.close()
    assert [e[1] for e in log if e[0] == "close"] == [0, 1, 2]
    assert isinstance(batch.batch_demodulator(2.4e6, 4096, 4, "cu8", depth=1), Plan)


def test_pipelined_slot_calls_wait_for_their_own_plan_only(monkeypatch):
    """CPU tier: the capture-loop calls with a slot, on stand-in plans that record every call in order.  `upload(slot=k)` is a
    blocking null-stream copy that the plan's non-blocking stream does not order: it must come after a sync of plan k % depth
    (which may still run the step it took a round ago) and sync no other plan; `download(slot=k)` syncs and reads plan k % depth
    only; `enqueue(slot=k)` goes to plan k % depth and the turn moves on from there.  Without a slot the calls behave as before."""
    import tetraear_amd.batch as batch
    log = []

    class Plan:
        count = 0

        def __init__(self, *a, **k):
            self.idx = Plan.count
            Plan.count += 1
            self.info, self.soft_dtype, self.data, self.busy = "info", np.complex128, None, False

        def alloc_device_io(self, shared_input=False): pass
        def upload(self, iq, fo=None, ps=None):
            assert not self.busy, f"plan {self.idx}: input overwritten under a step in flight"
            self.data = iq
            log.append(("upload", self.idx))
        def enqueue(self): self.busy = True; log.append(("enqueue", self.idx))
        def wait_for(self, other): log.append(("wait", self.idx, other.idx))
        def sync(self): self.busy = False; log.append(("sync", self.idx))
        def download(self): log.append(("download", self.idx)); return ("out", self.idx, self.data)
        def close(self): pass

    monkeypatch.setattr(batch, "BatchDemodulator", Plan)
    for depth in (2, 3):
        Plan.count = 0
        pl = batch.PipelinedBatchDemodulator(2.4e6, 4096, 4, "cu8", depth=depth)
        pl.alloc_device_io()
        outs = {}
        for k in range(12):
            if k >= depth:
                del log[:]
                outs[k - depth] = pl.download(slot=k)
                assert log == [("sync", k % depth), ("download", k % depth)], (depth, k, log)
            del log[:]
            pl.upload(f"chunk{k}", slot=k)
            assert log == [("sync", k % depth), ("upload", k % depth)], (depth, k, log)
            del log[:]
            pl.enqueue(slot=k)
            assert log == [("enqueue", k % depth)], (depth, k, log)
        for k in range(12 - depth, 12):
            del log[:]
            outs[k] = pl.download(slot=k)
            assert log == [("sync", k % depth), ("download", k % depth)]
        assert outs == {k: ("out", k % depth, f"chunk{k}") for k in range(12)}
        # a plan with a step in flight: its upload comes after its own sync, and no other plan is waited for
        pl.enqueue(slot=1)
        pl.enqueue(slot=0)
        del log[:]
        pl.upload("again", slot=depth + 1)
        assert log == [("sync", 1), ("upload", 1)]
        # enqueue(slot=k) moves the turn on from plan k % depth: a slot-less step goes to the next plan
        del log[:]
        pl.enqueue(slot=2 * depth - 1)
        pl.enqueue()
        pl.enqueue()
        assert [e[1] for e in log if e[0] == "enqueue"] == [depth - 1, 0, 1]
        # without a slot: download waits for every plan and reads the last step's plan; upload fills (and first waits for)
        # every plan
        del log[:]
        assert pl.download() == ("out", 1, "again")
        assert log == [("sync", i) for i in range(depth)] + [("download", 1)]
        del log[:]
        pl.upload("all")
        assert log == [e for i in range(depth) for e in (("sync", i), ("upload", i))]
        assert [p.data for p in pl.plans] == ["all"] * depth
        pl.close()
