"""CPU: the persistent host-fed stream (include/tetrahip.h tdm_stream_*) without a device.

- the new exports are bound with the header's signatures and the version moved to 103 everywhere;
- every argument refusal of tdm_stream_create / _acquire / _submit / _collect happens before any HIP call;
- the slot ring (csrc/stream_ring.hpp) compiled alone with g++ and driven through its states;
- the host logic of iter_recording(overlapped=True) on a stand-in StreamingDemodulator.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tetraear_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["tdm_stream_create", "tdm_stream_destroy", "tdm_stream_acquire", "tdm_stream_submit", "tdm_stream_collect",
       "tdm_link_ceiling"]


def _header():
    return open(os.path.join(REPO, "include", "tetrahip.h")).read()


def test_stream_exports_are_bound_with_the_headers_signatures():
    txt = _header()
    L = _lib.load()
    assert L.tdm_version() == 103 == _lib.ABI_VERSION == _lib.header_version()
    ctype = {"double": C.c_double, "int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t}
    for name in NEW:
        assert hasattr(L, name), name
        m = re.search(r"TDM_API\s+int\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params), (name, params, args)
        for p, a in zip(params, args):
            base = p.replace("const ", "").split()[0]
            if "*" in p:        # pointers: void* or a typed pointer of the right width
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is ctype[base], (name, p, a)


def test_stream_result_has_the_headers_layout(tmp_path):
    fields = [f[0] for f in _lib.StreamResult._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tetrahip.h"\nint main(void){printf("%zu", sizeof(tdm_stream_result));'
                   + "".join('printf(" %%zu", offsetof(tdm_stream_result, %s));' % f for f in fields)
                   + 'printf(" %d %d", (int)TDM_STREAM_SOFT, (int)TDM_NOT_READY);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.StreamResult)
    assert got[1:-2] == [getattr(_lib.StreamResult, f).offset for f in fields]
    assert got[-2:] == [_lib.STREAM_SOFT, _lib.TDM_NOT_READY]


def _create(fs=2.4e6, n=65536, rows=4, fmt=0, mode=0, depth=3, flags=0, fo=None, ps=None, rpc=1, out=True):
    L = _lib.load()
    h = C.c_void_p()
    return L.tdm_stream_create(fs, n, rows, fmt, mode, depth, flags, fo, ps, rpc, 0, C.byref(h) if out else None)


def test_stream_create_refusals_need_no_device():
    inv, uns = _lib.TDM_ERR_INVALID, _lib.TDM_ERR_UNSUPPORTED
    offs = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    cases = [
        (dict(depth=0), inv, "depth"),
        (dict(depth=-3), inv, "depth"),
        (dict(rows=0), inv, "n_rows"),
        (dict(n=0), inv, "n_samples"),
        (dict(fs=0.0), inv, "sample_rate"),
        (dict(fmt=4), inv, "in_fmt"),
        (dict(fmt=-1), inv, "in_fmt"),
        (dict(mode=3), inv, "mode"),
        (dict(flags=2), inv, "flags"),
        (dict(rpc=3), inv, "rows_per_chunk"),
        (dict(rpc=0), inv, "rows_per_chunk"),
        (dict(out=False), inv, "out"),
        (dict(mode=_lib.MODE_TETRA, fs=72000.0, ps=offs), uns, "pre_shift"),
        (dict(mode=_lib.MODE_TETRA_GARDNER, fs=72000.0, fo=offs), uns, "freq_offset"),
        (dict(mode=_lib.MODE_TETRA, fs=72000.0, rpc=2), uns, "rows_per_chunk"),
    ]
    for kw, code, word in cases:
        assert _create(**kw) == code, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())


def test_stream_calls_on_a_null_stream_are_refused():
    L = _lib.load()
    p, seq, r = C.c_void_p(), C.c_int64(), _lib.StreamResult()
    assert L.tdm_stream_acquire(None, C.byref(p), C.byref(seq)) == _lib.TDM_ERR_INVALID
    assert L.tdm_stream_submit(None, 100, 1) == _lib.TDM_ERR_INVALID
    assert L.tdm_stream_collect(None, 1, C.byref(r)) == _lib.TDM_ERR_INVALID
    assert L.tdm_stream_destroy(None) == 0
    assert L.tdm_link_ceiling(0, 1 << 30, 0, None) == _lib.TDM_ERR_INVALID


def test_no_device_stream_create_fails_loudly():
    L = _lib.load()
    if L.tdm_device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _create() == -2            # TDM_ERR_NO_DEVICE: valid arguments reach the device check
    gbs = (C.c_double * 3)()
    assert L.tdm_link_ceiling(0, 1 << 30, 4, gbs) == -2
    from tetraear_amd.stream import StreamingDemodulator
    with pytest.raises(_lib.TetraHipError):
        StreamingDemodulator(2.4e6, 65536, 4)


RING_DRIVER = r'''
#include <cstdio>
#include "stream_ring.hpp"
using tdm::StreamRing;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main()
{
    for (int depth = 1; depth <= 4; ++depth) {
        StreamRing r(depth);
        int k; int64_t q; const char *why = nullptr;
        CHECK(r.collect_slot() == -1 && r.submit_slot() == -1);          // nothing in flight, nothing acquired
        int64_t collected = 0;
        for (int64_t s = 0; s < 20; ++s) {
            if (r.in_flight() == depth) {                                  // every slot outstanding: acquire refuses
                CHECK(r.acquire(&k, &q, &why) == -1 && why);
                CHECK(r.submit_slot() == -1);
                CHECK(r.collect_slot() == (int)(collected % depth));
                r.commit_collect();
                ++collected;
            }
            CHECK(r.acquire(&k, &q, &why) == 0 && k == (int)(s % depth) && q == s);
            CHECK(r.acquire(&k, &q, &why) == 0 && k == (int)(s % depth) && q == s);   // again before submit: same slot
            CHECK(r.submit_slot() == k);
            r.commit_submit();
            CHECK(r.submit_slot() == -1);
        }
        while (r.collect_slot() >= 0) { CHECK(r.collect_slot() == (int)(collected % depth)); r.commit_collect(); ++collected; }
        CHECK(collected == 20 && r.in_flight() == 0);
        // a submit that is not committed (failed) leaves the slot acquired and the ring unchanged
        CHECK(r.acquire(&k, &q, &why) == 0 && q == 20);
        CHECK(r.collect_slot() == -1 && r.in_flight() == 0);
        CHECK(r.acquire(&k, &q, &why) == 0 && q == 20);
    }
    std::printf("RING OK\n");
    return 0;
}
'''


def test_stream_ring_state_machine_with_gpp(tmp_path):
    src = tmp_path / "ring.cpp"
    src.write_text(RING_DRIVER)
    exe = tmp_path / "ring"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(REPO, "tetraear_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "RING OK" in out.stdout, out.stdout + out.stderr


# ---- iter_recording(overlapped=True) on a stand-in stream ---------------------------------------------------------------

class FakeStream:
    """StreamingDemodulator's interface over host arrays: a 'result' row is the first byte of its input row (the read index
    is written there by the test), so yields show which read they came from.  Records every call; enforces the ring rules."""
    made = []

    def __init__(self, sample_rate, chunk, rows, fmt="cu8", depth=3, freq_offsets=None, pre_shifts=None, rows_per_chunk=1,
                 device=0, **kw):
        self.chunk, self.rows, self.depth, self.rpc = chunk, rows, depth, rows_per_chunk
        self.in_rows = rows // rows_per_chunk
        self.bufs = [np.full(self.in_rows * chunk * 2, 77, dtype=np.uint8) for _ in range(depth)]
        self.log, self.outs, self.next, self.collected, self.acq = [], {}, 0, 0, None
        self.closed = False
        self.pre_shifts = pre_shifts
        FakeStream.made.append(self)

    def input_buffer(self):
        assert not self.closed
        if self.acq is None:
            assert self.next - self.collected < self.depth, "slot handed out before its result was collected"
            self.acq = self.next
            self.log.append(("acquire", self.next))
        return self.bufs[self.acq % self.depth]

    def submit(self, n_samples=None, n_inputs=None):
        assert self.acq is not None and not self.closed
        b = self.bufs[self.acq % self.depth]
        n = self.chunk if n_samples is None else n_samples
        k = self.in_rows if n_inputs is None else n_inputs
        rows = []
        for i in range(k):
            first = b[2 * n * i]
            assert first != 77, "a row that was never filled was submitted"
            rows += [np.array([first, n % 256, c], dtype=np.uint8) for c in range(self.rpc)]
        rows += [np.zeros(0, dtype=np.uint8)] * (self.rows - len(rows))
        self.outs[self.acq] = rows
        self.log.append(("submit", self.acq, n, k))
        self.acq = None
        self.next += 1
        return self.next - 1

    def collect(self, wait=True):
        assert self.collected < self.next, "collect with nothing in flight"
        if not wait and self.collected % 2:      # every other poll: not ready yet
            self.log.append(("poll", self.collected))
            return None
        s = self.collected
        self.collected += 1
        self.log.append(("collect", s))
        return s, self.outs.pop(s), None, None, None

    def close(self):
        self.closed = True
        self.log.append(("close",))


def _recording(n_samples, chunk):
    """cu8 recording whose read i starts with byte i (first sample's I); the rest mid-scale"""
    u8 = np.full(2 * n_samples, 128, dtype=np.uint8)
    for i in range(0, n_samples, chunk):
        u8[2 * i] = (i // chunk) % 200
    return u8


@pytest.mark.parametrize("n_samples, rows", [(0, 4), (500, 4), (4 * 1000, 4), (6 * 1000, 4), (9 * 1000 + 28, 4),
                                             (13 * 1000 + 1, 4), (8 * 1000 + 999, 2), (3 * 1000 + 5, 1)])
def test_overlapped_host_logic_with_a_stand_in_stream(monkeypatch, n_samples, rows):
    import tetraear_amd.ingest as ingest
    monkeypatch.setattr(ingest, "StreamingDemodulator", FakeStream)
    FakeStream.made.clear()
    chunk = 1000
    u8 = _recording(n_samples, chunk)
    outs = list(ingest.iter_recording(u8, 2.4e6, chunk, 50.0, rows_per_batch=rows, overlapped=True))
    n_full, tail = divmod(n_samples, chunk)
    assert len(outs) == n_full + (1 if tail else 0)
    for i, o in enumerate(outs):                 # in order, one per read; the last one from a short submit of its length
        assert o[0] == i % 200, (i, o)
        assert o[1] == (chunk if i < n_full else tail) % 256
    sd = FakeStream.made[-1]
    subs = [e for e in sd.log if e[0] == "submit"]
    assert sum(e[3] for e in subs) == len(outs)                   # blank inputs never submitted
    if tail:
        assert subs[-1][2:] == (tail, 1)
        subs = subs[:-1]
    assert all(e[2] == chunk for e in subs)
    assert sd.log[-1] == ("close",) and sd.collected == sd.next   # everything collected, then closed
    assert [e[1] for e in sd.log if e[0] == "collect"] == list(range(sd.next))


def test_overlapped_many_carriers_map_onto_rows_per_chunk(monkeypatch):
    import tetraear_amd.ingest as ingest
    monkeypatch.setattr(ingest, "StreamingDemodulator", FakeStream)
    FakeStream.made.clear()
    offs = [-1000.0, 0.0, 2500.0]
    outs = list(ingest.iter_recording(_recording(5 * 1000 + 300, 1000), 2.4e6, 1000, 0.0, rows_per_batch=2, pre_shifts=offs,
                                      overlapped=True))
    sd = FakeStream.made[-1]
    assert sd.rpc == 3 and sd.rows == 6 and list(sd.pre_shifts) == offs * 2
    assert len(outs) == 6 and all(len(o) == 3 for o in outs)
    for i, o in enumerate(outs):
        assert [int(h[2]) for h in o] == [0, 1, 2] and all(h[0] == i for h in o)


def test_overlapped_stream_closed_on_early_stop_and_on_error(monkeypatch):
    import tetraear_amd.ingest as ingest
    monkeypatch.setattr(ingest, "StreamingDemodulator", FakeStream)
    FakeStream.made.clear()
    g = ingest.iter_recording(_recording(20 * 1000, 1000), 2.4e6, 1000, 0.0, rows_per_batch=2, overlapped=True)
    assert next(g)[0] == 0
    g.close()
    assert FakeStream.made[-1].closed

    class Boom:
        def __init__(self):
            self.k = 0

        def readinto(self, view):
            self.k += 1
            if self.k > 3:
                raise OSError("device unplugged")
            np.frombuffer(view, dtype=np.uint8)[:] = 128
            view[0] = self.k
            return len(view)
    with pytest.raises(OSError, match="unplugged"):
        list(ingest.iter_recording(Boom(), 2.4e6, 1000, 0.0, rows_per_batch=1, overlapped=True))
    assert FakeStream.made[-1].closed
