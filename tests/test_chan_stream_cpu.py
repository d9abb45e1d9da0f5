"""CPU: the stateful channeliser (include/tetrahip.h tdm_channeliser_*) without a device.

- the five exports are bound with the header's signatures;
- every argument refusal of tdm_channeliser_create happens before any HIP call;
- the position rule (csrc/chan_stream.hpp) compiled alone with g++ against a Python statement of the same rule over
  thousands of random chunkings: output counts, o, s_base, hist_valid and where every history sample comes from;
- iter_channels' read splitting on a stand-in StreamingChanneliser.
"""
import ctypes as C
import io
import os
import re
import subprocess

import numpy as np
import pytest

from tetraear_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["tdm_channeliser_create", "tdm_channeliser_push", "tdm_channeliser_reset", "tdm_channeliser_position",
       "tdm_channeliser_destroy"]
MS = [72, 80, 96, 128, 400]


def test_channeliser_exports_are_bound_with_the_headers_signatures():
    txt = open(os.path.join(REPO, "include", "tetrahip.h")).read()
    L = _lib.load()
    assert L.tdm_version() == 103 == _lib.ABI_VERSION == _lib.header_version()
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    for name in NEW:
        assert hasattr(L, name), name
        m = re.search(r"TDM_API\s+int\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params), (name, params, args)
        for p, a in zip(params, args):
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is ctype[p.replace("const ", "").split()[0]], (name, p, a)


def _create(M=400, D=125, fmt=0, streams=32, max_n_in=1 << 20, out=True):
    h = C.c_void_p()
    return _lib.load().tdm_channeliser_create(M, D, fmt, streams, max_n_in, 0, C.byref(h) if out else None)


def test_channeliser_create_refusals_need_no_device():
    inv, uns = _lib.TDM_ERR_INVALID, _lib.TDM_ERR_UNSUPPORTED
    cases = [
        (dict(M=100), uns, "M in"),
        (dict(M=0), uns, "M in"),
        (dict(fmt=3), inv, "in_fmt"),
        (dict(fmt=-1), inv, "in_fmt"),
        (dict(D=0), inv, "D < 1"),
        (dict(D=-5), inv, "D < 1"),
        (dict(streams=0), inv, "n_streams"),
        (dict(streams=65536), inv, "n_streams"),
        (dict(max_n_in=0), inv, "max_n_in"),
        (dict(max_n_in=1 << 40), inv, "max_n_in"),
        (dict(M=96, D=100000), uns, "LDS"),
        (dict(out=False), inv, "out"),
    ]
    for kw, code, word in cases:
        assert _create(**kw) == code, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())


def test_channeliser_calls_on_a_null_object_are_refused():
    L = _lib.load()
    a, b = C.c_int64(), C.c_int64()
    buf = np.zeros(16, dtype=np.uint8)
    assert L.tdm_channeliser_push(None, _lib.ptr(buf), 4, _lib.ptr(buf), 0, C.byref(a), 0) == _lib.TDM_ERR_INVALID
    assert L.tdm_channeliser_reset(None) == _lib.TDM_ERR_INVALID
    assert L.tdm_channeliser_position(None, C.byref(a), C.byref(b)) == _lib.TDM_ERR_INVALID
    assert L.tdm_channeliser_destroy(None) == 0


def test_no_device_channeliser_create_fails_loudly():
    L = _lib.load()
    if L.tdm_device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _create() == -2            # TDM_ERR_NO_DEVICE: valid arguments reach the device check
    from tetraear_amd.channeliser import StreamingChanneliser
    with pytest.raises(_lib.TetraHipError):
        StreamingChanneliser(400, 125, "cu8", streams=2, max_n_in=4096)


# ---- the position rule under g++ ------------------------------------------------------------------------------------------

POS_DRIVER = r'''
#include <cstdio>
#include "chan_stream.hpp"
// stdin: lines "pos n M D k j1 .. jk"; stdout per line: "n_out o s_base hist_valid src(j1) .. src(jk)"
int main()
{
    long long pos, n;
    int M, D, k;
    while (std::scanf("%lld %lld %d %d %d", &pos, &n, &M, &D, &k) == 5) {
        const tdm::ChanPush p = tdm::chan_push(pos, n, M, D, 3 * M);
        std::printf("%lld %lld %d %d", (long long)p.n_out, (long long)p.o, p.s_base, p.hist_valid);
        for (int i = 0; i < k; ++i) {
            long long j;
            if (std::scanf("%lld", &j) != 1) return 2;
            std::printf(" %lld", (long long)tdm::chan_hist_source(j, n, 3 * M));
        }
        std::printf("\n");
    }
    return 0;
}
'''


def _rule(pos, n, M, D):
    """the rule stated on absolute indices: the outputs whose instants m*D fall in [pos, pos + n)"""
    inst = range(pos + (-pos) % D, pos + n, D)
    o = inst[0] - pos if len(inst) else pos + (-pos) % D - pos
    return len(inst), o, (pos + (-pos) % D) % M, min(pos, 3 * M - 1)


def test_position_rule_with_gpp(tmp_path):
    src = tmp_path / "pos.cpp"
    src.write_text(POS_DRIVER)
    exe = tmp_path / "pos"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(REPO, "tetraear_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    rng = np.random.default_rng(2026)
    lines, want = [], []
    for c in range(400):                                   # random chunkings of one stream each
        M = int(rng.choice(MS))
        D = int(rng.choice([1, 2, 24, 27, 32, 125, M, M + 1, 4 * M + 3]))
        L1 = 3 * M - 1
        pos = 0 if c % 4 else int(rng.integers(0, 1 << 62))   # a quarter start far out: no overflow of s_base
        for _ in range(12):
            n = int(rng.choice([0, 1, D - 1 if D > 1 else 1, L1 - 1, L1, L1 + 1, 7 * D + 3, int(rng.integers(1, 5 * L1)),
                                1 << 20]))
            js = sorted({j for j in (0, L1 - 1, L1 - n - 1, L1 - n, L1 - n + 1, int(rng.integers(0, L1))) if 0 <= j < L1})
            lines.append(f"{pos} {n} {M} {D} {len(js)} " + " ".join(map(str, js)))
            want.append((pos, n, M, D, js))
            pos += n
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    got = out.stdout.split("\n")
    assert len(got) >= len(want)
    for (pos, n, M, D, js), g in zip(want, got):
        v = [int(t) for t in g.split()]
        assert tuple(v[:4]) == _rule(pos, n, M, D), (pos, n, M, D, v[:4])
        L1 = 3 * M - 1
        # history slot j after the push holds absolute sample pos + n - L1 + j: from the push (local index) or from the
        # old history, whose slot s holds absolute sample pos - L1 + s
        for j, s in zip(js, v[4:]):
            absolute = pos + s if s >= 0 else pos - L1 + (-1 - s)
            assert absolute == pos + n - L1 + j, (pos, n, M, j, s)
            assert (s >= 0 and s < n) or (s < 0 and 0 <= -1 - s < L1), (n, j, s)


# ---- iter_channels on a stand-in ------------------------------------------------------------------------------------------

class FakeChanneliser:
    """StreamingChanneliser's interface over host arrays: push records the bytes it got and returns them as [streams][n]."""
    made = []

    def __init__(self, M, D, fmt="cu8", streams=1, max_n_in=1 << 20, device=0):
        self.M, self.D, self.fmt, self.streams, self.max_n_in = M, D, fmt, streams, max_n_in
        self.pushes, self.closed = [], False
        FakeChanneliser.made.append(self)

    def push(self, iq):
        iq = np.asarray(iq)
        assert iq.dtype == np.uint8 and iq.nbytes % self.streams == 0
        n = iq.nbytes // self.streams // {"cu8": 2, "cs8": 2, "cf32": 8}[self.fmt]
        assert 1 <= n <= self.max_n_in
        self.pushes.append(n)
        return iq.copy().reshape(self.streams, -1)

    def close(self):
        self.closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class Trickle(io.RawIOBase):
    """a pipe that hands out at most 999 bytes per read"""

    def __init__(self, data):
        self.data, self.pos = bytes(data), 0

    def readinto(self, view):
        k = min(len(view), 999, len(self.data) - self.pos)
        view[:k] = self.data[self.pos:self.pos + k]
        self.pos += k
        return k


@pytest.mark.parametrize("n, chunk, streams, fmt", [(10000, 3001, 1, "cu8"), (9003, 3001, 1, "cu8"), (1, 3001, 1, "cs8"),
                                                    (0, 500, 1, "cu8"), (3 * 777 + 3 * 10, 777, 3, "cu8"),
                                                    (2 * 400 * 5, 400, 2, "cf32")])
def test_iter_channels_read_splitting(monkeypatch, tmp_path, n, chunk, streams, fmt):
    import tetraear_amd.ingest as ingest
    monkeypatch.setattr(ingest, "StreamingChanneliser", FakeChanneliser)
    fb = 8 if fmt == "cf32" else 2
    data = (np.arange(n * fb, dtype=np.int64) % 251).astype(np.uint8)
    path = tmp_path / "x.bin"
    data.tofile(path)
    for source in (data, str(path), Trickle(data)):
        FakeChanneliser.made.clear()
        blocks = list(ingest.iter_channels(source, 96, 32, chunk, fmt=fmt, streams=streams))
        ch = FakeChanneliser.made[-1]
        per_read = streams * chunk
        full, tail = divmod(n, per_read)
        assert ch.pushes == [chunk] * full + ([tail // streams] if tail else [])
        assert ch.max_n_in == chunk and ch.streams == streams and ch.closed
        assert len(blocks) == len(ch.pushes)
        if blocks:
            np.testing.assert_array_equal(np.concatenate([b.reshape(-1) for b in blocks]), data)


def test_iter_channels_refuses_a_source_that_ends_inside_a_sample(monkeypatch):
    import tetraear_amd.ingest as ingest
    monkeypatch.setattr(ingest, "StreamingChanneliser", FakeChanneliser)
    with pytest.raises(ValueError, match="inside a sample"):
        list(ingest.iter_channels(np.zeros(2 * 1000 + 1, dtype=np.uint8), 96, 32, 300))
    assert FakeChanneliser.made[-1].closed
