"""Device-memory leak check of the host-fed paths (GPU box; uses torch only to read the device's free memory): 60 cycles of
StreamingDemodulator -- reference mode with pre-shifts and rows_per_chunk, a short read, a partial batch, soft symbols, a
TETRA-mode stream, and a stream destroyed with steps still in flight --, BatchDemodulator.process_stream
(tdm_process_pipelined), StreamingChanneliser -- host pushes, device pushes, and one destroyed with a push in flight -- and
tdm_link_ceiling / tdm_hbm_ceiling at 1 MiB must leave the free memory where it was.  (tools/leak_check.py does the same for
plans.)"""
import sys; sys.path.insert(0, ".")
import ctypes as C
import numpy as np, torch
from tetraear_amd.stream import StreamingDemodulator
from tetraear_amd.batch import BatchDemodulator, DeviceBuffer
from tetraear_amd.channeliser import StreamingChanneliser
from tetraear_amd._lib import MODE_TETRA
from tetraear_amd import _lib, synth
lib = _lib.load()
def free(): torch.cuda.synchronize(); return torch.cuda.mem_get_info()[0]
u8 = synth.noise_cu8(65536 * 8, 1)
x32 = (np.random.default_rng(0).standard_normal(8 * 8192) + 0j).astype(np.complex64)
u8x2 = np.concatenate([u8, u8])                                   # two batches for process_stream
w8 = u8.reshape(2, -1)                                            # two wideband streams of 262 144 cu8 samples
M, D, N = 400, 125, 1 << 16                                       # channeliser: a push of N samples per stream
d_in, d_out = DeviceBuffer(0, 2 * N * 2), DeviceBuffer(0, 2 * M * -(-N // D) * 8)   # (made once, outside the cycles)
d_in.upload(w8[:, :2 * N])
gbs = (C.c_double * 3)()
def cycle():
    with StreamingDemodulator(2.4e6, 65536, 8, "cu8", depth=3, soft=True, freq_offsets=[100.0] * 8, pre_shifts=[1e4, -2e4] * 4,
                              rows_per_chunk=2) as sd:
        sd.submit_array(u8[:4 * 2 * 65536]); sd.submit_array(u8[:2 * 2 * 65536]); sd.submit_array(u8[:2 * 30000], n_samples=30000)
        while sd.in_flight: sd.collect()
    sd = StreamingDemodulator(2.4e6, 65536, 8, "cu8", depth=2)
    sd.submit_array(u8); sd.submit_array(u8); sd.close()          # destroyed with steps in flight
    with StreamingDemodulator(72000.0, 8192, 8, "cf32", mode=MODE_TETRA, depth=2) as sd:
        sd.submit_array(x32); sd.collect()
    b = BatchDemodulator(2.4e6, 65536, 8, "cu8"); b.process_stream(u8x2, 2, freq_offsets=[100.0] * 8); b.close()
    with StreamingChanneliser(M, D, "cu8", streams=2, max_n_in=N) as ch:
        ch.push(w8[:, :2 * 50000]); ch.push(w8[:, 2 * 50000:2 * N])  # host pushes
        ch.push_device(d_in.ptr, N, d_out.ptr, -(-N // D)); _lib.check(lib.tdm_dev_sync(0))
    ch = StreamingChanneliser(M, D, "cu8", streams=2, max_n_in=N)
    ch.push_device(d_in.ptr, N, d_out.ptr, -(-N // D)); ch.close()   # destroyed with a push in flight
    _lib.check(lib.tdm_link_ceiling(0, 1 << 20, 1, gbs)); _lib.check(lib.tdm_hbm_ceiling(0, 1 << 20, 1, gbs))
cycle(); cycle()
f0 = free()
for i in range(60): cycle()
f1 = free()
print("free before", f0, "after 60 cycles", f1, "delta MB", (f0 - f1) / 1e6)
