"""Device-memory leak check of the persistent host-fed stream (GPU box; uses torch only to read the device's free memory):
60 create / use / destroy cycles of StreamingDemodulator -- reference mode with pre-shifts and rows_per_chunk, a short read, a
partial batch, soft symbols, a TETRA-mode stream, and a stream destroyed with steps still in flight -- must leave the free
memory where it was.  (tools/leak_check.py does the same for plans.)"""
import sys; sys.path.insert(0, ".")
import numpy as np, torch
from tetraear_amd.stream import StreamingDemodulator
from tetraear_amd._lib import MODE_TETRA
from tetraear_amd import synth
def free(): torch.cuda.synchronize(); return torch.cuda.mem_get_info()[0]
u8 = synth.noise_cu8(65536 * 8, 1)
x32 = (np.random.default_rng(0).standard_normal(8 * 8192) + 0j).astype(np.complex64)
def cycle():
    with StreamingDemodulator(2.4e6, 65536, 8, "cu8", depth=3, soft=True, freq_offsets=[100.0] * 8, pre_shifts=[1e4, -2e4] * 4,
                              rows_per_chunk=2) as sd:
        sd.submit_array(u8[:4 * 2 * 65536]); sd.submit_array(u8[:2 * 2 * 65536]); sd.submit_array(u8[:2 * 30000], n_samples=30000)
        while sd.in_flight: sd.collect()
    sd = StreamingDemodulator(2.4e6, 65536, 8, "cu8", depth=2)
    sd.submit_array(u8); sd.submit_array(u8); sd.close()          # destroyed with steps in flight
    with StreamingDemodulator(72000.0, 8192, 8, "cf32", mode=MODE_TETRA, depth=2) as sd:
        sd.submit_array(x32); sd.collect()
cycle(); cycle()
f0 = free()
for i in range(60): cycle()
f1 = free()
print("free before", f0, "after 60 cycles", f1, "delta MB", (f0 - f1) / 1e6)
