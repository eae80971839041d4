"""Device-side cost of placing DNA reads on an amino-acid database in six reading frames (rk_place_packed_device_translated) on C4's
database: in one process, after bench.py's warm-up, with HIP events around every step,
  (a) the translated six-frame call,
  (b) six plain rk_place_packed_device calls over the same six record sets translated beforehand (the existing entry point),
  (c) the translate kernel alone, all six frames,
  (d) the merge kernel alone, the five merges of a call,
  (e) rk_place_batch_translated over the same reads as characters in pageable host memory (wall clock, not events).
(a) - (b) is what the new kernels add; it should be explained by (c) + (d).  Reads are uniform random DNA, generated on the device
into the 2-bit packed layout (seed 1).

    python scripts/translate_rate.py [--reads 1000000] [--len 300] [--steps 10] [--warmup 10] > profiles/translate_rate.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rappas_amd as ra
from rappas_amd import _lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--len", type=int, default=300)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=10)
a = ap.parse_args()

sdb = synth.make_config_db("C4", seed=42)
db = ra.PhyloKmerDB.from_synth(sdb)
pp = ra.PlacementProcess(db)
lib = _lib.load()
dev = torch.device("cuda", 0)
n, K, rlen = a.reads, 7, a.len
wpr = (2 * rlen + 31) // 32
gen = torch.Generator(device=dev)
gen.manual_seed(1)
dna = torch.randint(-2**31, 2**31, (n, wpr), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
tail_bits = rlen * 2 - 32 * (wpr - 1)
if tail_bits < 32:
    dna[:, wpr - 1] &= (1 << tail_bits) - 1
new_out = lambda: dict(n_rows=torch.empty(n, dtype=torch.uint8, device=dev), branch=torch.empty((n, K), dtype=torch.int16, device=dev),
                       score=torch.empty((n, K), dtype=torch.float32, device=dev), lwr=torch.empty((n, K), dtype=torch.float64, device=dev),
                       flags=torch.empty(n, dtype=torch.int32, device=dev), frame=torch.empty(n, dtype=torch.uint8, device=dev))
out = new_out()
print(f"{torch.cuda.get_device_name(0)}; C4 database ({sdb.n_keys} keys / {sdb.n_entries} entries, seed 42), {n} reads of {rlen} bases, keep_at_most {K}; "
      f"{a.warmup} warm-up + {a.steps} timed steps per line, HIP events around every step")
print("kernel:", db.kernel_name())


def timed(step):
    step()  # first launch: code object load, lazy set-up, the workspace
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    for e0, e1 in evs:
        e0.record()
        step()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in evs]


def line(tag, ms):
    med = statistics.median(ms)
    print(f"{tag:58s} median {med:9.3f} ms  min {min(ms):9.3f}  max {max(ms):9.3f}  -> {n / (med * 1e-3) / 1e6:7.2f} M DNA reads/s", flush=True)
    return med


# (a)
t_a = line("(a) rk_place_packed_device_translated, six frames", timed(lambda: pp.place_translated(dna, fixed_len=rlen, out=out, keepAtMost=K)))
placed = int((out["n_rows"] != 0).sum().item())
frames = torch.bincount(out["frame"].to(torch.int64), minlength=256)
print(f"    reads with a result {placed}; winning frames 0..5: {[int(x) for x in frames[:6].tolist()]}")
# (b)
sets = [pp.translate_packed(dna, f, fixed_len=rlen) for f in range(6)]
outs = [new_out() for _ in range(6)]


def six_plain():
    for (aa, aa_lens), o in zip(sets, outs):
        pp.place_packed(aa, lens=aa_lens, out=o, keepAtMost=K)


t_b = line("(b) six rk_place_packed_device calls, records made before", timed(six_plain))
mean_len = sum(float(l.to(torch.float64).mean().item()) for _, l in sets) / 6
print(f"    mean residues per frame record {mean_len:.1f} (of {rlen // 3} codons)")
# (c)
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
aa0, lens0 = sets[0]


def six_translations():
    for f in range(6):
        _lib.check(lib.rk_translate_packed_device(db.handle, f, n, dna.data_ptr(), wpr, None, rlen, aa0.data_ptr(), aa0.shape[1], lens0.data_ptr(), st))


t_c = line("(c) translate_frame_kernel alone, six frames", timed(six_translations))
# (d)
res = lambda d: _lib.rk_result(d["n_rows"].data_ptr(), d["branch"].data_ptr(), d["score"].data_ptr(), d["lwr"].data_ptr(), d["flags"].data_ptr())
best, rs = res(outs[0]), [res(o) for o in outs]


def five_merges():
    for f in range(1, 6):
        _lib.check(lib.rk_merge_frames_device(db.handle, K, n, C.byref(best), outs[0]["frame"].data_ptr(), C.byref(rs[f]), f, st))


t_d = line("(d) merge_results_kernel alone, five merges (later calls tie)", timed(five_merges))
print(f"(a) - (b) = {t_a - t_b:.3f} ms per {n} reads; (c) + (d) = {t_c + t_d:.3f} ms; (a) / (b) = {t_a / t_b:.3f}")
# (e) the host entry point over the same reads as characters in pageable memory: wall clock, the host's packing and PCIe included
idx = np.arange(rlen)
seq = np.ascontiguousarray(synth.DNA_LETTERS[(dna.cpu().numpy().view(np.uint32)[:, idx // 16] >> (2 * (idx % 16)).astype(np.uint32)) & 3]).reshape(-1)
off = np.arange(n + 1, dtype=np.uint64) * rlen
host_out = None


def host_call():
    global host_out
    t0 = time.perf_counter()
    host_out = pp.processQueriesTranslated(seq, off, keepAtMost=K, out=host_out)
    return (time.perf_counter() - t0) * 1e3


for _ in range(1 + a.warmup):
    host_call()
line("(e) rk_place_batch_translated, characters from the host", [host_call() for _ in range(a.steps)])
assert np.array_equal(host_out.frame, out["frame"].cpu().numpy()) and np.array_equal(host_out.n_rows, out["n_rows"].cpu().numpy())
db.close()
