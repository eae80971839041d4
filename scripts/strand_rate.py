"""Device-side cost of placing DNA reads on the reverse strand / on both strands (rk_place_packed_device_strands) on C2's database:
FORWARD, REVERSE and BOTH through the device entry point in one process, on bench.py's reads (uniform, generated on the device into
the packed layout, seed 1), with bench.py's warm-up and per-step event timing.  The yardstick is the FORWARD line of the same run
(it is rk_place_packed_device: compare it with `python bench.py`'s C2 line).  The reverse-complement and merge kernels are also
timed on their own, to say what BOTH costs beyond two placements.

    python scripts/strand_rate.py [--reads 10000000] [--steps 10] [--warmup 10] > profiles/strand_rate.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import rappas_amd as ra
from rappas_amd import _lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=10)
a = ap.parse_args()

alphabet, k, leaves, n_keys, n_entries, rlen, _ = synth.CONFIGS["C2"]
sdb = synth.make_config_db("C2", seed=42)
db = ra.PhyloKmerDB.from_synth(sdb)
pp = ra.PlacementProcess(db)
dev = torch.device("cuda", 0)
n, K, wpr = a.reads, 7, db.packed_words(rlen)
gen = torch.Generator(device=dev)
gen.manual_seed(1)
packed = torch.randint(-2**31, 2**31, (n, wpr), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
tail_bits = rlen * 2 - 32 * (wpr - 1)
if tail_bits < 32:
    packed[:, wpr - 1] &= (1 << tail_bits) - 1
out = dict(n_rows=torch.empty(n, dtype=torch.uint8, device=dev), branch=torch.empty((n, K), dtype=torch.int16, device=dev),
           score=torch.empty((n, K), dtype=torch.float32, device=dev), lwr=torch.empty((n, K), dtype=torch.float64, device=dev),
           flags=torch.empty(n, dtype=torch.int32, device=dev))
print(f"{torch.cuda.get_device_name(0)}; C2 database ({sdb.n_keys} keys / {sdb.n_entries} entries, seed 42), {n} reads of {rlen} bases, keep_at_most {K}; "
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


rates = {}
for strand in ("forward", "reverse", "both", "forward"):  # (forward again at the end: drift within the run)
    ms = timed(lambda: pp.place_packed(packed, fixed_len=rlen, out=out, keepAtMost=K, strand=strand))
    med = statistics.median(ms)
    rates.setdefault(strand, []).append(n / (med * 1e-3))
    rev = int((out["flags"] & ra.RK_FLAG_REVERSE != 0).sum().item())
    placed = int((out["flags"] & 1 != 0).sum().item())
    print(f"{strand.upper():8s} median {med:8.3f} ms  min {min(ms):8.3f}  max {max(ms):8.3f}  -> {n / (med * 1e-3) / 1e6:7.1f} Mreads/s   "
          f"(placed {placed}, results from the reverse strand {rev})", flush=True)
fwd = max(rates["forward"])
print(f"BOTH / FORWARD = {fwd / rates['both'][0]:.3f} x the time (expectation <= 2.1), REVERSE / FORWARD = {fwd / rates['reverse'][0]:.3f} x; "
      f"FORWARD first / last in this run: {rates['forward'][0] / 1e6:.1f} / {rates['forward'][1] / 1e6:.1f} Mreads/s")

# the kernels BOTH adds to two placements, on their own
lib = _lib.load()
st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
rev_rec = torch.empty_like(packed)
out2 = {key: t.clone() for key, t in out.items()}
res = lambda d: _lib.rk_result(d["n_rows"].data_ptr(), d["branch"].data_ptr(), d["score"].data_ptr(), d["lwr"].data_ptr(), d["flags"].data_ptr())
r1, r2 = res(out), res(out2)
ms = timed(lambda: _lib.check(lib.rk_revcomp_packed_device(db.handle, n, packed.data_ptr(), wpr, None, rlen, rev_rec.data_ptr(), st)))
print(f"revcomp_packed_kernel alone: median {statistics.median(ms):.3f} ms ({2 * n * wpr * 4 / statistics.median(ms) / 1e6:.0f} GB/s read + written)")
ms = timed(lambda: _lib.check(lib.rk_merge_strands_device(db.handle, K, n, C.byref(r1), C.byref(r2), st)))
print(f"merge_results_kernel alone (second set = a copy: ties, nothing switches): median {statistics.median(ms):.3f} ms")
out2["score"] += 1.0
ms = timed(lambda: _lib.check(lib.rk_merge_strands_device(db.handle, K, n, C.byref(r1), C.byref(r2), st)))
print(f"merge_results_kernel alone (every placed read switches on the first call, later calls tie): median {statistics.median(ms):.3f} ms")
db.close()
