"""Device-side cost of the edge masses (rk_masses_accumulate_device) next to the placement that made the results:
10^7 reads at keep_at_most 7 on C2's tree (999 branches: the kernel's LDS variant) and on T64k's (65 535: global atomics behind the
per-block cache of the busiest bins), uniform
reads (bench.py's: generated on the device into the packed layout, seed 1) and clade-shaped ones (scripts/clade_bench.py's:
synth.make_clade_db / make_clade_reads, 2 * 10^6 reads cut from the genome, repeated five times), plus the contention case no
placement produces: every row of every read on one branch.  Per batch: the accumulate call's time, the plain placement call's time
on the same batch in the same process, and the bytes of the result set the call reads (n_rows, branch, lwr: 1 + 10 K per read)
divided by its time.  Warm-up, then HIP events around every step, median.

--variants switches to the developer build and repeats the accumulate call with the variant forced (RK_MASSES_VARIANT: lds | global |
cache; RK_MASSES_BLOCKS_PER_CU), also on T4k's tree (3 999 branches, the largest bench tree below the LDS limit): the runs the
constants RK_MASSES_LDS_MAX_BRANCHES / RK_MASSES_LDS_BLOCKS_PER_CU in rk_masses_impl.h were chosen from.  (The "+combine" lines of
profiles/masses_rate.txt are of a variant that was measured, rejected and removed: DESIGN.md 4.7.)

    python scripts/masses_rate.py [--reads 10000000] [--steps 10] [--warmup 10] [--variants] >> profiles/masses_rate.txt
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rappas_amd as ra
from rappas_amd import _lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--variants", action="store_true")
ap.add_argument("--configs", default=None, help="comma-separated, default C2,T64k (with --variants: C2,T4k,T64k)")
a = ap.parse_args()
if a.variants:
    _lib._LIB = _lib.load_dev()  # the only build that reads the knobs; everything below goes through it
configs = (a.configs or ("C2,T4k,T64k" if a.variants else "C2,T64k")).split(",")
dev = torch.device("cuda", 0)
n, K = a.reads, 7
print(f"# {torch.cuda.get_device_name(0)}; {n} reads, keep_at_most {K}; {a.warmup} warm-up + {a.steps} timed steps per line, HIP events around every step, median (min .. max); "
      f"{'developer build, variants forced' if a.variants else 'product build'}")


def timed(step):
    step()
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
    ms = [e0.elapsed_time(e1) for e0, e1 in evs]
    return statistics.median(ms), min(ms), max(ms)


def report(tag, pp, out, place_ms=None):
    B = pp.db.info.n_branches
    m = torch.zeros(ra.masses_words(B), dtype=torch.int64, device=dev)
    nbytes = n * (1 + 10 * K)
    rows = int(out["n_rows"].sum(dtype=torch.int64).item())
    top = torch.bincount(out["branch"].view(torch.int16)[:, 0][out["n_rows"] > 0].to(torch.int64) & 0xFFFF, minlength=B)
    shape = f"{rows / n:.2f} rows a read, busiest best-branch {int(top.max().item()) / max(1, int((out['n_rows'] > 0).sum().item())):.4f} of the placed reads"
    runs = [("", {})]
    if a.variants:
        runs = [(v, {"RK_MASSES_VARIANT": v}) for v in ("lds", "global", "cache") if B <= 4094 or "lds" not in v]
        if B <= 4094:
            runs += [(f"lds, {b} blocks a CU", {"RK_MASSES_VARIANT": "lds", "RK_MASSES_BLOCKS_PER_CU": str(b)}) for b in (1, 2, 8, 16)]
    for name, env in runs:
        for k_, v_ in env.items():
            os.environ[k_] = v_
        med, lo, hi = timed(lambda: pp.accumulate_masses(out, masses=m))
        for k_ in env:
            del os.environ[k_]
        vs = f"; placement {place_ms:8.3f} ms: the accumulate call adds {100 * med / place_ms:5.2f} %" if place_ms else ""
        print(f"{tag:28s} {name:22s} accumulate {med:7.3f} ms ({lo:7.3f} .. {hi:7.3f}), {nbytes / med / 1e6:7.0f} GB/s of result set{vs}   [{shape}]", flush=True)


def empty_out():
    return dict(n_rows=torch.empty(n, dtype=torch.uint8, device=dev), branch=torch.empty((n, K), dtype=torch.int16, device=dev),
                score=torch.empty((n, K), dtype=torch.float32, device=dev), lwr=torch.empty((n, K), dtype=torch.float64, device=dev),
                flags=torch.empty(n, dtype=torch.int32, device=dev))


for cfg in configs:
    alphabet, k, leaves, n_keys, n_entries, rlen, _ = synth.CONFIGS[cfg]
    # ---- uniform: bench.py's database and reads ----
    sdb = synth.make_config_db(cfg, seed=42)
    db = ra.PhyloKmerDB.from_synth(sdb)
    pp = ra.PlacementProcess(db)
    wpr = db.packed_words(rlen)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    packed = torch.randint(-2**31, 2**31, (n, wpr), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
    tail_bits = rlen * 2 - 32 * (wpr - 1)
    if tail_bits < 32:
        packed[:, wpr - 1] &= (1 << tail_bits) - 1
    out = empty_out()
    place_ms = timed(lambda: pp.place_packed(packed, fixed_len=rlen, out=out, keepAtMost=K))[0]
    report(f"{cfg} ({sdb.n_branches}) uniform", pp, out, place_ms)
    # ---- the contention case: every row on one branch (no placement behind it) ----
    out["n_rows"].fill_(K)
    out["branch"].fill_(7)
    out["lwr"].fill_(0.5)
    report(f"{cfg} ({sdb.n_branches}) one branch", pp, out)
    db.close()
    del packed
    # ---- clade-shaped: the same tree, rows of a stretch of the genome share a neighbourhood ----
    cdb_s, genome = synth.make_clade_db(k=k, n_branches=sdb.n_branches)
    nc = min(2_000_000, n)
    cseq, coff = synth.make_clade_reads(genome, nc, rlen)
    cdb = ra.PhyloKmerDB.from_synth(cdb_s)
    cpp = ra.PlacementProcess(cdb)
    cpk = torch.from_numpy(cpp.pack_reads_host(cseq, coff)[0].view(np.int32)).to(dev)
    cpk = cpk.repeat((n + nc - 1) // nc, 1)[:n].contiguous()
    place_ms = timed(lambda: cpp.place_packed(cpk, fixed_len=rlen, out=out, keepAtMost=K))[0]
    report(f"{cfg} ({sdb.n_branches}) clade", cpp, out, place_ms)
    cdb.close()
    del cpk, out
