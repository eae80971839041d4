"""Device-side cost of the per-sample edge masses (rk_masses_accumulate_samples_device) on the result sets of
scripts/masses_rate.py: 10^7 reads at keep_at_most 7 on C2's tree (999 branches) and on T64k's (65 535), uniform and clade-shaped, at
S = 1, 8, 64 and 1 024 samples and three membership shapes:
    runs         one entry per read, the samples in contiguous runs of reads (d_member_read NULL)
    interleaved  one entry per read, sample r mod S (d_member_read NULL)
    dedup-like   every read in 1 + geometric(1/2) samples drawn at random, weights 1 .. 4, entries in read order
next to what the engine offered for the same tables before: S calls of rk_masses_accumulate_device, each with the weights zeroed
outside its sample (the one-entry-per-read shapes only; from S = 64 on, 8 of the S calls are timed and the sum is scaled, which the
line says).  At S = 1 the single existing call on the same set stands beside it.  Last, the contention line: every entry on one
(sample, branch) of the 65 535-branch tree.  Warm-up, then HIP events around every step, median (min .. max).

    python scripts/masses_samples_rate.py [--reads 10000000] [--steps 10] [--warmup 10] >> profiles/masses_samples_rate.txt
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rappas_amd as ra
from rappas_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--configs", default="C2,T64k")
ap.add_argument("--samples", default="1,8,64,1024")
a = ap.parse_args()
dev = torch.device("cuda", 0)
n, K = a.reads, 7
SAMPLES = [int(s) for s in a.samples.split(",")]
print(f"# {torch.cuda.get_device_name(0)}; {n} reads, keep_at_most {K}; {a.warmup} warm-up + {a.steps} timed steps per line, HIP events around every step, "
      f"median (min .. max); product build")


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


def members(shape, S, gen):
    """(member_read or None, member_sample, member_weight or None) on the device"""
    r = torch.arange(n, dtype=torch.int64, device=dev)
    if shape == "runs":
        return None, (r * S // n).to(torch.int32), None
    if shape == "interleaved":
        return None, (r % S).to(torch.int32), None
    counts = torch.empty(n, device=dev).geometric_(0.5, generator=gen).clamp_(max=8).to(torch.int64)  # 1 + geometric: 1, 2, 3, ... with mean 2
    read = torch.repeat_interleave(r, counts).to(torch.int32)
    m = read.numel()
    return (read, torch.randint(0, S, (m,), dtype=torch.int32, device=dev, generator=gen), torch.randint(1, 5, (m,), dtype=torch.int32, device=dev, generator=gen))


def report(tag, pp, out):
    B = pp.db.info.n_branches
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    old = torch.zeros(ra.masses_words(B), dtype=torch.int64, device=dev)
    single = timed(lambda: pp.accumulate_masses(out, masses=old))
    print(f"{tag:26s} the existing call, one table             {single[0]:9.3f} ms ({single[1]:9.3f} .. {single[2]:9.3f})", flush=True)
    for S in SAMPLES:
        buf = torch.zeros(ra.masses_samples_words(B, S), dtype=torch.int64, device=dev)
        for shape in ("runs", "interleaved", "dedup-like"):
            read, sample, weight = members(shape, S, gen)
            m = sample.numel()
            med, lo, hi = timed(lambda: pp.accumulate_masses_samples(out, S, sample, member_read=read, member_weight=weight, masses=buf))
            line = f"{tag:26s} S = {S:5d} {shape:12s} {m:9d} entries {med:9.3f} ms ({lo:9.3f} .. {hi:9.3f})"
            if shape != "dedup-like":
                # what the same tables cost before: a call per sample, the weights zero outside it
                some = min(S, 8)
                masks = [(sample == s).to(torch.int32) for s in range(some)]

                def masked():
                    for w in masks:
                        pp.accumulate_masses(out, weights=w, masses=old)
                b = timed(masked)[0] * S / some
                line += f"; {S} masked calls of the existing one {b:10.3f} ms{'' if some == S else f' ({some} timed, scaled)'}: {b / med:7.1f} x"
                if S == 1:
                    line += f"; against the single existing call {med / single[0]:5.2f} x"
                del masks
            print(line, flush=True)
            del read, sample, weight
        del buf


def empty_out():
    return dict(n_rows=torch.empty(n, dtype=torch.uint8, device=dev), branch=torch.empty((n, K), dtype=torch.int16, device=dev),
                score=torch.empty((n, K), dtype=torch.float32, device=dev), lwr=torch.empty((n, K), dtype=torch.float64, device=dev),
                flags=torch.empty(n, dtype=torch.int32, device=dev))


for cfg in a.configs.split(","):
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
    pp.place_packed(packed, fixed_len=rlen, out=out, keepAtMost=K)
    torch.cuda.synchronize()
    del packed
    report(f"{cfg} ({sdb.n_branches}) uniform", pp, out)
    if sdb.n_branches == 65535:
        # ---- the contention line: every row of every read on one branch, every entry in one sample ----
        out["n_rows"].fill_(K)
        out["branch"].fill_(7)
        out["lwr"].fill_(0.5)
        S = 8
        buf = torch.zeros(ra.masses_samples_words(sdb.n_branches, S), dtype=torch.int64, device=dev)
        sample = torch.full((n,), 3, dtype=torch.int32, device=dev)
        med, lo, hi = timed(lambda: pp.accumulate_masses_samples(out, S, sample, masses=buf))
        old = torch.zeros(ra.masses_words(sdb.n_branches), dtype=torch.int64, device=dev)
        one = timed(lambda: pp.accumulate_masses(out, masses=old))[0]
        print(f"{cfg} ({sdb.n_branches}) one (sample, branch) of S = {S}: {med:9.3f} ms ({lo:9.3f} .. {hi:9.3f}); the existing call on the one-branch set {one:9.3f} ms", flush=True)
        del buf, sample, old
    db.close()
    # ---- clade-shaped: the same tree, rows of a stretch of the genome share a neighbourhood ----
    cdb_s, genome = synth.make_clade_db(k=k, n_branches=sdb.n_branches)
    nc = min(2_000_000, n)
    cseq, coff = synth.make_clade_reads(genome, nc, rlen)
    cdb = ra.PhyloKmerDB.from_synth(cdb_s)
    cpp = ra.PlacementProcess(cdb)
    cpk = torch.from_numpy(cpp.pack_reads_host(cseq, coff)[0].view(np.int32)).to(dev)
    cpk = cpk.repeat((n + nc - 1) // nc, 1)[:n].contiguous()
    cpp.place_packed(cpk, fixed_len=rlen, out=out, keepAtMost=K)
    torch.cuda.synchronize()
    del cpk
    report(f"{cfg} ({sdb.n_branches}) clade", cpp, out)
    cdb.close()
    del out
