"""Device-side cost of the squash clustering (rk_squash_device) at S = 64 and 1 024 samples on C2's tree (999
branches) and on T64k's (65 535), in the manner of scripts/kr_rate.py: the sample buffers come from a synthetic batch placed on the
configuration's database, its reads dealt to the samples at random.  The whole call is timed on the product build, beside
rk_kr_distances_device on the same buffer (the squash call contains it).  The developer build (RK_SQUASH_STEPS) leaves steps out from
the back -- the row reduce, the row kernel, the merge, the pick -- and the differences are the kernels' shares; the row kernel's bytes
a second (16 bytes a node for every sample it sums, over all steps) stand beside what a streaming device-to-device copy reaches on
the same box.  Beside them rk_squash_host at 16 threads on the same buffer, once.  Warm-up, then HIP events around every call, median
(min .. max).  Nothing is gated: recorded numbers.

    python scripts/squash_rate.py [--reads 1000000] [--steps 5] [--warmup 2] >> profiles/squash_rate.txt
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rappas_amd as ra
from rappas_amd import _lib, hostio, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--configs", default="C2,T64k")
ap.add_argument("--samples", default="64,1024")
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
n, K = a.reads, 7
print(f"# {torch.cuda.get_device_name(0)}; sample buffers from {n} reads, keep_at_most {K}; {a.warmup} warm-up + {a.steps} timed calls per line, "
      f"HIP events around every call, median (min .. max)")


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


def fmt(t):
    return f"{t[0]:10.3f} ms ({t[1]:10.3f} .. {t[2]:10.3f})"


# what a streaming copy reaches here: 1 GiB device to device, read and written once each
src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
dst = torch.empty_like(src)
copy = timed(lambda: dst.copy_(src))
copy_rate = 2 * src.numel() / (copy[0] * 1e-3)
print(f"streaming copy, 1 GiB device to device {fmt(copy)}  {copy_rate / 1e12:6.2f} TB/s read + written", flush=True)
del src, dst

for cfg in a.configs.split(","):
    alphabet, k, leaves, n_keys, n_entries, rlen, _ = synth.CONFIGS[cfg]
    sdb = synth.make_config_db(cfg, seed=42)
    B = sdb.n_branches
    tree = hostio.parse_newick(synth.make_newick(B, seed=6))
    parent = np.array([nd.parent.id if nd.parent is not None else -1 for nd in tree.nodes], np.int32)
    bl = np.array([nd.bl for nd in tree.nodes], np.float32)
    db = ra.PhyloKmerDB.from_synth(sdb)
    pp = ra.PlacementProcess(db)
    wpr = db.packed_words(rlen)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    packed = torch.randint(-2**31, 2**31, (n, wpr), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
    tail_bits = rlen * 2 - 32 * (wpr - 1)
    if tail_bits < 32:
        packed[:, wpr - 1] &= (1 << tail_bits) - 1
    out = pp.place_packed(packed, fixed_len=rlen, keepAtMost=K)
    torch.cuda.synchronize()
    del packed
    for S in (int(s) for s in a.samples.split(",")):
        sample = torch.randint(0, S, (n,), dtype=torch.int32, device=dev, generator=gen)
        masses = pp.accumulate_masses_samples(out, S, sample)
        torch.cuda.synchronize()
        tag = f"{cfg} ({B}) S = {S:5d}"
        # ---- the product build: the whole call, and the KR matrix it starts from ----
        et = ra.EdgeTree(parent, bl)
        whole = timed(lambda: et.squash(masses, S))
        kr = timed(lambda: et.kr_distances(masses, S))
        rows, n_merges = et.squash(masses, S)
        rows, n_merges = rows.cpu().numpy().reshape(-1).view(ra.SQUASH_MERGE), int(n_merges.cpu()[0])
        print(f"{tag} rk_squash_device          {fmt(whole)}  {n_merges} merges, workspace {et.squash_work_bytes(S) / 2**20:9.1f} MiB", flush=True)
        print(f"{tag} rk_kr_distances_device    {fmt(kr)}  {kr[0] / whole[0] * 100:5.1f} % of the squash call", flush=True)
        et.close()
        # ---- the developer build: steps left out from the back; the differences are the kernels' shares ----
        product = _lib._LIB
        _lib._LIB = _lib.load_dev()
        try:
            et = ra.EdgeTree(parent, bl)
            t = {}
            for steps in (31, 15, 7, 3, 1):
                os.environ["RK_SQUASH_STEPS"] = str(steps)
                t[steps] = timed(lambda: et.squash(masses, S))
            os.environ.pop("RK_SQUASH_STEPS")
            et.close()
        finally:
            _lib._LIB = product
        # the samples the row kernel sums at step k: the active clusters but the merged one
        summed = sum(n_merges - k for k in range(n_merges))
        print(f"{tag} developer build, all steps {fmt(t[31])}", flush=True)
        for name, hi, lo in (("squash_row_reduce_kernel", 31, 15), ("squash_row_kernel", 15, 7), ("squash_merge_kernel", 7, 3), ("squash_pick_kernel + finish", 3, 1)):
            d = t[hi][0] - t[lo][0]
            line = f"{tag} {name:28s} {d:10.3f} ms over {S - 1} steps, {d / (S - 1) * 1e3:8.2f} us a step"
            if name == "squash_row_kernel" and d > 0:
                rate = 16.0 * B * summed / (d * 1e-3)
                line += f"  {rate / 1e12:6.3f} TB/s of U and V: {rate / copy_rate * 100:5.1f} % of the streaming copy"
            print(line, flush=True)
        print(f"{tag} KR matrix and start        {fmt(t[1])}", flush=True)
        # ---- the host twin at 16 threads, once ----
        if not a.no_host:
            hm = masses.cpu().numpy().view(np.uint64)
            t0 = time.perf_counter()
            H, hn = ra.squash_host(parent, bl, hm, S, threads=16)
            dt = time.perf_counter() - t0
            same = hn == n_merges and bool((H.view(np.uint8) == rows.view(np.uint8)).all())
            print(f"{tag} rk_squash_host, 16 threads {dt * 1e3:11.1f} ms: {dt * 1e3 / whole[0]:8.1f} x the device call; the same bits: {same}", flush=True)
        del sample, masses
    db.close()
    del out
