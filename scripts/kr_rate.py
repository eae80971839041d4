"""Device-side cost of the sample-level calls (rk_clade_masses_device, rk_kr_distances_device) at S = 64 and 1 024
samples on C2's tree (999 branches) and on T64k's (65 535).  The sample buffers come from the existing samples path: a synthetic
batch placed on the configuration's database, its reads dealt to the samples at random (accumulate_masses_samples).  The whole call
is timed on the product build; the clade kernel, the profiles pass and the pair kernel (with its reduction, where partials are used)
one by one on the developer build (RK_KR_STEPS).  Beside them rk_kr_distances_host at 16 threads on the same buffer, once: the only
thing to measure against -- the reference has no counterpart.  Warm-up, then HIP events around every step, median (min .. max).

    python scripts/kr_rate.py [--reads 1000000] [--steps 10] [--warmup 10] >> profiles/kr_rate.txt
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
from rappas_amd import _lib, hostio, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--configs", default="C2,T64k")
ap.add_argument("--samples", default="64,1024")
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
n, K = a.reads, 7
FP64_PEAK = 78.6e12 / 2  # FP64 vector operations a second with an FMA counted once (78.6 TFLOP/s counts it twice); these kernels may not fuse
print(f"# {torch.cuda.get_device_name(0)}; sample buffers from {n} reads, keep_at_most {K}; {a.warmup} warm-up + {a.steps} timed steps per line, "
      f"HIP events around every step, median (min .. max)")


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
    return f"{t[0]:9.3f} ms ({t[1]:9.3f} .. {t[2]:9.3f})"


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
        terms = S * (S + 1) // 2 * B * 2  # |.| terms of the pairs on or above the diagonal
        # ---- the product build: the whole call, and the clade call on its own ----
        et = ra.EdgeTree(parent, bl)
        whole = timed(lambda: et.kr_distances(masses, S))
        clade = timed(lambda: et.clade_masses(masses, S))
        D = et.kr_distances(masses, S).cpu().numpy()
        print(f"{tag} rk_kr_distances_device   {fmt(whole)}  workspace {et.kr_work_bytes(S) / 2**20:9.1f} MiB", flush=True)
        print(f"{tag} rk_clade_masses_device   {fmt(clade)}", flush=True)
        et.close()
        # ---- the developer build: the three steps of the call one by one ----
        product = _lib._LIB
        _lib._LIB = _lib.load_dev()
        try:
            et = ra.EdgeTree(parent, bl)
            et.kr_distances(masses, S)  # (the workspace holds what every step reads)
            for bit, name in ((1, "clade_masses_kernel"), (2, "kr_profiles_kernel"), (4, "kr_pairs_kernel (+ reduce)")):
                os.environ["RK_KR_STEPS"] = str(bit)
                t = timed(lambda: et.kr_distances(masses, S))
                line = f"{tag} {name:26s} {fmt(t)}"
                if bit == 4:
                    tiles = (S + 63) // 64
                    tile_terms = tiles * (tiles + 1) // 2 * 64 * 64 * B * 2  # what the launched tiles sum, padding and both triangles of a diagonal tile included
                    line += (f"  {terms / t[0] / 1e6:8.2f} G terms/s of the matrix; 3 FP64 operations a term over the launched tiles: "
                             f"{3 * tile_terms / (t[0] * 1e-3) / FP64_PEAK * 100:5.1f} % of the FP64 vector rate")
                print(line, flush=True)
            os.environ.pop("RK_KR_STEPS")
            et.close()
        finally:
            _lib._LIB = product
        # ---- the host twin at 16 threads, once ----
        if not a.no_host:
            hm = masses.cpu().numpy().view(np.uint64)
            t0 = time.perf_counter()
            H = ra.kr_distances_host(parent, bl, hm, S, threads=16)
            dt = time.perf_counter() - t0
            same = bool((H.view(np.uint64) == D.view(np.uint64)).all())
            print(f"{tag} rk_kr_distances_host, 16 threads {dt * 1e3:11.1f} ms: {dt * 1e3 / whole[0]:8.1f} x the device call; the same bits: {same}", flush=True)
        del sample, masses
    db.close()
    del out
