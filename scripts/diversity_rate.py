"""Device-side cost of the per-sample diversity measures (rk_diversity_device) at S = 64 and 1 024 samples and
n_theta = 0, 1, 4 and 8 on C2's tree (999 branches) and on T64k's (65 535), in the manner of scripts/kmeans_rate.py and on the same
buffers: the sample buffers come from a synthetic batch placed on the configuration's database, its reads dealt to the samples at
random.  The whole call is timed on the product build.  The kernels' times come from the developer build, with RK_DIVERSITY_STEPS
leaving kernels out from the back -- the differences are the kernels' shares: the clade_masses_kernel pass on its own (the device-side
cost the call cannot avoid: it runs no profiles pass), diversity_kernel, its reduce.  The measure kernel's binary64 operation rate
counts what the definition asks for, from the half-edges that carry mass (a > 0; the others are skipped): 47 operations a half-edge
for the fixed columns (two for D and E, two for M, 31 for lg D, the terms and the five pairs of additions), 31 more for lg M once
there is a theta, and 72 a theta (two exponentials of 33, the products, the additions); a division counts as one.  Beside it
kr_pairs_kernel's rate on the same buffers and the same box (RK_KR_STEPS: six operations a node and pair), and rk_diversity_host
at 16 threads, once a shape, for n_theta = 4.  Warm-up, then HIP events around every call, median (min .. max).  Nothing is gated:
recorded numbers.

    python scripts/diversity_rate.py [--reads 1000000] [--steps 5] [--warmup 2] >> profiles/diversity_rate.txt
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
ap.add_argument("--thetas", default="0,1,4,8")
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
n, K = a.reads, 7
THETA = (0.25, 0.5, 1.0, 2.0, 0.0, 3.0, 1.5, 8.0)
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


def with_dev(knob, values, call):
    """{value: timing} of `call(tree)` on the developer build with the environment knob set to each value"""
    product = _lib._LIB
    _lib._LIB = _lib.load_dev()
    t = {}
    try:
        et = ra.EdgeTree(parent, bl)
        for v in values:
            os.environ[knob] = str(v)
            t[v] = timed(lambda: call(et))
        et.close()
    finally:
        os.environ.pop(knob, None)
        _lib._LIB = product
    return t


for cfg in a.configs.split(","):
    alphabet, k_mer, leaves, n_keys, n_entries, rlen, _ = synth.CONFIGS[cfg]
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
        hm = masses.cpu().numpy().view(np.uint64)
        clade = ra.clade_masses_host(parent, hm, S)
        W = 2 * B + 4
        mass = np.stack([hm[s * W:s * W + B] for s in range(S)])
        half_edges = int((clade > 0).sum() + ((clade - mass) > 0).sum())
        tag0 = f"{cfg} ({B}) S = {S:5d}"
        print(f"{tag0} half-edges with mass {half_edges} of {2 * S * B} ({half_edges / (2 * S * B) * 100:5.1f} %)", flush=True)
        # kr_pairs_kernel on the same buffers: the developer build with and without its last step
        kr = with_dev("RK_KR_STEPS", (7, 3), lambda et: et.kr_distances(masses, S))
        pairs_ms = kr[7][0] - kr[3][0]
        pairs_ops = 6.0 * B * S * (S + 1) / 2
        print(f"{tag0} kr_pairs_kernel            {pairs_ms * 1e3:10.2f} us  {pairs_ops / (pairs_ms * 1e-3) / 1e12 if pairs_ms > 0 else 0.0:7.3f} T binary64 operations a second "
              f"(six a node and pair)", flush=True)
        for nt in (int(x) for x in a.thetas.split(",")):
            theta = THETA[:nt]
            tag = f"{tag0} n_theta = {nt}"
            et = ra.EdgeTree(parent, bl)
            whole = timed(lambda: et.diversity(masses, S, theta))
            res = et.diversity(masses, S, theta).values
            torch.cuda.synchronize()
            print(f"{tag} rk_diversity_device        {fmt(whole)}  workspace {et.diversity_work_bytes(S, nt) / 2**20:9.1f} MiB", flush=True)
            et.close()
            t = with_dev("RK_DIVERSITY_STEPS", (7, 3, 1), lambda et: et.diversity(masses, S, theta))
            kern = t[3][0] - t[1][0]
            ops = half_edges * (47.0 + (31.0 if nt else 0.0) + 72.0 * nt)
            print(f"{tag} clade_masses_kernel        {fmt(t[1])}", flush=True)
            print(f"{tag} diversity_kernel           {kern * 1e3:10.2f} us  {ops / (kern * 1e-3) / 1e12 if kern > 0 else 0.0:7.3f} T binary64 operations a second, "
                  f"{(B * S * 24.0) / (kern * 1e-3) / 1e12 if kern > 0 else 0.0:6.3f} TB/s of masses, clade sums and h read", flush=True)
            print(f"{tag} diversity_reduce_kernel    {(t[7][0] - t[3][0]) * 1e3:10.2f} us", flush=True)
            if not a.no_host and nt == 4:
                t0 = time.perf_counter()
                H = ra.diversity_host(parent, bl, hm, S, theta, threads=16).values
                dt = time.perf_counter() - t0
                same = bool((res.cpu().numpy().view(np.uint64) == H.view(np.uint64)).all())
                print(f"{tag} rk_diversity_host, 16 threads {dt * 1e3:11.1f} ms: {dt * 1e3 / whole[0]:8.1f} x the device call; the same bits: {same}", flush=True)
        del sample, masses
    db.close()
    del out
