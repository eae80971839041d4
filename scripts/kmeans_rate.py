"""Device-side cost of the phylogenetic k-means (rk_kmeans_device) at S = 64 and 1 024 samples and k = 2, 8 and 64
clusters on C2's tree (999 branches) and on T64k's (65 535), in the manner of scripts/squash_rate.py and on the same buffers: the
sample buffers come from a synthetic batch placed on the configuration's database, its reads dealt to the samples at random.  The
whole call (farthest-first seeds, at most 100 rounds) is timed on the product build.  The kernels' times a round come from the
developer build: one round (max_rounds = 1) from the caller's seeds 0 .. k - 1, so that every kernel of the round runs exactly once
and no farthest-first step stands in front of it, with RK_KMEANS_STEPS leaving kernels out from the back -- the differences are the
kernels' shares.  RK_KMEANS_KC forces the rung of the distance kernel's ladder: the k = 8 step with 8 running sums a thread (U and V
streamed once) stands beside the same step as eight single-centroid groups (KC = 1: U and V streamed eight times), with 16 bytes a
node for every sample and centroid group as the bytes a second, and beside squash_row_kernel's time a step as profiles/squash_rate.txt
records it.  Beside them rk_kmeans_host at 16 threads on the same buffer, once, for k = 8.  Warm-up, then HIP events around every
call, median (min .. max).  Nothing is gated: recorded numbers.

    python scripts/kmeans_rate.py [--reads 1000000] [--steps 5] [--warmup 2] >> profiles/kmeans_rate.txt
"""
import argparse
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rappas_amd as ra
from rappas_amd import _lib, hostio, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--configs", default="C2,T64k")
ap.add_argument("--samples", default="64,1024")
ap.add_argument("--clusters", default="2,8,64")
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


def squash_row_step(cfg, S):
    """squash_row_kernel's microseconds a step as profiles/squash_rate.txt records them for this shape, or None"""
    try:
        text = open(os.path.join(ROOT, "profiles", "squash_rate.txt")).read()
    except OSError:
        return None
    m = re.search(rf"^{cfg} \(\d+\) S = +{S} squash_row_kernel .* ([0-9.]+) us a step", text, re.M)
    return float(m.group(1)) if m else None


# what a streaming copy reaches here: 1 GiB device to device, read and written once each
src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
dst = torch.empty_like(src)
copy = timed(lambda: dst.copy_(src))
copy_rate = 2 * src.numel() / (copy[0] * 1e-3)
print(f"streaming copy, 1 GiB device to device {fmt(copy)}  {copy_rate / 1e12:6.2f} TB/s read + written", flush=True)
del src, dst

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
        row_step = squash_row_step(cfg, S)
        for k in (int(x) for x in a.clusters.split(",")):
            tag = f"{cfg} ({B}) S = {S:5d} k = {k:2d}"
            # ---- the product build: the whole call ----
            et = ra.EdgeTree(parent, bl)
            whole = timed(lambda: et.kmeans(masses, S, k))
            res = et.kmeans(masses, S, k, centroids=True)
            torch.cuda.synchronize()
            info = res.info.cpu().numpy().view(np.uint32)
            print(f"{tag} rk_kmeans_device           {fmt(whole)}  k_eff {info[0]}, {info[1]} active, {info[2]} rounds, converged {info[3] & 1}, "
                  f"workspace {et.kmeans_work_bytes(S, k) / 2**20:9.1f} MiB", flush=True)
            et.close()
            # ---- the developer build: one round from the caller's seeds, kernels left out from the back ----
            product = _lib._LIB
            _lib._LIB = _lib.load_dev()
            t = {}
            try:
                et = ra.EdgeTree(parent, bl)
                seeds = list(range(k))
                one = et.kmeans(masses, S, k, 1, seeds=seeds)
                torch.cuda.synchronize()
                if int(one.info.cpu()[3]) >> 1:
                    print(f"{tag} one of the samples 0 .. {k - 1} holds no mass: no round to time", flush=True)
                else:
                    for steps in (31, 15, 7, 3, 1):
                        os.environ["RK_KMEANS_STEPS"] = str(steps)
                        t[steps] = timed(lambda: et.kmeans(masses, S, k, 1, seeds=seeds))
                    ladder = {}
                    for kc in (1, 2, 4, 8):
                        if kc > 1 and kc >= 2 * k:
                            continue
                        os.environ["RK_KMEANS_KC"] = str(kc)
                        os.environ["RK_KMEANS_STEPS"] = "3"
                        ladder[kc] = timed(lambda: et.kmeans(masses, S, k, 1, seeds=seeds))[0] - t[1][0]
                    os.environ.pop("RK_KMEANS_KC")
                    os.environ.pop("RK_KMEANS_STEPS")
                et.close()
            finally:
                os.environ.pop("RK_KMEANS_KC", None)
                os.environ.pop("RK_KMEANS_STEPS", None)
                _lib._LIB = product
            if t:
                print(f"{tag} one round, caller's seeds  {fmt(t[31])}", flush=True)
                for name, hi, lo in (("kmeans_update_kernel", 31, 15), ("kmeans_assign_kernel", 15, 7), ("kmeans_reduce_kernel", 7, 3), ("kmeans_dist_kernel", 3, 1)):
                    print(f"{tag} {name:26s} {(t[hi][0] - t[lo][0]) * 1e3:10.2f} us a round", flush=True)
                print(f"{tag} profiles, start, gather    {fmt(t[1])}", flush=True)
                for kc, d in ladder.items():
                    groups = (k + kc - 1) // kc
                    rate = 16.0 * B * S * groups / (d * 1e-3) if d > 0 else 0.0
                    line = (f"{tag} distance step, KC = {kc}: {groups:2d} group(s) {d * 1e3:10.2f} us  {rate / 1e12:6.3f} TB/s of U and V streamed "
                            f"({rate / copy_rate * 100:5.1f} % of the streaming copy), {16.0 * B * S * k / (d * 1e-3) / 1e12 if d > 0 else 0.0:7.3f} TB/s a centroid")
                    print(line, flush=True)
                if k == 8 and 1 in ladder and 8 in ladder and ladder[8] > 0:
                    print(f"{tag} eight single-centroid groups / one group of eight: {ladder[1] / ladder[8]:5.2f} x", flush=True)
                if row_step is not None:
                    print(f"{tag} squash_row_kernel (profiles/squash_rate.txt) {row_step:10.2f} us a step, one centroid", flush=True)
            # ---- the host twin at 16 threads, once ----
            if not a.no_host and k == 8:
                hm = masses.cpu().numpy().view(np.uint64)
                t0 = time.perf_counter()
                H = ra.kmeans_host(parent, bl, hm, S, k, threads=16)
                dt = time.perf_counter() - t0
                same = all(bool((np.ascontiguousarray(getattr(res, f).cpu().numpy()).view(np.uint8) == np.ascontiguousarray(getattr(H, f)).view(np.uint8)).all())
                           for f in ("assign", "dist", "sizes", "within", "info", "centroids"))
                print(f"{tag} rk_kmeans_host, 16 threads {dt * 1e3:11.1f} ms: {dt * 1e3 / whole[0]:8.1f} x the device call; the same bits: {same}", flush=True)
        del sample, masses
    db.close()
    del out
