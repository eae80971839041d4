"""Device-side cost of the edge statistics (rk_edgestat_device) at S = 64, 1 024 and 4 096 samples and F = 0, 1 and 8
metadata columns on C2's tree (999 branches) and on T64k's (65 535), in the manner of scripts/diversity_rate.py and on the same kind
of buffers: the sample buffers come from a synthetic batch placed on the configuration's database, its reads dealt to the samples at
random.  Per shape: the whole call on the product build; its kernels one by one from the developer build, with RK_EDGESTAT_STEPS
leaving kernels out from the back -- the differences are the kernels' shares: clade_masses_kernel, edgestat_profiles_kernel, the start
and the column prelude, edgestat_edge_kernel --; the edge kernel's rate over the 2 * B * S doubles it must read; a device-to-device
copy of as many doubles, the byte floor; and rk_edgestat_host at 16 threads (for F = 1).  The section `crossover` times the edge
kernel alone in both ranking forms (RK_EDGESTAT_COUNT_MAX on the developer build: 1024 = every row by counting, 0 = every row by
the sort) at sample counts on both sides of RK_EDGESTAT_COUNT_MAX_SAMPLES: that constant is the largest S at which counting still
wins.  Warm-up, then HIP events around every call, median (min .. max).  Nothing is gated: recorded numbers.

    python scripts/edgestat_rate.py [--reads 1000000] [--steps 5] [--warmup 2] [--sections crossover,shapes] >> profiles/edgestat_rate.txt
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
from rappas_amd import _lib, edgestats as ES, hostio, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--configs", default="C2,T64k")
ap.add_argument("--samples", default="64,1024,4096")
ap.add_argument("--features", default="0,1,8")
ap.add_argument("--crossover-samples", default="32,64,96,128,192,256,512,1024")
ap.add_argument("--sections", default="crossover,shapes")
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
n, K = a.reads, 7
sections = a.sections.split(",")
print(f"# {torch.cuda.get_device_name(0)}; sample buffers from {n} reads, keep_at_most {K}; {a.warmup} warm-up + {a.steps} timed calls per line, "
      f"HIP events around every call, median (min .. max); RK_EDGESTAT_COUNT_MAX_SAMPLES = {ES.COUNT_MAX_SAMPLES}")


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


def with_dev(settings, call):
    """[timing] of `call(tree)` on the developer build under each of `settings`, dicts of environment knobs; the tree's workspace is
    filled by one whole call first, so that a subset of the kernels finds what the ones left out would have written"""
    product = _lib._LIB
    _lib._LIB = _lib.load_dev()
    t = []
    try:
        et = ra.EdgeTree(parent, bl)
        call(et)
        torch.cuda.synchronize()
        for env in settings:
            os.environ.update({k: str(v) for k, v in env.items()})
            t.append(timed(lambda: call(et)))
            for k in env:
                os.environ.pop(k, None)
        et.close()
    finally:
        _lib._LIB = product
    return t


def sample_buffer(S):
    sample = torch.randint(0, S, (n,), dtype=torch.int32, device=dev, generator=gen)
    masses = pp.accumulate_masses_samples(out, S, sample)
    torch.cuda.synchronize()
    return masses


def metadata(S, F):
    rng = np.random.default_rng(S * 16 + F)
    return torch.from_numpy(np.stack([rng.normal(size=S) if f % 2 == 0 else rng.integers(0, 6, S).astype(np.float64) for f in range(F)]).reshape(F, S)).to(dev)


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
    if "crossover" in sections:
        for S in (int(s) for s in a.crossover_samples.split(",")):
            masses, meta = sample_buffer(S), metadata(S, 1)
            t = with_dev([dict(RK_EDGESTAT_STEPS=8, RK_EDGESTAT_COUNT_MAX=1024), dict(RK_EDGESTAT_STEPS=8, RK_EDGESTAT_COUNT_MAX=0)], lambda et: ES.edgestat(et, masses, S, meta))
            print(f"{cfg} ({B}) S = {S:5d} F = 1 edgestat_edge_kernel  counting {fmt(t[0])}   sorting {fmt(t[1])}   counting / sorting {t[0][0] / t[1][0]:6.2f}", flush=True)
            del masses
    if "shapes" in sections:
        for S in (int(s) for s in a.samples.split(",")):
            masses = sample_buffer(S)
            hm = masses.cpu().numpy().view(np.uint64)
            src = torch.empty(2 * B * S, dtype=torch.float64, device=dev).normal_()
            dst = torch.empty_like(src)
            floor = timed(lambda: dst.copy_(src))
            del src, dst
            tag0 = f"{cfg} ({B}) S = {S:5d}"
            print(f"{tag0} device-to-device copy of 2 B S doubles (the byte floor) {fmt(floor)}", flush=True)
            for F in (int(x) for x in a.features.split(",")):
                meta = metadata(S, F)
                tag = f"{tag0} F = {F}"
                et = ra.EdgeTree(parent, bl)
                whole = timed(lambda: ES.edgestat(et, masses, S, meta))
                raw, info = ES.edgestat(et, masses, S, meta)
                torch.cuda.synchronize()
                need = _lib.load().rk_edgestat_work_bytes(et.handle, S, F)
                print(f"{tag} rk_edgestat_device         {fmt(whole)}  workspace {need / 2**20:9.1f} MiB  form: {'counting' if S <= ES.COUNT_MAX_SAMPLES else 'sorting'}", flush=True)
                et.close()
                t = with_dev([dict(RK_EDGESTAT_STEPS=v) for v in (1, 3, 7, 15)], lambda et: ES.edgestat(et, masses, S, meta))
                edge = t[3][0] - t[2][0]
                print(f"{tag} clade_masses_kernel        {fmt(t[0])}", flush=True)
                print(f"{tag} edgestat_profiles_kernel   {(t[1][0] - t[0][0]) * 1e3:10.2f} us", flush=True)
                print(f"{tag} start and column prelude   {(t[2][0] - t[1][0]) * 1e3:10.2f} us", flush=True)
                print(f"{tag} edgestat_edge_kernel       {edge * 1e3:10.2f} us  {(2.0 * B * S * 8) / (edge * 1e-3) / 1e12 if edge > 0 else 0.0:6.3f} TB/s of rows read, "
                      f"{edge / floor[0] if floor[0] > 0 else 0.0:7.1f} x the copy", flush=True)
                if not a.no_host and F == 1:
                    t0 = time.perf_counter()
                    H, hinfo = ES.edgestat_host(parent, hm, S, meta.cpu().numpy(), threads=16)
                    dt = time.perf_counter() - t0
                    same = bool((raw.cpu().numpy().view(np.uint64) == H).all() and (info.cpu().numpy().view(np.uint32) == hinfo).all())
                    print(f"{tag} rk_edgestat_host, 16 threads {dt * 1e3:11.1f} ms: {dt * 1e3 / whole[0]:8.1f} x the device call; the same bits: {same}", flush=True)
                del meta
            del masses, hm
    db.close()
    del out
