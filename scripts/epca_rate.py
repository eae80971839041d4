"""Device-side cost of the edge PCA (rk_epca_device) at S = 64 and 1 024 samples on C2's tree (999 branches) and on
T64k's (65 535), k = 5 components, 200 iterations, in the manner of scripts/kr_rate.py and scripts/squash_rate.py: the sample buffers
come from a synthetic batch placed on the configuration's database, its reads dealt to the samples at random.  The whole call is
timed on the product build, beside rk_kr_distances_device and rk_squash_device on the same buffer (they must measure as before), and
rk_epca_host at 16 threads, once.  The developer build (RK_EPCA_STEPS, RK_KR_STEPS) then runs single steps on the workspace a whole
call has left: the centring pass, the Gram kernel (with its reduce where the chunk partials go through the workspace), the
iterations, the results with the loadings, and kr_pairs_kernel on the same shape.  For the Gram kernel: terms a second (S (S + 1) / 2
pairs x B nodes) and the share of the unfused FP64 vector rate (39.3e12 operations a second, two a term).  Warm-up, then HIP events
around every call, median (min .. max).  One JSON line per shape (prefixed `json `) and the text lines.  Nothing is gated: recorded
numbers.

    python scripts/epca_rate.py [--reads 1000000] [--steps 10] [--warmup 10] >> profiles/epca_rate.txt
"""
import argparse
import json
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
ap.add_argument("--components", type=int, default=5)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--no-squash", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
n, K, k, iters = a.reads, 7, a.components, a.iters
FP64_VECTOR = 39.3e12
print(f"# {torch.cuda.get_device_name(0)}; sample buffers from {n} reads, keep_at_most {K}; k = {k}, iters = {iters}; {a.warmup} warm-up + {a.steps} timed calls "
      f"per line, HIP events around every call, median (min .. max)")


def timed(step, steps=None, warmup=None):
    steps, warmup = steps or a.steps, a.warmup if warmup is None else warmup
    step()
    torch.cuda.synchronize()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in evs:
        e0.record()
        step()
        e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in evs]
    return statistics.median(ms), min(ms), max(ms)


def fmt(t):
    return f"{t[0]:10.3f} ms ({t[1]:10.3f} .. {t[2]:10.3f})"


for cfg in a.configs.split(","):
    alphabet, kk, leaves, n_keys, n_entries, rlen, _ = synth.CONFIGS[cfg]
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
        rec = dict(config=cfg, branches=B, samples=S, k=k, iters=iters)
        # ---- the product build: the whole call, and the two calls that must measure as before ----
        et = ra.EdgeTree(parent, bl)
        whole = timed(lambda: et.epca(masses, S, k, iters))
        kr = timed(lambda: et.kr_distances(masses, S))
        raw, info = et.epca(masses, S, k, iters)
        f = ra.epca_finish(B, S, k, raw, info)
        raw = raw.cpu().numpy()
        print(f"{tag} rk_epca_device            {fmt(whole)}  n_active {f.n_active}, k_eff {f.k_eff}, workspace {et.epca_work_bytes(S, k) / 2**20:9.1f} MiB", flush=True)
        print(f"{tag}   eigenvalue shares {' '.join('%.4f' % x for x in f.share)}; residual / eigenvalue_0 {' '.join('%.1e' % (x / f.eigenvalue[0]) for x in f.residual)}", flush=True)
        print(f"{tag} rk_kr_distances_device    {fmt(kr)}", flush=True)
        rec.update(epca_ms=whole[0], kr_ms=kr[0], n_active=f.n_active, k_eff=f.k_eff)
        if not a.no_squash:
            sq = timed(lambda: et.squash(masses, S), steps=3, warmup=1)
            print(f"{tag} rk_squash_device          {fmt(sq)}  (1 warm-up + 3 timed)", flush=True)
            rec.update(squash_ms=sq[0])
        et.close()
        # ---- the developer build: single steps on the workspace a whole call has left ----
        product = _lib._LIB
        _lib._LIB = _lib.load_dev()
        try:
            et = ra.EdgeTree(parent, bl)
            et.kr_distances(masses, S)
            os.environ["RK_KR_STEPS"] = "4"
            pairs = timed(lambda: et.kr_distances(masses, S))
            os.environ.pop("RK_KR_STEPS")
            et.epca(masses, S, k, iters)
            t = {}
            for name, steps in (("gram", 4), ("iterations", 8), ("results_loadings", 16), ("clade_profiles_start", 1), ("centre", 2)):
                os.environ["RK_EPCA_STEPS"] = str(steps)
                t[name] = timed(lambda: et.epca(masses, S, k, iters))
            os.environ.pop("RK_EPCA_STEPS")
            et.close()
        finally:
            _lib._LIB = product
            os.environ.pop("RK_KR_STEPS", None)
            os.environ.pop("RK_EPCA_STEPS", None)
        terms = S * (S + 1) / 2 * B
        g = t["gram"][0] * 1e-3
        print(f"{tag} epca_gram_kernel (+ reduce) {fmt(t['gram'])}  {terms / g / 1e12:7.3f} T terms/s, {2 * terms / g / FP64_VECTOR * 100:5.1f} % of the FP64 vector rate", flush=True)
        p = pairs[0] * 1e-3
        print(f"{tag} kr_pairs_kernel (+ reduce)  {fmt(pairs)}  {terms / p / 1e12:7.3f} T terms/s, {3 * terms / p / FP64_VECTOR * 100:5.1f} % of the FP64 vector rate (three a term)", flush=True)
        print(f"{tag} epca_centre_kernel          {fmt(t['centre'])}  {24.0 * B * S / (t['centre'][0] * 1e-3) / 1e12:6.3f} TB/s (U and V read, Xc written)", flush=True)
        print(f"{tag} {iters} iterations            {fmt(t['iterations'])}  {t['iterations'][0] / iters * 1e3:8.2f} us an iteration (multiply + orth)", flush=True)
        print(f"{tag} results and loadings        {fmt(t['results_loadings'])}", flush=True)
        print(f"{tag} clade sums, profiles, start {fmt(t['clade_profiles_start'])}", flush=True)
        rec.update(gram_ms=t["gram"][0], kr_pairs_ms=pairs[0], gram_terms_per_s=terms / g, gram_share_fp64_vector=2 * terms / g / FP64_VECTOR, centre_ms=t["centre"][0],
                   iteration_us=t["iterations"][0] / iters * 1e3, results_loadings_ms=t["results_loadings"][0], clade_profiles_start_ms=t["clade_profiles_start"][0])
        # ---- the host twin at 16 threads, once ----
        if not a.no_host:
            hm = masses.cpu().numpy().view(np.uint64)
            t0 = time.perf_counter()
            H, hi = ra.epca_host(parent, bl, hm, S, k, iters, threads=16)
            dt = time.perf_counter() - t0
            same = hi.tolist() == [f.n_active, f.k_eff] and bool((H.view(np.uint64) == raw.view(np.uint64)).all())
            print(f"{tag} rk_epca_host, 16 threads   {dt * 1e3:11.1f} ms: {dt * 1e3 / whole[0]:8.1f} x the device call; the same bits: {same}", flush=True)
            rec.update(host_ms=dt * 1e3, same_bits=same)
        print("json " + json.dumps(rec), flush=True)
        del sample, masses
    db.close()
    del out
