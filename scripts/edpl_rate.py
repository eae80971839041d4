"""Device-side cost of the EDPL pass (rk_edpl_device) over the result set of one batch, keep_at_most 7, in the manner of
scripts/masses_rate.py: on C2's tree (999 branches: the tables in the LDS) and on T64k's (65 535: the tables in global memory), for
uniform reads (bench.py's) and clade-shaped ones (synth.make_clade_db / make_clade_reads), and on a caterpillar of 65 535 nodes with
a synthetic result set whose rows are spread over the whole chain (every pair far apart, the deepest tree there is).  Beside each:
rk_masses_accumulate_device on the same result set -- the yardstick: a pass over the same bytes --, the placement of the same batch,
rk_edpl_host at 16 threads, once, with the check that device and host give the same bits, and, where the tables are in the LDS, the
other form of the kernel on the same tree (the developer build with RK_EDPL_LDS_BYTES=0).  Warm-up, then HIP events around
every call, median (min .. max).  One JSON line per case (prefixed `json `) and the text lines.  Nothing is gated: recorded numbers.

    python scripts/edpl_rate.py [--reads 10000000] [--steps 10] [--warmup 5] >> profiles/edpl_rate.txt
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
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--configs", default="C2,T64k")
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
n, K = a.reads, 7
print(f"# {torch.cuda.get_device_name(0)}; {n} reads, keep_at_most {K}; {a.warmup} warm-up + {a.steps} timed calls per line, HIP events around every call, "
      f"median (min .. max)")


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
    return f"{t[0]:8.3f} ms ({t[1]:8.3f} .. {t[2]:8.3f})"


def report(tag, pp, parent, bl, out, place=None):
    """the EDPL pass, the edge-mass pass and the host twin on one result set"""
    B = len(parent)
    et = ra.EdgeTree(parent, bl)
    m = torch.zeros(ra.masses_words(B), dtype=torch.int64, device=dev)
    nbytes = n * (1 + 10 * K)
    rows = int(out["n_rows"].sum(dtype=torch.int64).item())
    pairs = int((out["n_rows"].to(torch.int64) * (out["n_rows"].to(torch.int64) - 1) // 2).sum().item())
    form = "tables in the LDS" if et.edpl_lds_bytes() else "tables in global memory"
    edpl = timed(lambda: et.edpl(out, K))
    mass = timed(lambda: pp.accumulate_masses(out, masses=m))
    got = et.edpl(out, K)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    print(f"{tag:30s} rk_edpl_device              {fmt(edpl)}  {nbytes / edpl[0] / 1e6:6.0f} GB/s of result set, {pairs / edpl[0] / 1e6:7.2f} G pairs/s  "
          f"[{form}; {rows / n:.2f} rows and {pairs / n:.2f} pairs a read; mean EDPL {float(got.mean()):.4g}]", flush=True)
    print(f"{tag:30s} rk_masses_accumulate_device {fmt(mass)}  {nbytes / mass[0] / 1e6:6.0f} GB/s of result set: the EDPL pass takes {edpl[0] / mass[0]:5.2f} x its time", flush=True)
    rec = dict(case=tag, branches=B, reads=n, form=form, rows_per_read=rows / n, pairs_per_read=pairs / n, edpl_ms=edpl[0], masses_ms=mass[0], edpl_over_masses=edpl[0] / mass[0])
    if et.edpl_lds_bytes():  # the other form on the same tree: the developer build with the limit at 0
        product = _lib._LIB
        _lib._LIB = _lib.load_dev()
        os.environ["RK_EDPL_LDS_BYTES"] = "0"
        try:
            eg = ra.EdgeTree(parent, bl)
            assert eg.edpl_lds_bytes() == 0
            glob = timed(lambda: eg.edpl(out, K))
            eg.close()
        finally:
            os.environ.pop("RK_EDPL_LDS_BYTES")
            _lib._LIB = product
        print(f"{tag:30s}   tables in global memory     {fmt(glob)}  (developer build, RK_EDPL_LDS_BYTES=0): the LDS form takes {edpl[0] / glob[0]:5.2f} x its time", flush=True)
        rec.update(edpl_global_form_ms=glob[0])
    if place:
        print(f"{tag:30s} placement of the batch     {fmt(place)}  the EDPL pass adds {100 * edpl[0] / place[0]:5.2f} %", flush=True)
        rec.update(place_ms=place[0])
    if not a.no_host:
        n_rows, branch, lwr = out["n_rows"].cpu().numpy(), out["branch"].cpu().numpy().view(np.uint16), out["lwr"].cpu().numpy()
        t0 = time.perf_counter()
        H = ra.edpl_host(parent, bl, K, n_rows, branch, lwr, threads=16)
        dt = time.perf_counter() - t0
        same = bool((H.view(np.uint64) == got.view(np.uint64)).all())
        print(f"{tag:30s} rk_edpl_host, 16 threads    {dt * 1e3:8.1f} ms: {dt * 1e3 / edpl[0]:7.1f} x the device call; the same bits: {same}", flush=True)
        rec.update(host_ms=dt * 1e3, same_bits=same)
    print("json " + json.dumps(rec), flush=True)
    et.close()
    return edpl[0]


def empty_out():
    return dict(n_rows=torch.empty(n, dtype=torch.uint8, device=dev), branch=torch.empty((n, K), dtype=torch.int16, device=dev),
                score=torch.empty((n, K), dtype=torch.float32, device=dev), lwr=torch.empty((n, K), dtype=torch.float64, device=dev),
                flags=torch.empty(n, dtype=torch.int32, device=dev))


def tree_of(B):
    tree = hostio.parse_newick(synth.make_newick(B, seed=6))
    return (np.array([nd.parent.id if nd.parent is not None else -1 for nd in tree.nodes], np.int32), np.array([nd.bl for nd in tree.nodes], np.float32))


for cfg in a.configs.split(","):
    alphabet, k, leaves, n_keys, n_entries, rlen, _ = synth.CONFIGS[cfg]
    # ---- uniform: bench.py's database and reads ----
    sdb = synth.make_config_db(cfg, seed=42)
    B = sdb.n_branches
    parent, bl = tree_of(B)
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
    place = timed(lambda: pp.place_packed(packed, fixed_len=rlen, out=out, keepAtMost=K))
    t_random = report(f"{cfg} ({B}) uniform", pp, parent, bl, out, place)
    del packed
    if B == 65535:
        # ---- the deepest tree of that size: a caterpillar, every read's rows spread over the whole chain (no placement behind it) ----
        width = B // K
        out["n_rows"].fill_(K)
        ids = torch.arange(K, device=dev)[None, :] * width + torch.randint(0, width, (n, K), device=dev, generator=gen)
        out["branch"].copy_(((ids + 32768) % 65536 - 32768).to(torch.int16))  # (the bits of the unsigned 16-bit id)
        del ids
        out["lwr"].fill_(1.0 / K)
        t_rand_spread = report(f"{cfg} ({B}) random tree, spread rows", pp, parent, bl, out)
        cat_parent = np.arange(-1, B - 1, dtype=np.int32)
        t_cat = report(f"caterpillar ({B}), spread rows", pp, cat_parent, np.full(B, 0.01, np.float32), out)
        print(f"caterpillar over the random tree of the same size, the same rows: {t_cat / t_rand_spread:5.2f} x (over its uniform batch: {t_cat / t_random:5.2f} x)", flush=True)
    db.close()
    # ---- clade-shaped: the same tree, rows of a stretch of the genome share a neighbourhood ----
    cdb_s, genome = synth.make_clade_db(k=k, n_branches=B)
    nc = min(2_000_000, n)
    cseq, coff = synth.make_clade_reads(genome, nc, rlen)
    cdb = ra.PhyloKmerDB.from_synth(cdb_s)
    cpp = ra.PlacementProcess(cdb)
    cpk = torch.from_numpy(cpp.pack_reads_host(cseq, coff)[0].view(np.int32)).to(dev)
    cpk = cpk.repeat((n + nc - 1) // nc, 1)[:n].contiguous()
    place = timed(lambda: cpp.place_packed(cpk, fixed_len=rlen, out=out, keepAtMost=K))
    report(f"{cfg} ({B}) clade", cpp, parent, bl, out, place)
    cdb.close()
    del cpk, out
