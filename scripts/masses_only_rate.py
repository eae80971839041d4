"""Developer measurement: profile-only placement (rk_place_batch*_masses) against the full host path followed by the
host sum, PCIe included, in one process.  Per database (C2: 999 branches, T64k: 65 535) and per input (packed records, characters;
pageable, page-locked), alternately:
    full          rk_place_batch_packed / rk_place_batch into reused result arrays, then rk_masses_accumulate_host (16 threads)
    profile-only  rk_place_batch_packed_masses / rk_place_batch_masses
--runs timed calls each after two untimed ones; medians with min .. max, 10^6 reads/s.  The words of both sides are compared.

--driver N: rk_place --timing on a FASTA of N uniform reads on C2 (the file of scripts/f2j_rate.py), `--masses-only` against
`--out ... --masses ...`, best of three runs each; both JSON lines are printed.

    python scripts/masses_only_rate.py [--reads 10000000] [--runs 5] [--configs C2,T64k] [--driver 4000000] >> profiles/masses_only_rate.txt
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import rappas_amd as ra
from rappas_amd import build, hostio, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--configs", default="C2,T64k")
ap.add_argument("--driver", type=int, default=0, metavar="N", help="also the driver comparison on a FASTA of N reads (C2)")
a = ap.parse_args()
n, K = a.reads, 7
print(f"# {n} reads of 150 bases, keep_at_most {K}; {os.cpu_count()} cpus visible, {len(os.sched_getaffinity(0))} usable; "
      f"2 untimed + {a.runs} timed calls a side, alternating; 10^6 reads/s, median (min .. max)", flush=True)


def alternate(full, only):
    for _ in range(2):
        full(), only()
    tf, to = [], []
    for _ in range(a.runs):
        t0 = time.perf_counter(); full(); t1 = time.perf_counter(); only(); t2 = time.perf_counter()
        tf.append(t1 - t0); to.append(t2 - t1)
    return tf, to


def line(tag, tf, to):
    rf, ro = sorted(n / t / 1e6 for t in tf), sorted(n / t / 1e6 for t in to)
    mf, mo = statistics.median(rf), statistics.median(ro)
    verdict = "above the full path's spread" if mo > rf[-1] else "within the full path's spread" if mo >= rf[0] else "BELOW the full path's spread"
    print(f"{tag:52s} full {mf:7.1f} ({rf[0]:7.1f} .. {rf[-1]:7.1f})   profile-only {mo:7.1f} ({ro[0]:7.1f} .. {ro[-1]:7.1f})   x{mo / mf:5.2f}, {verdict}", flush=True)


seq, off = synth.make_reads(4, n, 150, seed=1)
for cfg in a.configs.split(","):
    sdb = synth.make_config_db(cfg, seed=42)
    B = sdb.n_branches
    db = ra.PhyloKmerDB.from_synth(sdb)
    pp = ra.PlacementProcess(db)
    packed, _, _ = pp.pack_reads_host(seq, off)
    weights = np.ones(n, np.uint32)
    mk = lambda alloc: ra.Placements(alloc(n, np.uint8), alloc((n, K), np.uint16), alloc((n, K), np.float32), alloc((n, K), np.float64), alloc(n, np.uint32), {})
    for memory in ("pageable", "page-locked"):
        if memory == "pageable":
            out, pk, sq, so, w, fo = mk(np.zeros), packed, seq, off, weights, np.zeros(n, np.uint32)
        else:
            out = mk(ra.host_alloc)
            pk, sq, so, w, fo = (ra.host_alloc(x.shape, x.dtype) for x in (packed, seq, off, weights, np.zeros(n, np.uint32)))
            pk[:], sq[:], so[:], w[:] = packed, seq, off, weights
        words = {}

        def full_packed():
            pp.processQueriesPacked(pk, fixed_len=150, out=out, keepAtMost=K)
            words["full"] = ra.accumulate_masses_host(B, out, w, threads=16)

        def only_packed():
            words["only"] = pp.processQueriesPackedMasses(pk, fixed_len=150, weights=w, flags_out=fo, keepAtMost=K)[0]

        def full_chars():
            pp.processQueries(sq, so, out=out, keepAtMost=K)
            words["full"] = ra.accumulate_masses_host(B, out, w, threads=16)

        def only_chars():
            words["only"] = pp.processQueriesMasses(sq, so, weights=w, flags_out=fo, keepAtMost=K)[0]

        for what, f, o in (("packed records", full_packed, only_packed), ("characters", full_chars, only_chars)):
            tf, to = alternate(f, o)
            assert np.array_equal(words["full"], words["only"]) and np.array_equal(fo, out.flags)
            line(f"{cfg} ({B} branches), {what}, {memory}", tf, to)
        del out, pk, sq, so, w, fo
    db.close()

if a.driver:
    m = a.driver
    sdb = synth.make_config_db("C2", seed=42)
    db = ra.PhyloKmerDB.from_synth(sdb)
    exe = build.build_host_tools()
    threads = max(1, min(32, len(os.sched_getaffinity(0))))
    d = tempfile.mkdtemp(prefix="rk_mo_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        img = os.path.join(d, "db.rkimg")
        db.save(img, user=hostio.tree_to_blob(hostio.parse_newick(synth.make_newick(sdb.n_branches, seed=3))))
        db.close()
        hw = len(str(m - 1))
        rec = np.empty((m, 2 + hw + 1 + 150 + 1), np.uint8)
        rec[:, 0], rec[:, 1] = ord(">"), ord("r")
        idx = np.arange(m)
        for j in range(hw):
            rec[:, 2 + hw - 1 - j] = ord("0") + (idx // 10 ** j) % 10
        rec[:, 2 + hw] = ord("\n")
        rec[:, 3 + hw:3 + hw + 150] = seq[:m * 150].reshape(m, 150)
        rec[:, -1] = ord("\n")
        fa = os.path.join(d, "q.fasta")
        rec.tofile(fa)
        common = [exe, "--dbimage", img, "--fasta", fa, "--keep-at-most", str(K), "--threads", str(threads), "--logs", os.path.join(d, "logs"), "--timing"]
        sides = (("full", ["--out", os.path.join(d, "q.jplace"), "--masses", os.path.join(d, "full.tsv")], "fasta_to_jplace_s"),
                 ("masses-only", ["--masses-only", os.path.join(d, "only.tsv")], "fasta_to_masses_s"))
        best = {}
        for _ in range(3):
            for name, args, key in sides:
                t0 = time.perf_counter()
                r = subprocess.run(common + args, capture_output=True, text=True, timeout=600)
                wall = time.perf_counter() - t0
                if r.returncode != 0:
                    raise RuntimeError(r.stderr[-300:])
                t = json.loads(r.stdout.strip().splitlines()[-1])
                t["process_wall_s"] = round(wall, 3)
                if name not in best or t[key] < best[name][key]:
                    best[name] = t
        same = open(os.path.join(d, "full.tsv"), "rb").read() == open(os.path.join(d, "only.tsv"), "rb").read()
        print(f"# rk_place --timing, {m} reads on C2, {threads} threads, best of 3 (the --masses table is written after fasta_to_jplace_s is taken; "
              f"process_wall_s has it, with the database load); tables byte-identical: {same}")
        for name, _, key in sides:
            print(f"{name:12s} {m / best[name][key] / 1e6:7.2f} 10^6 reads/s by {key}   {json.dumps(best[name])}", flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
