"""GPU (-m gpu): profile-only placement -- rk_place_batch_masses / rk_place_batch_packed_masses (the masses sink of the
host path) -- for equality of all 2 * B + 4 words with the numpy restatement of the definition (tests/masses_ref.py) over the result
set of the corresponding existing, oracle-checked entry point; flags and counters against that call's.  Nothing expected comes from
the new calls.  Child processes run under a time limit."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, hostio, synth
from tests import masses_ref as MR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300
N, K = 5000, 7
POISON = np.uint64(0xA5A5A5A5DEADBEEF)
FLAG_POISON = np.uint32(0xDEADBEEF)


@functools.lru_cache(maxsize=None)
def database(name):
    if name == "C1":
        return synth.make_config_db("C1")
    if name == "T20k":
        return synth.make_db(4, 6, 20001, 300, 1500, seed=20001)
    from tests.test_gpu_translate import planted_case
    return planted_case(3)[0]


@functools.lru_cache(maxsize=None)
def reads(name):
    """5 000 ragged reads with ambiguity codes, unsupported characters and reads shorter than k; the planted DNA reads for the
    protein database"""
    if name == "protein":
        from tests.test_gpu_translate import planted_case
        from tests import translate_ref as TR
        seq, off = TR.batch(planted_case(3)[1])
    else:
        seq, off = synth.make_reads(4, N, 150, seed=11, amb_rate=0.002, bad_rate=0.01, var_len=148)
    seq, off = np.ascontiguousarray(seq, np.uint8), np.ascontiguousarray(off, np.uint64)
    seq.setflags(write=False)
    off.setflags(write=False)
    return seq, off


def weights_of(n, kind):
    return MR.make_weights(n, kind, seed=4)


def full_call(pp, step, seq, off, packed=None):
    """the existing entry point of a step -> Placements"""
    if step == "translated":
        return pp.processQueriesTranslated(seq, off, keepAtMost=K)
    if step == "packed":
        return pp.processQueriesPacked(packed[0], lens=packed[1], flags=packed[2], seq=seq, seq_off=off, keepAtMost=K)
    if step == "packed_no_chars":
        return pp.processQueriesPacked(packed[0], lens=packed[1], flags=packed[2], keepAtMost=K)
    return pp.processQueries(seq, off, keepAtMost=K, strand=step)


def masses_call(pp, step, seq, off, packed=None, **kw):
    if step == "translated":
        return pp.processQueriesMasses(seq, off, translate=True, keepAtMost=K, **kw)
    if step == "packed":
        return pp.processQueriesPackedMasses(packed[0], lens=packed[1], flags=packed[2], seq=seq, seq_off=off, keepAtMost=K, **kw)
    if step == "packed_no_chars":
        return pp.processQueriesPackedMasses(packed[0], lens=packed[1], flags=packed[2], keepAtMost=K, **kw)
    return pp.processQueriesMasses(seq, off, strand=step, keepAtMost=K, **kw)


def ref_words(B, full, w=None, masses=None):
    return MR.masses_ref(B, full.n_rows, full.branch, full.lwr, w, masses=masses)


def check_flags_seen(name, step, full):
    fl = full.flags
    n = len(fl)
    placed = int((fl & ra.RK_FLAG_PLACED != 0).sum())
    assert 0 < placed < n, (name, step, placed)  # the comparison cannot pass on an empty profile
    assert (fl & ra.RK_FLAG_TOO_SHORT).any() and (fl & ra.RK_FLAG_BAD_CHAR).any() and (fl & ra.RK_FLAG_AMBIGUOUS).any(), (name, step)
    if step in ("reverse", "both"):
        assert (fl & ra.RK_FLAG_REVERSE).any()


def locked(a):
    h = ra.host_alloc(a.shape, a.dtype)
    h[...] = a
    return h


STEPS = [("C1", "forward"), ("C1", "reverse"), ("C1", "both"), ("C1", "packed"), ("C1", "packed_no_chars"), ("T20k", "forward"), ("T20k", "both"),
         ("T20k", "packed"), ("protein", "translated"), ("protein", "forward")]


# ---- 1. steps and inputs ----
@pytest.mark.parametrize("memory", ["pageable", "page_locked"])
@pytest.mark.parametrize("name,step", STEPS)
def test_every_step_equals_the_reference_over_the_existing_call(name, step, memory):
    sdb = database(name)
    B = sdb.n_branches
    seq, off = reads(name)
    if name == "protein" and step == "forward":  # an amino-acid handle placing amino-acid characters: the forward step is not DNA's alone
        seq, off = synth.make_reads(20, 600, 40, seed=3, bad_rate=0.01, var_len=39)
    n = len(off) - 1
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        pp = ra.PlacementProcess(db)
        packed = pp.pack_reads_host(seq, off) if step.startswith("packed") else None
        full = full_call(pp, step, seq, off, packed)
        if not (name == "protein" and step == "forward"):
            check_flags_seen(name, step, full)
        if memory == "page_locked":
            seq, off = locked(seq), locked(off)
            if packed:
                packed = tuple(locked(a) for a in packed)
        for kind in (None, "mixed", "zero"):
            w = weights_of(n, kind)
            want = ref_words(B, full, w)
            wl = w if w is None or memory == "pageable" else locked(w)
            fo = ra.host_alloc(n, np.uint32) if memory == "page_locked" else np.zeros(n, np.uint32)
            fo[:] = FLAG_POISON
            got, flags, counters = masses_call(pp, step, seq, off, packed, weights=wl, flags_out=fo)
            assert got.dtype == np.uint64 and got.shape == (2 * B + 4,)
            assert np.array_equal(got, want), (kind, np.flatnonzero(got != want)[:8])
            assert flags is fo and np.array_equal(flags, full.flags)
            assert counters == full.counters
        assert want[2 * B] == 0 and not want.any()  # (all weights zero: a read adds 0 everywhere)
        assert np.array_equal(got, ra.accumulate_masses_host(B, full, w))
        # flags_out = NULL and counters = NULL
        lib = pp._lib
        p = pp._params(K, 0.01, True, False)
        m = np.zeros(2 * B + 4, np.uint64)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        if step.startswith("packed"):
            chars = (ptr(seq), ptr(off)) if step == "packed" else (None, None)
            rc = lib.rk_place_batch_packed_masses(db.handle, C.byref(p), n, ptr(packed[0]), packed[0].shape[1], ptr(packed[1]), 0, ptr(packed[2]), *chars,
                                                  None, ptr(m), None, None)
        else:
            code = {"forward": 0, "reverse": 1, "both": 2, "translated": 3}[step]
            rc = lib.rk_place_batch_masses(db.handle, C.byref(p), code, n, ptr(seq), ptr(off), None, ptr(m), None, None)
        assert rc == _lib.RK_OK, lib.rk_last_error()
        assert np.array_equal(m, ref_words(B, full))
    finally:
        db.close()


# ---- 2. chunking ----
@pytest.mark.parametrize("name,step", [("C1", "both"), ("T20k", "forward"), ("C1", "packed"), ("protein", "translated")])
def test_five_chunks_over_four_workspaces_give_the_single_chunk_words(name, step, monkeypatch, dev_lib):
    sdb = database(name)
    B = sdb.n_branches
    seq, off = reads("C1") if name == "protein" else reads(name)  # (5 000 reads on every database: five chunks of 1 024)
    n = len(off) - 1
    assert n == N
    w = weights_of(n, "mixed")
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        pp = ra.PlacementProcess(db)
        packed = pp.pack_reads_host(seq, off) if step.startswith("packed") else None
        single, flags1, ct1 = masses_call(pp, step, seq, off, packed, weights=w)
        monkeypatch.setenv("RK_CHUNK_READS", "1024")
        full = full_call(pp, step, seq, off, packed)
        assert (full.n_rows > 0).any()
        for ww in (w, locked(w)):
            got, flags, ct = masses_call(pp, step, seq, off, packed, weights=ww)
            assert np.array_equal(got, single) and np.array_equal(flags, flags1) and ct == ct1
        assert np.array_equal(single, ref_words(B, full, w)) and np.array_equal(flags1, full.flags) and ct1 == full.counters
    finally:
        db.close()


# ---- 3. adding ----
@pytest.mark.parametrize("name", ["C1", "T20k"])
def test_calls_add_into_the_callers_buffer(name):
    sdb = database(name)
    B = sdb.n_branches
    seq, off = reads(name)
    w = weights_of(N, "mixed")
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        pp = ra.PlacementProcess(db)
        full = pp.processQueries(seq, off, keepAtMost=K)
        start = np.arange(2 * B + 4, dtype=np.uint64) * np.uint64(5)
        m = start.copy()
        got, _, _ = pp.processQueriesMasses(seq, off, weights=w, masses=m, keepAtMost=K)
        assert got is m and np.array_equal(m, ref_words(B, full, w, masses=start))
        # two calls over the two halves of the batch give the whole
        cut = 2222
        cb = int(off[cut])
        m = np.zeros(2 * B + 4, np.uint64)
        _, f1, c1 = pp.processQueriesMasses(seq[:cb], off[:cut + 1], weights=np.ascontiguousarray(w[:cut]), masses=m, keepAtMost=K)
        _, f2, c2 = pp.processQueriesMasses(seq[cb:], off[cut:] - off[cut], weights=np.ascontiguousarray(w[cut:]), masses=m, keepAtMost=K)
        assert np.array_equal(m, ref_words(B, full, w))
        assert np.array_equal(np.concatenate([f1, f2]), full.flags)
        assert {k: c1[k] + c2[k] for k in c1} == full.counters
    finally:
        db.close()


# ---- 4. handle reuse ----
def same(a, b):
    return all(np.array_equal(getattr(a, f).view(np.uint8), getattr(b, f).view(np.uint8)) for f in ("n_rows", "branch", "score", "lwr", "flags"))


def test_one_handle_full_then_profile_only_then_full_and_a_fresh_handle():
    sdb = database("C1")
    B = sdb.n_branches
    seq, off = reads("C1")
    db, fresh = ra.PhyloKmerDB.from_synth(sdb), ra.PhyloKmerDB.from_synth(sdb)
    try:
        pp = ra.PlacementProcess(db)
        first = pp.processQueries(seq, off, keepAtMost=K, strand="both")
        got, flags, ct = pp.processQueriesMasses(seq, off, strand="both", keepAtMost=K)
        second = pp.processQueries(seq, off, keepAtMost=K, strand="both")
        assert same(first, second) and first.counters == second.counters
        want = ref_words(B, first)
        assert np.array_equal(got, want) and np.array_equal(flags, first.flags) and ct == first.counters
        # a profile-only call as the very first call of a handle
        got, flags, ct = ra.PlacementProcess(fresh).processQueriesMasses(seq, off, strand="both", keepAtMost=K)
        assert np.array_equal(got, want) and np.array_equal(flags, first.flags) and ct == first.counters
    finally:
        db.close()
        fresh.close()


def test_reserve_host_path_then_profile_only():
    sdb = database("C1")
    seq, off = reads("C1")
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        pp = ra.PlacementProcess(db)
        _lib.check(pp._lib.rk_reserve_host_path(db.handle, K, 150))
        got, flags, _ = pp.processQueriesMasses(seq, off, keepAtMost=K)
        full = pp.processQueries(seq, off, keepAtMost=K)
        assert np.array_equal(got, ref_words(sdb.n_branches, full)) and np.array_equal(flags, full.flags)
    finally:
        db.close()


# ---- 5. error calls ----
def test_error_calls_leave_poisoned_buffers_untouched():
    dna, prot = database("C1"), database("protein")
    seq, off = reads("C1")
    n = 100
    seq, off = np.ascontiguousarray(seq[:int(off[n])]), np.ascontiguousarray(off[:n + 1])
    ddb, pdb = ra.PhyloKmerDB.from_synth(dna), ra.PhyloKmerDB.from_synth(prot)
    try:
        lib = _lib.load()
        pp = ra.PlacementProcess(ddb)
        packed, lens, fl = pp.pack_reads_host(seq, off)
        words = 2 * max(dna.n_branches, prot.n_branches) + 4
        m = np.full(words, POISON, np.uint64)
        fo = np.full(n, FLAG_POISON, np.uint32)
        ct = _lib.rk_counters()
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

        def call(db=ddb, K=K, step=0, n=n, seq=seq, off=off, masses=m):
            p = _lib.rk_params(K, 0.01, _lib.RK_AMB_MEAN, float("-inf"))
            return lib.rk_place_batch_masses(None if db is None else db.handle, C.byref(p), step, n, ptr(seq), ptr(off), None, ptr(masses), ptr(fo), C.byref(ct))

        def call_packed(db=ddb, K=K, n=n, packed=packed, masses=m):
            p = _lib.rk_params(K, 0.01, _lib.RK_AMB_MEAN, float("-inf"))
            return lib.rk_place_batch_packed_masses(None if db is None else db.handle, C.byref(p), n, ptr(packed), 0 if packed is None else packed.shape[1],
                                                    ptr(lens), 0, ptr(fl), None, None, None, ptr(masses), ptr(fo), C.byref(ct))

        invalid = [dict(db=None), dict(masses=None), dict(seq=None), dict(off=None), dict(K=0), dict(K=17), dict(step=4), dict(step=2 ** 31)]
        for kw in invalid:
            assert call(**kw) == _lib.RK_ERR_INVALID, kw
            assert lib.rk_last_error() != b"", kw
        for kw in (dict(db=None), dict(masses=None), dict(packed=None), dict(K=0), dict(K=17)):
            assert call_packed(**kw) == _lib.RK_ERR_INVALID, kw
            assert lib.rk_last_error() != b"", kw
        for kw in (dict(db=pdb, step=1), dict(db=pdb, step=2), dict(db=ddb, step=3)):
            assert call(**kw) == _lib.RK_ERR_UNSUPPORTED, kw
            assert lib.rk_last_error() != b"", kw
        assert call(n=0) == _lib.RK_OK and call_packed(n=0) == _lib.RK_OK
        assert (m == POISON).all() and (fo == FLAG_POISON).all()
        # and the same arguments without the fault work
        m[:] = 0
        assert call() == _lib.RK_OK
        full = pp.processQueries(seq, off, keepAtMost=K)
        B = dna.n_branches
        assert np.array_equal(m[:2 * B + 4], ref_words(B, full)) and np.array_equal(fo, full.flags)
    finally:
        ddb.close()
        pdb.close()


# ---- 6. the drivers ----
def test_drivers_masses_only_flag(tmp_path):
    """the FASTA of test_drivers_masses_flag, duplicates included, on both strands: --masses-only from rk_place and from the Python
    tool are byte-identical to each other and to the --masses table of a full run; the logs equal the full run's; no jplace"""
    from rappas_amd import build
    exe = build.build_host_tools()
    n_nodes = 75
    sdb, genome = synth.make_clade_db(k=8, n_branches=n_nodes, genome_len=12_000, mean_row=6, seed=13)
    nwk = synth.make_newick(n_nodes, seed=6)
    fs, _ = synth.make_clade_reads(genome, 300, 120, seed=10)
    lines = []
    for i in range(300):
        r = fs[i * 120:(i + 1) * 120].tobytes().decode()
        if i % 17 == 0:
            r = r[:30] + "N" + r[31:]
        lines += [f">read{i} sample=x/{i}", r[:60], r[60:]]
        for d in range(i % 4 if i % 5 == 0 else 0):  # up to three duplicates, one with a gap inserted
            lines += [f">dup{d}_{i} of read{i}", r[:7] + "-" * (d == 0) + r[7:]]
    lines += [">short", "ACG", ">random", "ACGTTGCAAGGCTTAAGCTAGCTAGGATCGATCGGATTTAGCGCGCTATATCGCGAATTCCGG"]
    (tmp_path / "db.json").write_text(hostio.dump_jsondb(sdb, nwk))
    (tmp_path / "q.fasta").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    common = ["--jsondb", str(tmp_path / "db.json"), "--fasta", str(tmp_path / "q.fasta"), "--strand", "both"]

    def run(cmd, d, args):
        d.mkdir()
        r = subprocess.run(cmd + common + ["--logs", str(d)] + args, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        logs = {f.split("_")[0]: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f.endswith(".tsv") and f.split("_")[0] in ("notplaced", "reversed")}
        return logs

    got = {}
    for name, cmd in (("cpp", [exe]), ("py", [sys.executable, "-m", "rappas_amd.tools.place"])):
        full_dir, only_dir = tmp_path / (name + "_full"), tmp_path / (name + "_only")
        full_logs = run(cmd, full_dir, ["--out", str(full_dir / "out.jplace"), "--masses", str(full_dir / "masses.table")])
        only_logs = run(cmd, only_dir, ["--masses-only", str(only_dir / "masses.table")])
        assert set(full_logs) == {"notplaced", "reversed"} and only_logs == full_logs, name
        assert (only_dir / "masses.table").read_bytes() == (full_dir / "masses.table").read_bytes(), name
        assert not [f for f in os.listdir(only_dir) if f.endswith(".jplace")] and (full_dir / "out.jplace").exists()
        got[name] = (only_dir / "masses.table").read_bytes()
    assert got["cpp"] == got["py"] and len(got["py"].split(b"\n")) == n_nodes + 3
    # the option does not go with --masses
    r = subprocess.run([exe] + common + ["--masses", str(tmp_path / "a"), "--masses-only", str(tmp_path / "b")], capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT, cwd=ROOT, env=env)
    assert r.returncode != 0
    # nor with --out: no jplace is written in this mode
    for cmd in ([exe], [sys.executable, "-m", "rappas_amd.tools.place"]):
        r = subprocess.run(cmd + common + ["--out", str(tmp_path / "c.jplace"), "--masses-only", str(tmp_path / "c")], capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT, cwd=ROOT, env=env)
        assert r.returncode != 0 and "--out" in r.stderr and not (tmp_path / "c.jplace").exists() and not (tmp_path / "c").exists()
