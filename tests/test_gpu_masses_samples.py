"""GPU (-m gpu): the per-sample edge masses -- rk_masses_accumulate_samples_device on hand-made result sets uploaded with torch, and
the membership form of the host path's masses sink (rk_place_batch_masses_samples and its packed twin) -- for equality of all
S * W + 1 words with the numpy restatement of the definition (tests/masses_samples_ref.py).  (B, S) = (999, 4) is the last shape whose
bins fit the LDS (8 009 words), (999, 5) the first behind the per-block cache.  Nothing expected comes from the new calls.  Child
processes run under a time limit."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import hostio, synth
from tests import masses_ref as MR
from tests import masses_samples_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300
SHAPES = [(999, 4), (999, 5), (5, 300), (20001, 40), (65535, 3)]
LIMIT_SHAPES = [(1363, 3), (2046, 2), (999, 130)]  # the last LDS shape, the first cached one, more samples than MASS_TOTAL_SLOTS
N, M = 5000, 20000  # reads of a hand-made set, entries of a membership list over it
SLOTS = 512         # MASS_CACHE_SLOTS in rappas_amd/csrc/rk_masses.h
POISON = np.uint64(0xA5A5A5A5DEADBEEF)


@pytest.fixture(scope="module")
def handles():
    """tiny hand-made databases: only their number of branches matters here"""
    dbs = {B: ra.PhyloKmerDB.from_synth(synth.make_db(4, 6, B, 300, 1500, seed=B)) for B in sorted({b for b, _ in SHAPES + LIMIT_SHAPES})}
    yield dbs
    for db in dbs.values():
        db.close()


@functools.lru_cache(maxsize=None)
def result_set(B, K, shape="mixed"):
    s = MR.make_set(B, K, N, seed=3, shape=shape)
    for a in (s.n_rows, s.branch, s.lwr):
        a.setflags(write=False)
    return s


def upload(s):
    import torch
    t = lambda a: torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared sets are read-only)
    return dict(n_rows=t(s.n_rows), branch=t(s.branch.view(np.int16)), lwr=t(s.lwr))


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


def words(t):
    return t.cpu().numpy().view(np.uint64)


def device_call(pp, out, S, mem, w=None, **kw):
    return pp.accumulate_masses_samples(out, S, dev(mem.sample), member_read=dev(mem.read), member_weight=dev(w), **kw)


# ---- 1. the device call against the reference ----
@pytest.mark.parametrize("K", [1, 7, 16])
@pytest.mark.parametrize("B,S", SHAPES)
def test_device_call_equals_the_reference(handles, B, S, K):
    pp = ra.PlacementProcess(handles[B])
    s = result_set(B, K)
    out = upload(s)
    for kind in SR.KINDS:
        mem = SR.make_members(kind, N, M, S, seed=K)
        SR.assert_not_trivial(mem, N, S)
        m = len(mem.sample)
        assert m == (N if kind == "identity" else M) or kind == "csr"
        for wk in (None, "zero", "max", "mixed"):
            w = MR.make_weights(m, wk, seed=K)
            want = SR.masses_samples_ref(B, S, s, mem.sample, mem.read, w)
            got = words(device_call(pp, out, S, mem, w))
            assert got.shape == (SR.words(B, S),)
            assert np.array_equal(got, want), (kind, wk, np.flatnonzero(got != want)[:8])
            assert want[-1] == mem.n_planted > 0
            assert np.array_equal(got, ra.accumulate_masses_samples_host(B, s, S, mem.sample, member_read=mem.read, member_weight=w))


@pytest.mark.parametrize("K", [1, 7, 16])
@pytest.mark.parametrize("B,S", LIMIT_SHAPES)
def test_device_call_at_the_lds_limit_and_with_more_samples_than_total_slots(handles, B, S, K):
    """(1363, 3): 8 191 words, the LDS form; (2046, 2): 8 193 words, the cached form; (999, 130): the cached form with more samples
    than the totals' table has slots -- the interleaved list puts 130 samples on the 64 slots of the first block, so a sample that
    does not hold its slot adds its totals to global memory"""
    assert SR.words(B, S) == {(1363, 3): 8191, (2046, 2): 8193, (999, 130): 260261}[B, S]
    pp = ra.PlacementProcess(handles[B])
    s = result_set(B, K)
    out = upload(s)
    for kind in SR.KINDS:
        mem = SR.make_members(kind, N, M, S, seed=K)
        SR.assert_not_trivial(mem, N, S)
        if kind == "interleaved" and S == 130:  # the first block's 256 entries name every sample: two and more to a slot of the totals' table
            assert len(np.unique(mem.sample[:256][mem.sample[:256] < S])) == S > 64
        w = MR.make_weights(len(mem.sample), "mixed", seed=K)
        want = SR.masses_samples_ref(B, S, s, mem.sample, mem.read, w)
        got = words(device_call(pp, out, S, mem, w))
        assert got.shape == (SR.words(B, S),)
        assert np.array_equal(got, want), (kind, np.flatnonzero(got != want)[:8])
        assert want[-1] == mem.n_planted > 0
        assert np.array_equal(got, ra.accumulate_masses_samples_host(B, s, S, mem.sample, member_read=mem.read, member_weight=w))


@pytest.mark.parametrize("B,S", [(999, 4), (20001, 40)])
def test_every_row_on_one_branch_and_every_entry_in_one_sample(handles, B, S):
    """the contention path and the cache's single slot: the sum in closed form"""
    K, smp = 16, S - 2
    s = result_set(B, K, "one_branch")
    mem = SR.SimpleNamespace(read=(np.arange(M) % N).astype(np.uint32), sample=np.full(M, smp, np.uint32))
    W = 2 * B + 4
    want = np.zeros(S * W + 1, np.uint64)
    want[smp * W + 7], want[smp * W + B + 7] = M * K * 2 ** 29, M
    want[smp * W + 2 * B:(smp + 1) * W] = [M, M, M * K, 0]
    assert np.array_equal(SR.masses_samples_ref(B, S, s, mem.sample, mem.read), want)
    pp = ra.PlacementProcess(handles[B])
    assert np.array_equal(words(device_call(pp, upload(s), S, mem)), want)


def test_more_hot_keys_than_the_cache_has_slots(handles):
    """every block meets more distinct (sample, branch) keys than its table holds: the rest goes to the global atomics"""
    B, S, K = 20001, 40, 7
    s = MR.make_set(B, K, N, seed=8)
    rng = np.random.default_rng(8)
    hot = rng.choice(B, 64, replace=False).astype(np.uint16)
    inside = s.branch < B
    s.branch[inside] = hot[rng.integers(0, 64, s.branch.shape)][inside]
    mem = SR.SimpleNamespace(read=(np.arange(M) % N).astype(np.uint32), sample=rng.integers(0, S, M).astype(np.uint32))
    # a block's four waves take 256 consecutive entries (the grid has a block per 256 entries at this size): the keys of the first block
    first = slice(0, 256)
    rows = np.arange(K)[None, :] < np.minimum(s.n_rows[mem.read[first]], K)[:, None]
    keys = (mem.sample[first].astype(np.int64)[:, None] << 16 | s.branch[mem.read[first]].astype(np.int64))[rows & (s.branch[mem.read[first]] < B)]
    assert len(np.unique(keys)) > SLOTS
    w = MR.make_weights(M, "mixed", 8)
    pp = ra.PlacementProcess(handles[B])
    got = words(device_call(pp, upload(s), S, mem, w))
    assert np.array_equal(got, SR.masses_samples_ref(B, S, s, mem.sample, mem.read, w))


# ---- 2. adding: a buffer that holds something, two streams into one buffer ----
@pytest.mark.parametrize("B,S", [(999, 4), (999, 5), (65535, 3)])
def test_non_zero_start_and_two_streams_into_one_buffer(handles, B, S):
    import torch
    K = 7
    s = result_set(B, K)
    out = upload(s)
    pp = ra.PlacementProcess(handles[B])
    mem = SR.make_members("csr", N, 0, S, seed=5)
    SR.assert_not_trivial(mem, N, S)
    m = len(mem.sample)
    w = MR.make_weights(m, "mixed", 5)
    start = np.full(SR.words(B, S), POISON, np.uint64) + np.arange(SR.words(B, S), dtype=np.uint64) * np.uint64(0x0123456789ABCDEF)
    buf = torch.from_numpy(start.view(np.int64).copy()).cuda()
    assert device_call(pp, out, S, mem, w, masses=buf) is buf
    want = SR.masses_samples_ref(B, S, s, mem.sample, mem.read, w, masses=start)
    assert np.array_equal(words(buf), want)
    # the two halves of the list on two streams, both into the buffer that holds the poison
    cut = m // 2 + 3
    halves = [(SR.SimpleNamespace(read=mem.read[a:b], sample=mem.sample[a:b]), w[a:b]) for a, b in ((0, cut), (cut, m))]
    args = [(dev(h.sample), dev(h.read), dev(hw)) for h, hw in halves]
    buf = torch.from_numpy(start.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for st, (ds, dr, dw) in zip(streams, args):
        with torch.cuda.stream(st):
            pp.accumulate_masses_samples(out, S, ds, member_read=dr, member_weight=dw, masses=buf, stream=st.cuda_stream)
    for st in streams:
        st.synchronize()
    assert np.array_equal(words(buf), want)


@pytest.mark.parametrize("B", [999, 20001])
def test_one_sample_over_every_read_is_the_existing_call_and_a_zero_word(handles, B):
    import torch
    K = 7
    s = result_set(B, K)
    out = upload(s)
    pp = ra.PlacementProcess(handles[B])
    w = MR.make_weights(N, "mixed", 2)
    W = 2 * B + 4
    for weights in (None, w):
        got = words(pp.accumulate_masses_samples(out, 1, torch.zeros(N, dtype=torch.int32, device="cuda"), member_weight=dev(weights)))
        old = words(pp.accumulate_masses(out, weights=dev(weights)))
        assert got.shape == (W + 1,) and np.array_equal(got[:W], old) and got[W] == 0 and old[2 * B] > 0


# ---- 3. the host path ----
K_HOST, S_HOST = 7, 7


def host_calls(pp, step, seq, off, mem, w, packed=None, **kw):
    common = dict(member_off=mem.off, member_weight=w, keepAtMost=K_HOST, **kw)
    if step == "packed":
        return pp.processQueriesPackedMassesSamples(packed[0], S_HOST, mem.sample, lens=packed[1], flags=packed[2], seq=seq, seq_off=off, **common)
    if step == "translated":
        return pp.processQueriesMassesSamples(seq, off, S_HOST, mem.sample, translate=True, **common)
    return pp.processQueriesMassesSamples(seq, off, S_HOST, mem.sample, strand=step, **common)


HOST_STEPS = [("C1", "forward"), ("C1", "both"), ("C1", "packed"), ("T20k", "forward"), ("T20k", "both"), ("T20k", "packed"), ("protein", "translated")]


@pytest.mark.parametrize("name,step", HOST_STEPS)
def test_host_path_equals_the_reference_over_the_existing_call(name, step):
    from tests import test_gpu_masses_only as MO
    sdb = MO.database(name)
    B = sdb.n_branches
    seq, off = MO.reads(name)
    n = len(off) - 1
    mem = SR.make_members("csr", n, 0, S_HOST, seed=n)
    SR.assert_not_trivial(mem, n, S_HOST)
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        pp = ra.PlacementProcess(db)
        packed = pp.pack_reads_host(seq, off) if step == "packed" else None
        full = MO.full_call(pp, step, seq, off, packed)
        assert 0 < int((full.n_rows > 0).sum()) < n
        for wk in (None, "mixed"):
            w = MR.make_weights(len(mem.sample), wk, seed=4)
            start = np.arange(SR.words(B, S_HOST), dtype=np.uint64) * np.uint64(5)
            want = SR.masses_samples_ref(B, S_HOST, full, mem.sample, mem.read, w, masses=start)
            fo = np.full(n, 0xDEADBEEF, np.uint32)
            got, flags, counters = host_calls(pp, step, seq, off, mem, w, packed, masses=start.copy(), flags_out=fo)
            assert np.array_equal(got, want), (wk, np.flatnonzero(got != want)[:8])
            assert flags is fo and np.array_equal(flags, full.flags) and counters == full.counters
            assert want[-1] - start[-1] == mem.n_planted > 0
        # one entry per read (member_off NULL): sample r mod S
        one = SR.SimpleNamespace(off=None, sample=(np.arange(n) % S_HOST).astype(np.uint32))
        got, _, _ = host_calls(pp, step, seq, off, one, None, packed)
        assert np.array_equal(got, SR.masses_samples_ref(B, S_HOST, full, one.sample))
        # and the existing profile-only call on the same handle afterwards still gives its 2B + 4 words
        if step == "forward":
            old, _, _ = pp.processQueriesMasses(seq, off, keepAtMost=K_HOST)
            assert np.array_equal(old, MR.masses_ref(B, full.n_rows, full.branch, full.lwr))
    finally:
        db.close()


@pytest.mark.parametrize("name,step", [("C1", "both"), ("T20k", "forward"), ("C1", "packed"), ("protein", "translated")])
def test_five_chunks_with_entries_across_their_borders_give_the_single_chunk_words(name, step, monkeypatch, dev_lib):
    from tests import test_gpu_masses_only as MO
    sdb = MO.database(name)
    B = sdb.n_branches
    seq, off = MO.reads("C1")  # (5 000 reads on every database: five chunks of 1 024)
    n = len(off) - 1
    assert n == 5000
    mem = SR.make_members("csr", n, 0, S_HOST, seed=1)
    for border in (1024, 2048, 3072, 4096):  # a chunk's entries begin in the middle of the list, next to a read that owns some
        assert 0 < mem.off[border] < mem.off[-1] and mem.off[border - 1] < mem.off[border + 1]
    w = MR.make_weights(len(mem.sample), "mixed", seed=4)
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        pp = ra.PlacementProcess(db)
        packed = pp.pack_reads_host(seq, off) if step == "packed" else None
        single, flags1, ct1 = host_calls(pp, step, seq, off, mem, w, packed)
        monkeypatch.setenv("RK_CHUNK_READS", "1024")
        full = MO.full_call(pp, step, seq, off, packed)
        assert (full.n_rows > 0).any()
        got, flags, ct = host_calls(pp, step, seq, off, mem, w, packed)
        assert np.array_equal(got, single) and np.array_equal(flags, flags1) and ct == ct1
        assert np.array_equal(single, SR.masses_samples_ref(B, S_HOST, full, mem.sample, mem.read, w))
        assert np.array_equal(flags1, full.flags) and ct1 == full.counters
    finally:
        db.close()


def test_host_call_errors_leave_poisoned_buffers_untouched():
    import ctypes as C
    from rappas_amd import _lib
    from tests import test_gpu_masses_only as MO
    sdb = MO.database("C1")
    B = sdb.n_branches
    seq, off = MO.reads("C1")
    n = 100
    seq, off = np.ascontiguousarray(seq[:int(off[n])]), np.ascontiguousarray(off[:n + 1])
    mem = SR.make_members("csr", n, 0, S_HOST, seed=3, planted=False)
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        lib = _lib.load()
        m = np.full(SR.words(B, S_HOST), POISON, np.uint64)
        fo = np.full(n, 0xDEADBEEF, np.uint32)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        bad_first, decreasing = mem.off.copy(), mem.off.copy()
        bad_first[0] = 1
        decreasing[50] = decreasing[51] + 1

        def call(db=db, K=K_HOST, step=0, S=S_HOST, moff=mem.off, sample=mem.sample, masses=m, seq=seq):
            p = _lib.rk_params(K, 0.01, _lib.RK_AMB_MEAN, float("-inf"))
            return lib.rk_place_batch_masses_samples(None if db is None else db.handle, C.byref(p), step, n, ptr(seq), ptr(off), S, ptr(moff), ptr(sample), None,
                                                     ptr(masses), ptr(fo), None)

        for kw in (dict(db=None), dict(masses=None), dict(seq=None), dict(sample=None), dict(K=0), dict(K=17), dict(step=4), dict(S=0), dict(S=65536),
                   dict(moff=bad_first), dict(moff=decreasing)):
            assert call(**kw) == _lib.RK_ERR_INVALID, kw
            assert lib.rk_last_error() != b"", kw
            assert (m == POISON).all() and (fo == 0xDEADBEEF).all(), kw
        assert call(step=3) == _lib.RK_ERR_UNSUPPORTED and (m == POISON).all()
        m[:] = 0
        assert call() == _lib.RK_OK
        full = ra.PlacementProcess(db).processQueries(seq, off, keepAtMost=K_HOST)
        assert np.array_equal(m, SR.masses_samples_ref(B, S_HOST, full, mem.sample, mem.read)) and np.array_equal(fo, full.flags)
    finally:
        db.close()


# ---- 4. the drivers, end to end ----
def test_drivers_sample_sep_equals_a_run_per_sample(tmp_path):
    """2 001 records from three samples, interleaved, sequences repeated inside and across samples, one sample with a single read:
    `--masses-only --sample-sep _` gives, per sample, byte for byte the table of a `--masses-only` run on that sample's records alone;
    `--masses --sample-sep _` writes the same file; rk_place and the Python tool write identical bytes"""
    from rappas_amd import build
    exe = build.build_host_tools()
    n_nodes = 75
    sdb, genome = synth.make_clade_db(k=8, n_branches=n_nodes, genome_len=12_000, mean_row=6, seed=13)
    nwk = synth.make_newick(n_nodes, seed=6)
    fs, _ = synth.make_clade_reads(genome, 601, 120, seed=10)
    read = lambda i: fs[i * 120:(i + 1) * 120].tobytes().decode()
    records = []
    for i in range(2000):
        idx = i % 600 if i < 1800 else (i * 13) % 600
        sample = ("gut", "soil")[(i // 600 + i) % 2]  # a read's three copies: two in one sample, one in the other
        seq = read(idx)
        if i % 97 == 0:
            seq = "ACG"  # too short to be placed, in both samples
        records.append((f"{sample}_{i} rec", seq))
    records.insert(1000, ("zoo_only", read(600)))
    samples = sorted({h.split("_")[0] for h, _ in records})
    assert samples == ["gut", "soil", "zoo"] and sum(h.startswith("zoo_") for h, _ in records) == 1
    fasta = lambda recs: "".join(f">{h}\n{s[:60]}\n{s[60:]}\n" if len(s) > 60 else f">{h}\n{s}\n" for h, s in recs)
    (tmp_path / "db.json").write_text(hostio.dump_jsondb(sdb, nwk))
    (tmp_path / "q.fasta").write_text(fasta(records))
    for s in samples:
        (tmp_path / f"{s}.fasta").write_text(fasta([r for r in records if r[0].startswith(s + "_")]))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    db_args = ["--jsondb", str(tmp_path / "db.json"), "--strand", "both"]

    def run(cmd, d, query, args, ok=True):
        d.mkdir()
        r = subprocess.run(cmd + db_args + ["--fasta", str(tmp_path / query), "--logs", str(d)] + args, capture_output=True, text=True, timeout=CHILD_TIMEOUT,
                           cwd=ROOT, env=env)
        assert (r.returncode == 0) == ok, r.stderr[-3000:]
        return r

    want = b""
    for i, s in enumerate(samples):
        d = tmp_path / ("alone_" + s)
        run([exe], d, f"{s}.fasta", ["--masses-only", str(d / "t")])
        alone = (d / "t").read_bytes()
        assert len(alone.split(b"\n")) == n_nodes + 3
        want += f"#sample\t{s}\t{i}\n".encode() + alone
    want += b"#skipped_entries\t0\n"
    placed = [int(ln.split(b"\t")[2]) for ln in want.split(b"\n") if ln.startswith(b"#total")]
    assert len(placed) == 3 and min(placed[:2]) > 100 and placed[0] + placed[1] + placed[2] < len(records)  # no empty profile; some reads unplaced
    for name, cmd in (("cpp", [exe]), ("py", [sys.executable, "-m", "rappas_amd.tools.place"])):
        only, full = tmp_path / (name + "_only"), tmp_path / (name + "_full")
        run(cmd, only, "q.fasta", ["--masses-only", str(only / "t"), "--sample-sep", "_"])
        assert (only / "t").read_bytes() == want, name
        run(cmd, full, "q.fasta", ["--out", str(full / "out.jplace"), "--masses", str(full / "t"), "--sample-sep", "_"])
        assert (full / "t").read_bytes() == want, name
    # a header without the separator is the documented error; the option needs one of the two tables
    (tmp_path / "bad.fasta").write_text(fasta(records[:10] + [("nosep here", read(3))]))
    r = run([exe], tmp_path / "bad", "bad.fasta", ["--masses-only", str(tmp_path / "bad_t"), "--sample-sep", "_"], ok=False)
    assert "--sample-sep: the header 'nosep here' does not contain the separator '_'" in r.stderr and not (tmp_path / "bad_t").exists()
    r = run([exe], tmp_path / "nomasses", "q.fasta", ["--out", str(tmp_path / "x.jplace"), "--sample-sep", "_"], ok=False)
    assert "--sample-sep" in r.stderr and not (tmp_path / "x.jplace").exists()
