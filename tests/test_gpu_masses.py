"""GPU (-m gpu): the edge masses on the device -- rk_masses_accumulate_device against the numpy restatement of the definition
(tests/masses_ref.py) on hand-made result sets uploaded with torch and on the engine's own results, for equality: the sums are
integers, so neither the order of the atomic adds nor the split into calls and streams shows.  B = 999 takes the kernel's LDS
variant, B = 20 001 the one that adds straight into the buffer.  Nothing expected comes from the engine.  Child processes run under
a time limit."""
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
TREES = (999, 20001)
POISON = int(np.uint64(0xA5A5A5A5DEADBEEF).astype(np.int64))


@pytest.fixture(scope="module")
def handles():
    """tiny hand-made databases: only their number of branches matters here"""
    dbs = {B: ra.PhyloKmerDB.from_synth(synth.make_db(4, 6, B, 300, 1500, seed=B)) for B in TREES}
    yield dbs
    for db in dbs.values():
        db.close()


@functools.lru_cache(maxsize=None)
def case(B, K, n, shape="mixed"):
    """(set, weights, reference without weights, reference with weights), computed once and never changed"""
    s = MR.make_set(B, K, n, seed=3, shape=shape)
    w = MR.make_weights(n, "mixed", seed=K)
    refs = (MR.masses_ref(B, s.n_rows, s.branch, s.lwr), MR.masses_ref(B, s.n_rows, s.branch, s.lwr, w))
    for a in (s.n_rows, s.branch, s.lwr, w, *refs):
        a.setflags(write=False)
    return s, w, refs


def upload(s, n=None):
    """the set as the dict of device tensors place_packed returns (score and flags too: the call must not need them, nor touch them)"""
    import torch
    n = len(s.n_rows) if n is None else n
    K = s.branch.shape[1]
    t = lambda a: torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared sets are read-only)
    return dict(n_rows=t(s.n_rows[:n]), branch=t(s.branch[:n].view(np.int16)), lwr=t(s.lwr[:n]),
                score=torch.full((n, K), -1.5, dtype=torch.float32, device="cuda"), flags=torch.full((n,), 7, dtype=torch.int32, device="cuda"))


def dev_weights(w):
    import torch
    return None if w is None else torch.from_numpy(np.array(w).view(np.int32)).cuda()


def words(t):
    return t.cpu().numpy().view(np.uint64)


def snapshot(out):
    return {k: v.clone() for k, v in out.items()}


def unchanged(out, before):
    import torch
    # bit patterns, not values: the sets carry NaN
    return all(torch.equal(out[k].reshape(-1).view(torch.uint8), before[k].reshape(-1).view(torch.uint8)) for k in before)


# ---- 1, 2. the device call against the reference; the result set stays as it was ----
@pytest.mark.parametrize("K", [1, 7, 16])
@pytest.mark.parametrize("B", TREES)
def test_device_call_equals_the_reference(handles, B, K):
    import torch
    pp = ra.PlacementProcess(handles[B])
    for n in (0, 1, 63, 65, 100003):
        s, w, refs = case(B, K, n)
        out = upload(s)
        before = snapshot(out)
        for weights, want in ((None, refs[0]), (w, refs[1])):
            got = pp.accumulate_masses(out, weights=dev_weights(weights))
            torch.cuda.synchronize()
            assert got.dtype == torch.int64 and got.numel() == 2 * B + 4
            g = words(got)
            assert np.array_equal(g, want), (n, weights is not None, np.flatnonzero(g != want)[:8])
        assert unchanged(out, before), n
        if n >= 63:  # the planted rows are there
            assert want[2 * B + 3] > 0 and want[B + B - 1] > 0
    for kind in ("zero", "one", "max"):
        s, _, refs = case(B, K, 65)
        wk = MR.make_weights(65, kind)
        got = words(pp.accumulate_masses(upload(s), weights=dev_weights(wk)))
        assert np.array_equal(got, MR.masses_ref(B, s.n_rows, s.branch, s.lwr, wk)), kind
        assert kind != "one" or np.array_equal(got, refs[0])


@pytest.mark.parametrize("B", TREES)
def test_every_row_on_one_branch(handles, B):
    """the contention case: 100 003 x 16 rows on one bin, the sum known in closed form"""
    K, n = 16, 100003
    s, w, refs = case(B, K, n, "one_branch")
    want = np.zeros(2 * B + 4, np.uint64)
    want[7], want[B + 7] = n * K * 2 ** 29, n
    want[2 * B:] = [n, n, n * K, 0]
    assert np.array_equal(refs[0], want)
    pp = ra.PlacementProcess(handles[B])
    out = upload(s)
    before = snapshot(out)
    assert np.array_equal(words(pp.accumulate_masses(out)), want)
    assert np.array_equal(words(pp.accumulate_masses(out, weights=dev_weights(w))), refs[1])
    assert unchanged(out, before)


# ---- 2b. where the variant choice and the LDS sizing decide: the last tree whose bins fit the LDS and the first behind the cache ----
LIMIT_TREES = (4094, 4095)  # 2 * 4094 + 4 = 8192 words are exactly 64 KB of LDS


def limit_db(B):
    return ra.PhyloKmerDB.from_synth(synth.make_db(4, 6, B, 300, 1500, seed=B))


@pytest.mark.parametrize("K", [1, 7, 16])
@pytest.mark.parametrize("B", LIMIT_TREES)
def test_the_lds_limit_equals_the_reference_and_the_host_call(B, K):
    s, w, refs = case(B, K, 5000)
    assert refs[1][2 * B + 3] > 0 and refs[1][B + B - 1] > 0  # the planted rows are there
    db = limit_db(B)
    try:
        got = words(ra.PlacementProcess(db).accumulate_masses(upload(s), weights=dev_weights(w)))
    finally:
        db.close()
    assert got.shape == (2 * B + 4,)
    assert np.array_equal(got, refs[1]), np.flatnonzero(got != refs[1])[:8]
    assert np.array_equal(got, ra.accumulate_masses_host(B, s, w))


@pytest.mark.parametrize("K", [1, 7, 16])
@pytest.mark.parametrize("B", LIMIT_TREES)
def test_the_lds_limit_forced_variants_give_the_same_words(B, K, monkeypatch, dev_lib):
    """developer build: RK_MASSES_VARIANT=global and =cache on both trees, the one that takes the LDS variant by default included"""
    s, w, refs = case(B, K, 5000)
    db = limit_db(B)
    try:
        pp = ra.PlacementProcess(db)
        out, dw = upload(s), dev_weights(w)
        for variant in ("global", "cache"):
            monkeypatch.setenv("RK_MASSES_VARIANT", variant)
            got = words(pp.accumulate_masses(out, weights=dw))
            assert np.array_equal(got, refs[1]), (variant, np.flatnonzero(got != refs[1])[:8])
    finally:
        db.close()


# ---- 3. calls add up: on one stream, and over two streams ----
@pytest.mark.parametrize("B", TREES)
def test_calls_accumulate_on_one_stream_and_over_two(handles, B):
    import torch
    K, n, cut = 7, 100003, 40001
    s, w, refs = case(B, K, n)
    pp = ra.PlacementProcess(handles[B])
    first = MR.SimpleNamespace(n_rows=s.n_rows[:cut], branch=s.branch[:cut], lwr=s.lwr[:cut])
    second = MR.SimpleNamespace(n_rows=s.n_rows[cut:], branch=s.branch[cut:], lwr=s.lwr[cut:])
    o1, o2 = upload(first), upload(second)
    w1, w2 = dev_weights(w[:cut]), dev_weights(w[cut:])
    m = pp.accumulate_masses(o1, weights=w1)
    assert pp.accumulate_masses(o2, weights=w2, masses=m) is m
    assert np.array_equal(words(m), refs[1])
    # a buffer that holds something already is added to
    start = np.arange(2 * B + 4, dtype=np.uint64) * np.uint64(5)
    m = torch.from_numpy(start.view(np.int64).copy()).cuda()
    pp.accumulate_masses(o1, weights=w1, masses=m)
    assert np.array_equal(words(m), MR.masses_ref(B, first.n_rows, first.branch, first.lwr, w[:cut], masses=start))
    # two buffers filled on two streams add up to the single-call buffer
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        ma = pp.accumulate_masses(o1, weights=w1, stream=sa.cuda_stream)
    with torch.cuda.stream(sb):
        mb = pp.accumulate_masses(o2, weights=w2, stream=sb.cuda_stream)
    sa.synchronize()
    sb.synchronize()
    assert np.array_equal(words(ma) + words(mb), refs[1])
    assert np.array_equal(words(ma), MR.masses_ref(B, first.n_rows, first.branch, first.lwr, w[:cut]))


# ---- 4. end to end on the engine's own results ----
def to_host(out):
    return ra.Placements(out["n_rows"].cpu().numpy(), out["branch"].cpu().numpy().view(np.uint16), out["score"].cpu().numpy(),
                         out["lwr"].cpu().numpy(), out["flags"].cpu().numpy().view(np.uint32), {})


def check_end_to_end(db, out, n_branches, min_placed):
    import torch
    pp = ra.PlacementProcess(db)
    n = out["n_rows"].numel()
    w = MR.make_weights(n, "mixed", seed=1)
    before = snapshot(out)
    got = words(pp.accumulate_masses(out))
    got_w = words(pp.accumulate_masses(out, weights=dev_weights(w)))
    torch.cuda.synchronize()
    assert unchanged(out, before)
    host = to_host(out)
    want = MR.masses_ref(n_branches, host.n_rows, host.branch, host.lwr)
    assert np.array_equal(got, want)
    assert np.array_equal(got_w, MR.masses_ref(n_branches, host.n_rows, host.branch, host.lwr, w))
    assert np.array_equal(got, ra.accumulate_masses_host(n_branches, host)) and np.array_equal(got_w, ra.accumulate_masses_host(n_branches, host, w))
    B = n_branches
    placed = int((host.n_rows > 0).sum())
    assert want[2 * B] == n and want[2 * B + 1] == placed and min_placed <= placed < n and want[2 * B + 3] == 0
    assert want[2 * B + 2] == host.n_rows.astype(np.int64).sum() > placed and want[B:2 * B].sum() == placed
    # a sanity bound on the reference itself: the LWRs of a read sum to one over ALL its branches, so its kept rows hold at most one
    # (and half a unit of rounding each), and its best row at least the mean, 1 / B
    assert placed * 2 ** 30 // B - placed <= int(want[:B].sum()) <= placed * 2 ** 30 + 8 * placed


def test_end_to_end_on_C1_both_strands():
    import torch
    sdb = synth.make_config_db("C1")
    seq, off = synth.make_reads(4, 3000, 150, seed=5, amb_rate=0.002, bad_rate=0.01, var_len=148)
    assert (np.diff(off.astype(np.int64)) < sdb.k).any()
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        pp = ra.PlacementProcess(db)
        d_seq, d_off = torch.from_numpy(seq).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        packed, lens, flags = pp.pack_reads(d_seq, d_off, 150)
        out = pp.place_packed(packed, lens=lens, flags_in=flags, seq_ascii=d_seq, seq_off=d_off, strand="both")
        torch.cuda.synchronize()
        fl = out["flags"].cpu().numpy().view(np.uint32)
        assert (fl & ra.RK_FLAG_TOO_SHORT).any() and (fl & ra.RK_FLAG_AMBIGUOUS).any() and (fl & ra.RK_FLAG_BAD_CHAR).any() and (fl & ra.RK_FLAG_REVERSE).any()
        check_end_to_end(db, out, sdb.n_branches, 2000)
    finally:
        db.close()


def test_end_to_end_translated():
    from tests.test_gpu_translate import planted_case
    from tests import translate_ref as TR
    import torch
    sdb, reads, _ = planted_case(3)
    seq, off = TR.batch(reads)
    packed, lens, flags = ra.pack_reads(4, 1, seq, off)
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        out = ra.PlacementProcess(db).place_translated(torch.from_numpy(packed.view(np.int32)).cuda(), lens=torch.from_numpy(lens.view(np.int32)).cuda(),
                                                       flags_in=torch.from_numpy(flags.view(np.int32)).cuda())
        torch.cuda.synchronize()
        check_end_to_end(db, out, sdb.n_branches, 1000)
    finally:
        db.close()


# ---- 5. error calls ----
@pytest.mark.parametrize("B", TREES)
def test_error_calls_leave_a_poisoned_buffer_untouched(handles, B):
    import torch
    lib = _lib.load()
    K, n = 7, 65
    s, _, refs = case(B, K, n)
    out = upload(s)
    m = torch.full((2 * B + 4,), POISON, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(n_rows=out["n_rows"].data_ptr(), branch=out["branch"].data_ptr(), lwr=out["lwr"].data_ptr())

    def call(K=K, n=n, masses=m.data_ptr(), db=handles[B].handle, **kw):
        f = dict(good, **kw)
        res = _lib.rk_result(f["n_rows"], f["branch"], None, f["lwr"], None)
        return lib.rk_masses_accumulate_device(db, K, n, C.byref(res), None, masses, st)

    for kw in (dict(n_rows=None), dict(branch=None), dict(lwr=None), dict(masses=None), dict(K=0), dict(K=17), dict(n=2 ** 32), dict(db=None)):
        assert call(**kw) == _lib.RK_ERR_INVALID, kw
        assert lib.rk_last_error() != b"", kw
    assert lib.rk_masses_accumulate_device(handles[B].handle, K, n, None, None, m.data_ptr(), st) == _lib.RK_ERR_INVALID
    assert call(n=0) == _lib.RK_OK and lib.rk_masses_accumulate_device(handles[B].handle, K, 0, None, None, None, st) == _lib.RK_OK
    torch.cuda.synchronize()
    assert bool((m == POISON).all())
    m.zero_()
    assert call() == _lib.RK_OK  # score and flags NULL: not read
    assert np.array_equal(words(m), refs[0])
    with pytest.raises(ValueError):
        ra.PlacementProcess(handles[B]).accumulate_masses(out, masses=torch.zeros(2 * B + 3, dtype=torch.int64, device="cuda"))


# ---- 6. the drivers ----
def test_drivers_masses_flag(tmp_path):
    from rappas_amd import build
    exe = build.build_host_tools()
    n_nodes = 75
    sdb, genome = synth.make_clade_db(k=8, n_branches=n_nodes, genome_len=12_000, mean_row=6, seed=13)
    nwk = synth.make_newick(n_nodes, seed=6)
    fs, _ = synth.make_clade_reads(genome, 300, 120, seed=10)
    lines, n_records = [], 0
    for i in range(300):
        r = fs[i * 120:(i + 1) * 120].tobytes().decode()
        if i % 17 == 0:
            r = r[:30] + "N" + r[31:]
        lines += [f">read{i} sample=x/{i}", r[:60], r[60:]]
        n_records += 1
        for d in range(i % 4 if i % 5 == 0 else 0):  # up to three duplicates, one with a gap inserted
            lines += [f">dup{d}_{i} of read{i}", r[:7] + "-" * (d == 0) + r[7:]]
            n_records += 1
    lines += [">short", "ACG", ">random", "ACGTTGCAAGGCTTAAGCTAGCTAGGATCGATCGGATTTAGCGCGCTATATCGCGAATTCCGG"]
    n_records += 2
    (tmp_path / "db.json").write_text(hostio.dump_jsondb(sdb, nwk))
    (tmp_path / "q.fasta").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    tables = {}
    for name, cmd in (("cpp", [exe]), ("py", [sys.executable, "-m", "rappas_amd.tools.place"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run(cmd + ["--jsondb", str(tmp_path / "db.json"), "--fasta", str(tmp_path / "q.fasta"), "--out", str(d / "out.jplace"), "--strand", "both",
                                  "--masses", str(d / "masses.tsv")], capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        tables[name] = (d / "masses.tsv").read_bytes()
    assert tables["cpp"] == tables["py"]
    rows = tables["py"].decode().split("\n")
    assert rows[0].split("\t") == ["node_id", "edge_num", "label", "best_reads", "mass_q30", "mass", "clade_best_reads", "clade_mass_q30", "clade_mass"]
    assert len(rows) == n_nodes + 3 and rows[-1] == ""
    total = rows[-2].split("\t")
    assert total[0] == "#total" and int(total[1]) == n_records and n_records > 340  # reads, not unique sequences
    assert 300 <= int(total[2]) < n_records and int(total[3]) >= int(total[2]) and int(total[4]) == 0
    body = [r.split("\t") for r in rows[1:n_nodes + 1]]
    assert sum(int(r[3]) for r in body) == int(total[2])
    root = body[0]
    assert root[1] == "-1" and int(root[6]) == int(total[2]) and int(root[7]) == sum(int(r[4]) for r in body)
