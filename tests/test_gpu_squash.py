"""The squash clustering on the device (rk_squash_device) against its host twin, word for word -- the 24 bytes of
every row and the count --, the workspace and output rules, a pooled batch end to end, and `--squash` of the two drivers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, hostio, synth
from tests import kr_ref as R
from tests import squash_ref as Q

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300


def to_dev(m):
    import torch
    return torch.from_numpy(np.ascontiguousarray(m).view(np.int64)).cuda()


def device_rows(et, dm, S, stream=None):
    import torch
    merges, n = et.squash(dm, S, stream=stream)
    torch.cuda.synchronize()
    return merges.cpu().numpy().reshape(-1).view(Q.SQUASH_MERGE), int(n.cpu().numpy()[0])


def check_against_host(parent, bl, m, S):
    et = ra.EdgeTree(parent, bl)
    try:
        got, n = device_rows(et, to_dev(m), S)
    finally:
        et.close()
    want, n_want = ra.squash_host(parent, bl, m, S)
    assert n == n_want and Q.same_rows(got, want), (len(parent), S, n, n_want)
    return got, n


@pytest.mark.parametrize("B", [1, 2, 999, 2049, 4500])
def test_device_equals_host_twin_word_for_word(B):
    """B on both sides of a chunk edge and over three chunks, ids out of pre-order; S on both sides of the KR tile edge, which is also
    the edge of the row kernel's groups of 64 samples (65, 130), and past 256 (257: five groups, the last of one sample)"""
    parent, bl = R.random_tree(B, 40 + B)
    for S in (2, 3, 65, 130, 257):
        _, n = check_against_host(parent, bl, R.sample_buffer(B, S, 50 + S), S)
        assert n == S - 1


def test_empty_identical_and_huge_samples():
    for B, S, seed in ((2049, 65, 12), (300, 6, 14)):
        parent, bl = R.random_tree(B, seed - 1)
        got, n = check_against_host(parent, bl, R.special_buffer(B, S, seed), S)
        assert n == S - 2 and tuple(got[0])[:4] == (2, 3, 2, 0) and R.bits(got[0]["distance"]) == 0
        assert 1 not in set(got["a"][:n]) | set(got["b"][:n])
        assert tuple(got[S - 2])[:4] == (Q.NONE, Q.NONE, 0, 0) and R.bits(got[S - 2]["distance"]) == 0


def test_no_sample_with_mass_and_one():
    B, S = 300, 5
    parent, bl = R.random_tree(B, 8)
    m = np.zeros(S * (2 * B + 4) + 1, np.uint64)
    got, n = check_against_host(parent, bl, m, S)
    assert n == 0 and (got["a"] == Q.NONE).all()
    m[3 * (2 * B + 4) + 7] = 99
    got, n = check_against_host(parent, bl, m, S)
    assert n == 0 and (got["a"] == Q.NONE).all()


@pytest.mark.parametrize("kind", ["caterpillar", "random"])
def test_largest_tree(kind):
    B = 65535
    parent, bl = R.caterpillar(B) if kind == "caterpillar" else R.random_tree(B, 9)
    got, n = check_against_host(parent, bl, R.sample_buffer(B, 3, 77), 3)
    assert n == 2 and (got["distance"] > 0).all()


def test_workspace_and_output_rules():
    """the same call twice and on two streams gives the same bits; nothing is written beyond rk_squash_work_bytes, round the S - 1 rows
    or round the count; a short workspace or a NULL argument is RK_ERR_INVALID and leaves the outputs as they were"""
    import torch
    lib = _lib.load()
    B, S = 2049, 67
    parent, bl = R.random_tree(B, 31)
    m = R.special_buffer(B, S, 32)
    want, n_want = ra.squash_host(parent, bl, m, S)
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)
        need = et.squash_work_bytes(S)
        assert need > et.kr_work_bytes(S) + S * S * 8
        guard = 4096
        work = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device="cuda")
        rows_bytes = (S - 1) * 24
        out = torch.full((rows_bytes + 2 * guard,), 0x6B, dtype=torch.uint8, device="cuda")
        count = torch.full((3,), -7, dtype=torch.int32, device="cuda")
        d_rows, d_count = out.data_ptr() + guard, count.data_ptr() + 4

        def call(work_bytes=need, rows=d_rows, cnt=d_count, masses=dm.data_ptr(), w=work.data_ptr(), S=S, stream=None):
            st = stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream
            return lib.rk_squash_device(et.handle, S, masses, rows, cnt, w, work_bytes, C.c_void_p(st))

        assert call(work_bytes=need - 1) == _lib.RK_ERR_INVALID and b"rk_squash_work_bytes" in lib.rk_last_error()
        for kw in (dict(rows=None), dict(cnt=None), dict(masses=None), dict(w=None), dict(S=1), dict(S=4097)):
            assert call(**kw) == _lib.RK_ERR_INVALID, kw
        assert lib.rk_squash_device(None, S, dm.data_ptr(), d_rows, d_count, work.data_ptr(), need, None) == _lib.RK_ERR_INVALID
        torch.cuda.synchronize()
        assert (out == 0x6B).all() and (count == -7).all() and (work == 0x5A).all()  # nothing was launched

        def rows_now(buf=out, at=guard):
            return buf.cpu().numpy()[at:at + rows_bytes].copy().view(Q.SQUASH_MERGE)

        assert call() == _lib.RK_OK
        torch.cuda.synchronize()
        assert Q.same_rows(rows_now(), want) and count.cpu().numpy().tolist() == [-7, n_want, -7]
        whole = out.cpu().numpy()
        assert (whole[:guard] == 0x6B).all() and (whole[guard + rows_bytes:] == 0x6B).all()
        assert (work[need:] == 0x5A).all()
        assert call() == _lib.RK_OK  # the same call again, on the workspace the first one left
        torch.cuda.synchronize()
        assert Q.same_rows(rows_now(), want) and count.cpu().numpy().tolist() == [-7, n_want, -7]
        s2 = torch.cuda.Stream()
        out2 = torch.full((rows_bytes,), 0x6B, dtype=torch.uint8, device="cuda")
        work2 = torch.empty((need,), dtype=torch.uint8, device="cuda")
        count2 = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert call(rows=out2.data_ptr(), cnt=count2.data_ptr(), w=work2.data_ptr(), stream=s2) == _lib.RK_OK  # another stream
        s2.synchronize()
        assert Q.same_rows(rows_now(out2, 0), want) and int(count2.cpu()[0]) == n_want
        assert lib.rk_squash_work_bytes(et.handle, 1) == 0 and lib.rk_squash_work_bytes(et.handle, 4097) == 0
        assert lib.rk_squash_work_bytes(et.handle, 4096) > 0
    finally:
        et.close()


def test_pooled_batch_end_to_end():
    """a pooled batch through rk_place_batch_masses_samples, which leaves the sample buffer on the device in the handle:
    rk_squash_batch on it equals the host twin on the downloaded buffer"""
    n_nodes, S = 75, 5
    sdb, genome = synth.make_clade_db(k=8, n_branches=n_nodes, genome_len=12_000, mean_row=6, seed=13)
    seq, _ = synth.make_clade_reads(genome, 600, 120, seed=10)
    n = 600
    off = np.arange(n + 1, dtype=np.uint64) * 120
    rng = np.random.default_rng(3)
    sample = rng.integers(0, S - 1, n).astype(np.uint32)  # sample S - 1 stays empty
    parent, bl = R.random_tree(n_nodes, 5)
    db = ra.PhyloKmerDB.from_synth(sdb, device=0)
    et = ra.EdgeTree(parent, bl)
    try:
        words, flags, _ = ra.PlacementProcess(db).processQueriesMassesSamples(seq, off, S, sample)
        assert (flags & 1).sum() > 100
        got, n_got = et.squash_batch(db, S)            # the buffer where the call left it
        got2, n_got2 = et.squash_batch(db, S, words)   # the host copy, uploaded
        want, n_want = ra.squash_host(parent, bl, words, S)
        ref, n_ref = Q.squash_ref(parent, bl, words, S)
        assert n_got == n_got2 == n_want == n_ref == S - 2
        assert Q.same_rows(got, want) and Q.same_rows(got2, want) and Q.same_rows(want, ref)
        assert S - 1 not in set(got["a"][:n_got]) | set(got["b"][:n_got])
        with pytest.raises(ra.RkError):
            et.squash_batch(db, S + 1)                 # not the buffer of S + 1 samples
    finally:
        et.close()
        db.close()


def test_drivers_squash(tmp_path):
    """`--squash` on a small database with `--sample-sep _`: rk_place and the Python tool write identical bytes (and rk_place the same with
    --masses), the rows are the host twin's on the per-sample tables' masses, and without --sample-sep it is a usage error from both"""
    from rappas_amd import build
    exe = build.build_host_tools()
    n_nodes = 75
    sdb, genome = synth.make_clade_db(k=8, n_branches=n_nodes, genome_len=12_000, mean_row=6, seed=13)
    nwk = synth.make_newick(n_nodes, seed=6)
    fs, _ = synth.make_clade_reads(genome, 300, 120, seed=10)
    read = lambda i: fs[i * 120:(i + 1) * 120].tobytes().decode()
    records = [(f"{('gut', 'soil', 'sea', 'a,b')[(i * 7 + i // 100) % 4]}_{i}", read(i % 300)) for i in range(700)]
    records.append(("void_1", "ACG"))  # a sample whose only read is too short to be placed: no mass
    (tmp_path / "db.json").write_text(hostio.dump_jsondb(sdb, nwk))
    (tmp_path / "q.fasta").write_text("".join(f">{h}\n{s}\n" for h, s in records))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(cmd, d, args, ok=True):
        d.mkdir()
        r = subprocess.run(cmd + ["--jsondb", str(tmp_path / "db.json"), "--fasta", str(tmp_path / "q.fasta"), "--logs", str(d)] + args, capture_output=True,
                           text=True, timeout=CHILD_TIMEOUT, cwd=ROOT, env=env)
        assert (r.returncode == 0) == ok, r.stderr[-3000:]
        return r

    files = []
    for name, cmd in (("cpp", [exe]), ("py", [sys.executable, "-m", "rappas_amd.tools.place"])):
        only, full = tmp_path / (name + "_only"), tmp_path / (name + "_full")
        run(cmd, only, ["--masses-only", str(only / "t"), "--sample-sep", "_", "--squash", str(only / "sq"), "--kr", str(only / "kr")])
        files.append((only / "sq").read_bytes())
        assert (only / "kr").exists()
        if name == "cpp":  # the buffer summed on the host and uploaded: the same file (one driver is enough: the twins share the call)
            run(cmd, full, ["--out", str(full / "o.jplace"), "--masses", str(full / "t"), "--sample-sep", "_", "--squash", str(full / "sq")])
            files.append((full / "sq").read_bytes())
        r = run(cmd, tmp_path / (name + "_bad"), ["--masses-only", str(tmp_path / (name + "_bad_t")), "--squash", str(tmp_path / (name + "_bad_sq"))], ok=False)
        assert "--squash" in r.stderr and "--sample-sep" in r.stderr and not (tmp_path / (name + "_bad_sq")).exists()
    assert len(files) == 3 and files[0] == files[1] == files[2]
    # the rows: the host twin over the masses the per-sample tables print, on the database's tree
    tree = hostio.parse_newick(nwk)
    B = len(tree.nodes)
    parent = np.array([nd.parent.id if nd.parent is not None else -1 for nd in tree.nodes], np.int32)
    bl = np.array([nd.bl for nd in tree.nodes], np.float32)
    names, mass = [], []
    for line in (tmp_path / "cpp_only" / "t").read_text().splitlines():
        f = line.split("\t")
        if f[0] == "#sample":
            names.append(f[1])
            mass.append(np.zeros(2 * B + 4, np.uint64))
        elif f[0].isdigit():
            mass[-1][int(f[0])] = int(f[4])
    assert names == ["a,b", "gut", "sea", "soil", "void"]
    words = np.concatenate(mass + [np.zeros(1, np.uint64)])
    merges, n = ra.squash_host(parent, bl, words, 5)
    assert n == 3
    assert files[0].decode() == hostio.squash_table(names, merges, n, [True, True, True, True, False])
    lines = files[0].decode().splitlines()
    assert lines[0] == "#squash\t5\t3" and lines[-1] == "#samples_without_mass\t1" and "'a,b'" in lines[4] and "void" not in lines[4]
