"""The edge PCA on the device (rk_epca_device) against its host twin, bit for bit -- every raw double and both info
words --, against the numpy restatement on the smallest shapes, the workspace and output rules, a pooled batch end to end, and
`--epca` of the two drivers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, hostio, synth
from tests import epca_ref as E
from tests import kr_ref as R
from tests import squash_ref as Q

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300


def to_dev(m):
    import torch
    return torch.from_numpy(np.ascontiguousarray(m).view(np.int64)).cuda()


def device_raw(et, dm, S, k, iters, stream=None):
    import torch
    raw, info = et.epca(dm, S, k, iters, stream=stream)
    torch.cuda.synchronize()
    return raw.cpu().numpy(), info.cpu().numpy().view(np.uint32)


def check_against_host(parent, bl, m, S, k, iters, et=None, dm=None):
    own = et is None
    et = ra.EdgeTree(parent, bl) if own else et
    try:
        got, info = device_raw(et, to_dev(m) if dm is None else dm, S, k, iters)
    finally:
        if own:
            et.close()
    want, want_info = ra.epca_host(parent, bl, m, S, k, iters)
    assert info.tolist() == want_info.tolist(), (len(parent), S, k, iters, info, want_info)
    assert E.same(got, want), (len(parent), S, k, iters, np.nonzero(R.bits(got) != R.bits(want))[0][:8])
    return got, info


@pytest.mark.parametrize("B", [1, 2, 999, 2049, 4500])
def test_device_equals_host_twin_bit_for_bit(B):
    """B: one chunk, the chunk edge, three chunks, ids out of pre-order; S on both sides of the 64-lane edge, which is also the tile's
    (65, 130), and past 256; iters = 1 makes the output a direct function of G, so a wrong Gram entry shows"""
    parent, bl = R.random_tree(B, 40 + B)
    et = ra.EdgeTree(parent, bl)
    try:
        for S in (2, 3, 65, 130, 257):
            m = R.sample_buffer(B, S, 50 + S)
            dm = to_dev(m)
            for k in (1, 5, 8):
                for iters in (1, 3, 40):
                    _, info = check_against_host(parent, bl, m, S, k, iters, et, dm)
                    assert info.tolist() == [S, min(k, S - 1)]
    finally:
        et.close()


@pytest.mark.parametrize("B,S", [(1, 2), (2, 3)])
def test_device_equals_the_numpy_restatement(B, S):
    parent, bl = R.random_tree(B, 40 + B)
    m = R.sample_buffer(B, S, 50 + S)
    for k, iters in ((1, 1), (5, 3), (8, 40)):
        got, info = check_against_host(parent, bl, m, S, k, iters)
        want, want_info = E.epca_ref(parent, bl, m, S, k, iters)
        assert E.same(got, want) and info.tolist() == want_info.tolist()


def test_empty_identical_and_huge_samples():
    """sample 1 is empty: its q entries are zeros (of the sign of the column's divisor, as the definition has it) and it is not
    counted; samples 2 and 3 are identical: G is symmetric, so their projections are the same bits"""
    for B, S, seed in ((2049, 65, 12), (300, 6, 14)):
        parent, bl = R.random_tree(B, seed - 1)
        k = 3
        got, info = check_against_host(parent, bl, R.special_buffer(B, S, seed), S, k, 30)
        assert info.tolist() == [S - 1, k]
        q = E.split(got, B, S, k)[4]
        assert (q[:, 1] == 0.0).all()
        f = ra.epca_finish(B, S, k, got, info)
        assert (f.projection[1] == 0.0).all() and E.same(f.projection[2], f.projection[3]) and (f.eigenvalue > 0).all()


def test_no_sample_with_mass_and_one():
    B, S, k = 300, 5, 4
    parent, bl = R.random_tree(B, 8)
    m = np.zeros(S * (2 * B + 4) + 1, np.uint64)
    got, info = check_against_host(parent, bl, m, S, k, 3)
    assert info.tolist() == [0, 0] and (R.bits(got) == 0).all()
    m[3 * (2 * B + 4) + 7] = 99
    got, info = check_against_host(parent, bl, m, S, k, 3)
    assert info.tolist() == [1, 0] and (R.bits(got) == 0).all()


@pytest.mark.parametrize("kind", ["caterpillar", "random"])
def test_largest_tree(kind):
    B = 65535
    parent, bl = R.caterpillar(B) if kind == "caterpillar" else R.random_tree(B, 9)
    got, info = check_against_host(parent, bl, R.sample_buffer(B, 3, 77), 3, 2, 2)
    assert info.tolist() == [3, 2] and got[0] > 0


def test_both_forms_of_the_chunk_sum_give_the_same_bits(monkeypatch, dev_lib):
    """per-chunk partials of G in the workspace (small matrices), and added in the block that holds every chunk (large ones): the
    developer build's RK_KR_PART_BYTES moves the limit between them down to a small shape"""
    parent, bl = R.random_tree(4500, 21)
    S, k = 70, 3
    m = R.special_buffer(4500, S, 22)
    want, want_info = ra.epca_host(parent, bl, m, S, k, 1)
    sizes = []
    for limit in ("0", str(1 << 28)):
        monkeypatch.setenv("RK_KR_PART_BYTES", limit)
        et = ra.EdgeTree(parent, bl)
        try:
            sizes.append(et.epca_work_bytes(S, k))
            got, info = device_raw(et, to_dev(m), S, k, 1)
        finally:
            et.close()
        assert E.same(got, want) and info.tolist() == want_info.tolist(), limit
    assert sizes[1] == sizes[0] + 3 * S * S * 8  # three chunks of partials


def test_workspace_and_output_rules():
    """the same call twice and on two streams gives the same bits; nothing is written beyond rk_epca_work_bytes, round the raw output or
    round the info words; a short workspace or a bad argument is RK_ERR_INVALID and leaves outputs and workspace as they were"""
    import torch
    lib = _lib.load()
    B, S, k, iters = 2049, 67, 5, 4
    parent, bl = R.random_tree(B, 31)
    m = R.special_buffer(B, S, 32)
    want, want_info = ra.epca_host(parent, bl, m, S, k, iters)
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)
        need = et.epca_work_bytes(S, k)
        assert need > 3 * S * B * 8 + S * S * 8
        n_out = lib.rk_epca_out_doubles(B, S, k)
        assert n_out == 1 + k * (3 + S + B) == len(want)
        guard = 4096
        work = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device="cuda")
        raw_bytes = n_out * 8
        out = torch.full((raw_bytes + 2 * guard,), 0x6B, dtype=torch.uint8, device="cuda")
        inf = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        d_raw, d_info = out.data_ptr() + guard, inf.data_ptr() + 4

        def call(work_bytes=need, raw=d_raw, info=d_info, masses=dm.data_ptr(), w=work.data_ptr(), S=S, k=k, iters=iters, stream=None):
            st = stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream
            return lib.rk_epca_device(et.handle, S, masses, k, iters, raw, info, w, work_bytes, C.c_void_p(st))

        assert call(work_bytes=need - 1) == _lib.RK_ERR_INVALID and b"rk_epca_work_bytes" in lib.rk_last_error()
        for kw in (dict(raw=None), dict(info=None), dict(masses=None), dict(w=None), dict(S=1), dict(S=4097), dict(k=0), dict(k=9), dict(iters=0),
                   dict(iters=10001)):
            assert call(**kw) == _lib.RK_ERR_INVALID, kw
        assert lib.rk_epca_device(None, S, dm.data_ptr(), k, iters, d_raw, d_info, work.data_ptr(), need, None) == _lib.RK_ERR_INVALID
        torch.cuda.synchronize()
        assert (out == 0x6B).all() and (inf == -7).all() and (work == 0x5A).all()  # nothing was launched

        def raw_now(buf=out, at=guard):
            return buf.cpu().numpy()[at:at + raw_bytes].copy().view(np.float64)

        assert call() == _lib.RK_OK
        torch.cuda.synchronize()
        assert E.same(raw_now(), want) and inf.cpu().numpy().tolist() == [-7, int(want_info[0]), int(want_info[1]), -7]
        whole = out.cpu().numpy()
        assert (whole[:guard] == 0x6B).all() and (whole[guard + raw_bytes:] == 0x6B).all()
        assert (work[need:] == 0x5A).all()
        assert call() == _lib.RK_OK  # the same call again, on the workspace the first one left
        torch.cuda.synchronize()
        assert E.same(raw_now(), want) and inf.cpu().numpy().tolist() == [-7, int(want_info[0]), int(want_info[1]), -7]
        s2 = torch.cuda.Stream()
        out2 = torch.full((raw_bytes,), 0x6B, dtype=torch.uint8, device="cuda")
        work2 = torch.empty((need,), dtype=torch.uint8, device="cuda")
        inf2 = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert call(raw=out2.data_ptr(), info=inf2.data_ptr(), w=work2.data_ptr(), stream=s2) == _lib.RK_OK  # another stream
        s2.synchronize()
        assert E.same(raw_now(out2, 0), want) and inf2.cpu().numpy().tolist() == [int(want_info[0]), int(want_info[1])]
        for S_bad, k_bad in ((1, k), (4097, k), (S, 9), (S, 0)):
            assert lib.rk_epca_work_bytes(et.handle, S_bad, k_bad) == 0
        assert lib.rk_epca_work_bytes(et.handle, 4096, 8) > 0
    finally:
        et.close()


def test_kr_and_squash_after_epca_on_a_shared_tree():
    """one EdgeTree, one grow-only workspace: epca on a small shape, then on a larger one (the workspace grows), then kr and squash of
    the same buffer still equal their host twins"""
    import torch
    B = 999
    parent, bl = R.random_tree(B, 61)
    et = ra.EdgeTree(parent, bl)
    try:
        m0 = R.sample_buffer(B, 3, 62)
        check_against_host(parent, bl, m0, 3, 2, 2, et, to_dev(m0))
        S = 70
        m = R.special_buffer(B, S, 63)
        dm = to_dev(m)
        check_against_host(parent, bl, m, S, 5, 3, et, dm)
        D = et.kr_distances(dm, S)
        merges, n = et.squash(dm, S)
        torch.cuda.synchronize()
        assert (R.bits(D.cpu().numpy()) == R.bits(ra.kr_distances_host(parent, bl, m, S))).all()
        want, n_want = ra.squash_host(parent, bl, m, S)
        assert int(n.cpu()[0]) == n_want and Q.same_rows(merges.cpu().numpy().reshape(-1).view(Q.SQUASH_MERGE), want)
        check_against_host(parent, bl, m, S, 5, 3, et, dm)  # and the edge PCA again behind them
    finally:
        et.close()


def test_pooled_batch_end_to_end():
    """a pooled batch through rk_place_batch_masses_samples, which leaves the sample buffer on the device in the handle: rk_epca_batch
    on it equals the host twin on the downloaded buffer"""
    n_nodes, S, k, iters = 75, 5, 3, 50
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
        got, info = et.epca_batch(db, S, k, iters)            # the buffer where the call left it
        got2, info2 = et.epca_batch(db, S, k, iters, words)   # the host copy, uploaded
        want, want_info = ra.epca_host(parent, bl, words, S, k, iters)
        ref, ref_info = E.epca_ref(parent, bl, words, S, k, iters)
        assert info.tolist() == info2.tolist() == want_info.tolist() == ref_info.tolist() == [S - 1, k]
        assert E.same(got, want) and E.same(got2, want) and E.same(want, ref)
        assert (E.split(got, n_nodes, S, k)[4][:, S - 1] == 0.0).all()
        with pytest.raises(ra.RkError):
            et.epca_batch(db, S + 1, k, iters)                # not the buffer of S + 1 samples
    finally:
        et.close()
        db.close()


def test_drivers_epca(tmp_path):
    """`--epca` on a small database with `--sample-sep _`, together with --kr and --squash: rk_place and the Python tool write identical
    bytes (and rk_place the same with --masses), the table is the host twin's on the per-sample tables' masses, and without
    --sample-sep it is a usage error from both"""
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
    opts = ["--epca-components", "3", "--epca-iters", "60"]
    for name, cmd in (("cpp", [exe]), ("py", [sys.executable, "-m", "rappas_amd.tools.place"])):
        only, full = tmp_path / (name + "_only"), tmp_path / (name + "_full")
        run(cmd, only, ["--masses-only", str(only / "t"), "--sample-sep", "_", "--epca", str(only / "ep"), "--squash", str(only / "sq"), "--kr", str(only / "kr")] + opts)
        files.append((only / "ep").read_bytes())
        assert (only / "kr").exists() and (only / "sq").exists()
        if name == "cpp":  # the buffer summed on the host and uploaded: the same file (one driver is enough: the twins share the call)
            run(cmd, full, ["--out", str(full / "o.jplace"), "--masses", str(full / "t"), "--sample-sep", "_", "--epca", str(full / "ep")] + opts)
            files.append((full / "ep").read_bytes())
        r = run(cmd, tmp_path / (name + "_bad"), ["--masses-only", str(tmp_path / (name + "_bad_t")), "--epca", str(tmp_path / (name + "_bad_ep"))], ok=False)
        assert "--epca" in r.stderr and "--sample-sep" in r.stderr and not (tmp_path / (name + "_bad_ep")).exists()
    assert len(files) == 3 and files[0] == files[1] == files[2]
    # the table: the host twin over the masses the per-sample tables print, on the database's tree
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
    raw, info = ra.epca_host(parent, bl, words, 5, 3, 60)
    assert info.tolist() == [4, 3]
    f = ra.epca_finish(B, 5, 3, raw, info)
    assert files[0].decode() == hostio.epca_table(names, B, 3, 60, 4, 3, f.eigenvalue, f.share, f.residual, f.projection, f.loading)
    lines = files[0].decode().splitlines()
    assert lines[0] == f"#epca\t5\t{B}\t3\t4\t3\t60" and lines[-1] == "#samples_without_mass\t1" and "nan" not in files[0].decode()
    assert lines[4] == "#projections" and lines[5].startswith("a,b\t") and lines[10] == "#loadings" and len(lines) == 12 + B
