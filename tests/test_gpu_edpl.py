"""The EDPL on the device (rk_edpl_device) against its host twin, bit for bit: trees from one node to 65 535, every K
and batch sizes round a wave and a block, both forms of the tables, the golden file, a caterpillar under a time limit, streams and
split batches, the rows behind n_rows, a placed batch end to end, and `--edpl` of the two drivers."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, hostio, synth
from rappas_amd._lib import rk_result
from tests import edpl_ref as E
from tests import kr_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300


def to_dev(n_rows, branch, lwr):
    import torch
    return {"n_rows": torch.from_numpy(np.ascontiguousarray(n_rows)).cuda(), "branch": torch.from_numpy(np.ascontiguousarray(branch).view(np.int16)).cuda(),
            "lwr": torch.from_numpy(np.ascontiguousarray(lwr)).cuda()}


def device_edpl(et, n_rows, branch, lwr, K, stream=None):
    import torch
    got = et.edpl(to_dev(n_rows, branch, lwr), K, stream=stream)
    torch.cuda.synchronize()
    return got.cpu().numpy()


CASES = [("random", B) for B in (1, 2, 3, 999, 4500, 65535)] + [("caterpillar", 2049), ("star", 2049)]


def make_tree(kind, B):
    if kind == "random":
        return R.random_tree(B, 60 + B)
    return E.shuffled(R.caterpillar(B, B) if kind == "caterpillar" else R.star(B, B), B + 1)


@pytest.mark.parametrize("kind,B", CASES, ids=[f"{k}-{B}" for k, B in CASES])
def test_device_equals_host_twin_bit_for_bit(kind, B):
    """one handle a tree; 4 096 reads for every K, then K = 7 on both sides of a wave (64 reads) and of a block (4 096 + 1)"""
    parent, bl = make_tree(kind, B)
    et = ra.EdgeTree(parent, bl)
    try:
        assert et.edpl_lds_bytes() == (E.lca_bytes(B) if E.lca_bytes(B) <= 65536 else 0)
        for K in (1, 2, 7, 16):
            n_rows, branch, lwr = E.result_set(B, K, 4097 if K == 7 else 4096, seed=11 * B + K)
            want = ra.edpl_host(parent, bl, K, n_rows, branch, lwr)
            got = device_edpl(et, n_rows, branch, lwr, K)
            assert E.same(got, want), (kind, B, K, np.nonzero(R.bits(got) != R.bits(want))[0][:8])
            if K == 7:
                assert B < 3 or np.count_nonzero(want) > 2000  # the case is not empty
                for n in (1, 63, 64, 65):
                    assert E.same(device_edpl(et, n_rows[:n], branch[:n], lwr[:n], K), want[:n]), (kind, B, n)
    finally:
        et.close()


def smallest_global_B():
    B = 1000
    while E.lca_bytes(B) <= 65536:
        B += 1
    return B


def test_both_forms_of_the_tables_give_the_same_bits(monkeypatch, dev_lib):
    """the tables in the LDS of every block (small trees) and read from global memory (large ones): the developer build's
    RK_EDPL_LDS_BYTES moves the limit, so that 999 branches and the smallest tree the product's rule sends to global memory run in
    both forms"""
    Bg = smallest_global_B()
    assert E.lca_bytes(Bg) > 65536 >= E.lca_bytes(Bg - 1) and 1000 < Bg < 4500
    K = 7
    for B in (999, Bg):
        parent, bl = R.random_tree(B, 21 + B)
        n_rows, branch, lwr = E.result_set(B, K, 4096, seed=B)
        want = ra.edpl_host(parent, bl, K, n_rows, branch, lwr)
        forms = []
        for limit in ("0", str(1 << 20)):
            monkeypatch.setenv("RK_EDPL_LDS_BYTES", limit)
            et = ra.EdgeTree(parent, bl)
            try:
                forms.append(et.edpl_lds_bytes())
                got = device_edpl(et, n_rows, branch, lwr, K)
            finally:
                et.close()
            assert E.same(got, want), (B, limit)
        assert forms == [0, E.lca_bytes(B)]  # the two runs took different forms
        monkeypatch.delenv("RK_EDPL_LDS_BYTES")
        et = ra.EdgeTree(parent, bl)
        try:
            assert et.edpl_lds_bytes() == (E.lca_bytes(B) if B == 999 else 0)  # the rule itself
        finally:
            et.close()


def test_golden_file_on_the_device():
    g = E.golden()
    et = ra.EdgeTree(g["parent"], g["branch_len"])
    try:
        assert E.same(device_edpl(et, g["n_rows"], g["branch"], g["lwr"], g["keep_at_most"]), g["edpl"])
    finally:
        et.close()


def test_caterpillar_of_65535_nodes_under_a_time_limit():
    """4 096 reads of 16 rows spread over the whole chain, equal to the host twin, in a child process whose time limit comes from the
    random tree of the same size: a walk that is linear in the depth (65 535 dependent loads a pair) does not fit in it"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def child(kind, limit):
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, "-m", "tests.edpl_ref", kind, "65535"], capture_output=True, text=True, timeout=limit, cwd=ROOT, env=env)
        assert r.returncode == 0, (kind, r.stderr[-3000:])
        return time.perf_counter() - t0

    t_random = child("random", CHILD_TIMEOUT)
    child("caterpillar", 2 * t_random + 10)


def test_result_does_not_depend_on_stream_or_split():
    import torch
    B, K, n = 4500, 7, 4097
    parent, bl = R.random_tree(B, 31)
    n_rows, branch, lwr = E.result_set(B, K, n, seed=32)
    want = ra.edpl_host(parent, bl, K, n_rows, branch, lwr)
    et = ra.EdgeTree(parent, bl)
    try:
        side = torch.cuda.Stream()
        assert E.same(device_edpl(et, n_rows, branch, lwr, K, stream=side.cuda_stream), want)
        h = 2000  # two halves, neither a multiple of a wave
        halves = np.concatenate([device_edpl(et, n_rows[:h], branch[:h], lwr[:h], K), device_edpl(et, n_rows[h:], branch[h:], lwr[h:], K, stream=side.cuda_stream)])
        assert E.same(halves, want)
    finally:
        et.close()


def test_rows_behind_n_rows_are_never_read_and_nothing_else_is_written():
    import torch
    lib = _lib.load()
    B, K, n = 999, 7, 1000
    parent, bl = R.random_tree(B, 41)
    n_rows, branch, lwr = E.result_set(B, K, n, seed=42)
    want = ra.edpl_host(parent, bl, K, n_rows, branch, lwr)
    rng = np.random.default_rng(43)
    dead = np.arange(K)[None, :] >= n_rows[:, None]
    branch2 = np.where(dead, rng.integers(0, 65536, (n, K)), branch).astype(np.uint16)
    lwr2 = np.where(dead, np.nan, lwr)
    et = ra.EdgeTree(parent, bl)
    try:
        assert E.same(device_edpl(et, n_rows, branch2, lwr2, K), want)
        # the output is written, not added into, and only its n doubles
        d = to_dev(n_rows, branch, lwr)
        out = torch.full((n + 64,), -7.0, dtype=torch.float64, device="cuda")
        res = rk_result(d["n_rows"].data_ptr(), d["branch"].data_ptr(), None, d["lwr"].data_ptr(), None)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.rk_edpl_device(et.handle, K, n, C.byref(res), out.data_ptr() + 32 * 8, st) == _lib.RK_OK
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[:32] == -7.0).all() and (o[32 + n:] == -7.0).all() and E.same(o[32:32 + n], want)
        # refused: nothing is launched, no byte written
        out.fill_(-7.0)
        for K_bad, n_bad, r, o_ptr in ((0, n, res, out.data_ptr()), (17, n, res, out.data_ptr()), (K, 1 << 32, res, out.data_ptr()), (K, n, res, None),
                                       (K, n, rk_result(None, d["branch"].data_ptr(), None, d["lwr"].data_ptr(), None), out.data_ptr()),
                                       (K, n, rk_result(d["n_rows"].data_ptr(), None, None, d["lwr"].data_ptr(), None), out.data_ptr()),
                                       (K, n, rk_result(d["n_rows"].data_ptr(), d["branch"].data_ptr(), None, None, None), out.data_ptr())):
            assert lib.rk_edpl_device(et.handle, K_bad, n_bad, C.byref(r), o_ptr, st) == _lib.RK_ERR_INVALID
        assert lib.rk_edpl_device(et.handle, K, 0, None, None, st) == _lib.RK_OK
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -7.0).all()
    finally:
        et.close()


def test_placed_batch_end_to_end():
    """a small synthetic database placed with rk_place_packed_device: the EDPL of the device result set equals edpl_host of the
    downloaded one, and rk_edpl_batch on the downloaded set gives the same bits again"""
    import torch
    n_nodes, K, n = 75, 7, 600
    sdb, genome = synth.make_clade_db(k=8, n_branches=n_nodes, genome_len=12_000, mean_row=6, seed=13)
    seq, _ = synth.make_clade_reads(genome, n, 120, seed=10)
    off = np.arange(n + 1, dtype=np.uint64) * 120
    parent, bl = R.random_tree(n_nodes, 5)
    db = ra.PhyloKmerDB.from_synth(sdb, device=0)
    et = ra.EdgeTree(parent, bl)
    try:
        pp = ra.PlacementProcess(db)
        d_seq, d_off = torch.from_numpy(seq).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        packed, lens, flags = pp.pack_reads(d_seq, d_off, 120)
        out = pp.place_packed(packed, lens=lens, flags_in=flags, seq_ascii=d_seq, seq_off=d_off, keepAtMost=K)
        got = et.edpl(out, K)
        torch.cuda.synchronize()
        n_rows, branch, lwr = out["n_rows"].cpu().numpy(), out["branch"].cpu().numpy().view(np.uint16), out["lwr"].cpu().numpy()
        assert (n_rows > 1).sum() > 100
        want = ra.edpl_host(parent, bl, K, n_rows, branch, lwr)
        assert E.same(got.cpu().numpy(), want) and np.count_nonzero(want) > 100
        assert E.same(et.edpl_batch(db, K, n_rows, branch, lwr), want)
        assert E.same(want[:50], E.edpl_ref(parent, bl, K, n_rows[:50], branch[:50], lwr[:50]))
        other = ra.EdgeTree(*R.random_tree(n_nodes + 1, 5))
        try:
            with pytest.raises(ra.RkError):
                other.edpl_batch(db, K, n_rows, branch, lwr)  # not the database's B
        finally:
            other.close()
    finally:
        et.close()
        db.close()


def test_batch_call_over_more_than_one_chunk():
    """rk_edpl_batch uploads 2^22 reads a chunk into buffers it reuses: one chunk and 65 reads more, K = 2"""
    B, K, n = 999, 2, (1 << 22) + 65
    parent, bl = R.random_tree(B, 51)
    n_rows, branch, lwr = E.result_set(B, K, n, seed=52, plant=False)
    sdb, _ = synth.make_clade_db(k=8, n_branches=B, genome_len=12_000, mean_row=6, seed=13)
    db = ra.PhyloKmerDB.from_synth(sdb, device=0)
    et = ra.EdgeTree(parent, bl)
    try:
        got = et.edpl_batch(db, K, n_rows, branch, lwr)
    finally:
        et.close()
        db.close()
    want = ra.edpl_host(parent, bl, K, n_rows, branch, lwr)
    assert E.same(got, want) and np.count_nonzero(want[1 << 22:]) > 10 and np.count_nonzero(want) > n // 4


def test_drivers_edpl(tmp_path):
    """`--edpl` on a small database: rk_place and the Python tool write identical bytes, with --strand both as well; the values are
    edpl_host of the placements the jplace holds; without --out it is a usage error from both"""
    from rappas_amd import build
    from rappas_amd.tools import place
    exe = build.build_host_tools()
    n_nodes = 75
    sdb, genome = synth.make_clade_db(k=8, n_branches=n_nodes, genome_len=12_000, mean_row=6, seed=13)
    nwk = synth.make_newick(n_nodes, seed=6)
    fs, _ = synth.make_clade_reads(genome, 300, 120, seed=10)
    read = lambda i: fs[i * 120:(i + 1) * 120].tobytes().decode()  # noqa: E731
    records = [(f"r{i} copy {i // 300}", read(i % 300)) for i in range(400)] + [("short", "ACG")]
    (tmp_path / "db.json").write_text(hostio.dump_jsondb(sdb, nwk))
    fasta = "".join(f">{h}\n{s}\n" for h, s in records)
    (tmp_path / "q.fasta").write_text(fasta)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(cmd, d, args, ok=True):
        d.mkdir()
        r = subprocess.run(cmd + ["--jsondb", str(tmp_path / "db.json"), "--fasta", str(tmp_path / "q.fasta"), "--logs", str(d)] + args, capture_output=True,
                           text=True, timeout=CHILD_TIMEOUT, cwd=ROOT, env=env)
        assert (r.returncode == 0) == ok, r.stderr[-3000:]
        return r

    files = {}
    for name, cmd in (("cpp", [exe]), ("py", [sys.executable, "-m", "rappas_amd.tools.place"])):
        for strand in ("fwd", "both"):
            d = tmp_path / f"{name}_{strand}"
            run(cmd, d, ["--out", str(d / "o.jplace"), "--edpl", str(d / "edpl"), "--strand", strand])
            files[name, strand] = (d / "edpl").read_bytes()
        r = run(cmd, tmp_path / (name + "_bad"), ["--masses-only", str(tmp_path / (name + "_bad_t")), "--edpl", str(tmp_path / (name + "_bad_e"))], ok=False)
        assert "--edpl" in r.stderr and "--out" in r.stderr and not (tmp_path / (name + "_bad_e")).exists()
    assert files["cpp", "fwd"] == files["py", "fwd"] and files["cpp", "both"] == files["py", "both"]
    # the values: edpl_host of the placements, on the database's tree
    doc, res = place.place_file((tmp_path / "db.json").read_bytes(), fasta.encode(), edpl=True)
    assert res.edpl.encode() == files["cpp", "fwd"]
    tree = hostio.parse_newick(nwk)
    parent = np.array([nd.parent.id if nd.parent is not None else -1 for nd in tree.nodes], np.int32)
    bl = np.array([nd.bl for nd in tree.nodes], np.float32)
    want = ra.edpl_host(parent, bl, 7, res.n_rows, res.branch, res.lwr)
    recs = hostio.read_fasta(fasta.encode())
    unique, _ = hostio.dedup_reads(recs)
    assert res.edpl == hostio.edpl_table(recs, unique, res.n_rows, want)
    lines = res.edpl.splitlines()
    assert lines[0] == f"#edpl\t{len(lines) - 1}" and len(lines) - 1 > 300 and not any(l.startswith("short\t") for l in lines)
    assert lines[1].split("\t")[0] == "r0 copy 0" and float(lines[1].split("\t")[1]) == want[0]
    assert sum(float(l.split("\t")[1]) > 0 for l in lines[1:]) > 100
