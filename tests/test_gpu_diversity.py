"""The per-sample diversity measures on the device (rk_diversity_device) against the host twin, word for word, on
shapes on both sides of the 256 lanes, of a chunk edge, of a wave and a block of samples; the empty, identical and huge samples; the
largest tree; the known answers; two streams on one tree handle; the workspace and output rules; a pooled batch end to end; the
neighbours that run on the same buffers; and the two drivers."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, hostio, synth
from tests import kmeans_ref as K
from tests import kr_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300
THETAS = (0.0, 0.25, 0.5, 1.0, 2.0, 8.0, 3.3, 7.9)


def to_dev(m):
    import torch
    return torch.from_numpy(np.ascontiguousarray(m).view(np.int64)).cuda()


def check_against_host(parent, bl, m, S, theta):
    import torch
    et = ra.EdgeTree(parent, bl)
    try:
        r = et.diversity(to_dev(m), S, theta)
        torch.cuda.synchronize()
        got = r.values.cpu().numpy()
    finally:
        et.close()
    want = ra.diversity_host(parent, bl, m, S, theta)
    assert r.columns == want.columns and got.shape == want.values.shape == (S, 5 + 2 * len(theta))
    assert (R.bits(got) == R.bits(want.values)).all(), (len(parent), S, len(theta))
    return got


@pytest.mark.parametrize("B,S,n_theta", [(1, 1, 0), (2, 3, 1), (255, 2, 2), (257, 65, 8), (2049, 130, 3), (4500, 257, 1), (300, 4100, 2)])
def test_device_equals_host_twin_word_for_word(B, S, n_theta):
    """B on both sides of the 256 lanes and of a chunk edge, and over three chunks, ids out of pre-order; S on both sides of a wave and
    of a block, and past 4 096; every count of thetas the shapes of the kernel differ by"""
    parent, bl = R.random_tree(B, 40 + B)
    got = check_against_host(parent, bl, R.sample_buffer(B, S, 50 + S), S, THETAS[:n_theta])
    assert not np.isnan(got).any()


def test_empty_identical_and_huge_samples():
    for B, S, seed in ((2049, 65, 12), (300, 6, 14)):
        parent, bl = R.random_tree(B, seed - 1)
        got = check_against_host(parent, bl, R.special_buffer(B, S, seed), S, (0.0, 0.5, 2.0))
        assert (R.bits(got[1]) == 0x7FF8000000000000).all() and not np.isnan(np.delete(got, 1, 0)).any()
        assert (R.bits(got[2]) == R.bits(got[3])).all()


@pytest.mark.parametrize("T", [(1 << 53) + 1, (1 << 54) + 2, 1 << 62])
def test_huge_totals_follow_the_integer_indicators(T):
    from tests.test_diversity_host import huge_total_case
    parent, bl, m, S = huge_total_case(T)
    check_against_host(parent, bl, m, S, (0.0, 1.0, 0.25))


@pytest.mark.parametrize("kind", ["caterpillar", "random"])
def test_largest_tree(kind):
    B = 65535
    parent, bl = R.caterpillar(B) if kind == "caterpillar" else R.random_tree(B, 9)
    check_against_host(parent, bl, R.sample_buffer(B, 3, 77), 3, (0.5, 2.0))


def test_known_answers_on_the_device():
    from tests.test_diversity_host import golden_case
    g, parent, bl, m, S, want_bits = golden_case()
    got = check_against_host(parent, bl, m, S, g["theta"])
    assert (R.bits(got) == want_bits).all()


def test_workspace_streams_and_output_rules():
    """two calls on two streams share one tree handle, each with a workspace of its own; nothing is written beyond
    rk_diversity_work_bytes or round the output; a short or NULL workspace, a NULL argument, S, n_theta or a theta out of range are
    RK_ERR_INVALID, launch nothing and leave d_out as it was"""
    import torch
    lib = _lib.load()
    B, S = 2049, 67
    theta = np.array([0.25, 1.0], np.float64)
    parent, bl = R.random_tree(B, 31)
    m, m2 = R.special_buffer(B, S, 32), R.sample_buffer(B, S, 33)
    want, want2 = ra.diversity_host(parent, bl, m, S, theta).values, ra.diversity_host(parent, bl, m2, S, theta).values
    et = ra.EdgeTree(parent, bl)
    try:
        dm, dm2 = to_dev(m), to_dev(m2)
        need = et.diversity_work_bytes(S, 2)
        guard, out_bytes = 4096, S * 9 * 8
        work = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device="cuda")
        out = torch.full((out_bytes + 2 * guard,), 0x6B, dtype=torch.uint8, device="cuda")

        def call(work_bytes=need, masses=dm.data_ptr(), w=work.data_ptr(), S=S, n_theta=2, th=theta.ctypes.data, o=out.data_ptr() + guard, stream=None, tree=et.handle):
            st = stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream
            return lib.rk_diversity_device(tree, S, masses, n_theta, th, o, w, work_bytes, C.c_void_p(st))

        assert call(work_bytes=need - 1) == _lib.RK_ERR_INVALID and b"rk_diversity_work_bytes" in lib.rk_last_error()
        bad = np.array([0.25, np.nan]), np.array([-0.5, 1.0]), np.array([0.25, 8.5])
        for kw in (dict(w=None), dict(masses=None), dict(o=None), dict(S=0), dict(S=65536), dict(n_theta=9), dict(th=None), dict(tree=None),
                   dict(th=bad[0].ctypes.data), dict(th=bad[1].ctypes.data), dict(th=bad[2].ctypes.data)):
            assert call(**kw) == _lib.RK_ERR_INVALID, kw
        torch.cuda.synchronize()
        assert (out == 0x6B).all() and (work == 0x5A).all()  # nothing was launched
        for again in range(2):  # the second call runs on the workspace the first one left
            assert call() == _lib.RK_OK
            torch.cuda.synchronize()
            whole = out.cpu().numpy()
            assert (whole[guard:guard + out_bytes].view(np.uint64).reshape(S, 9) == R.bits(want)).all(), again
            assert (whole[:guard] == 0x6B).all() and (whole[guard + out_bytes:] == 0x6B).all() and (work[need:] == 0x5A).all()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        o1, o2 = (torch.empty((S, 9), dtype=torch.float64, device="cuda") for _ in range(2))
        w2 = torch.empty((need,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert call(o=o1.data_ptr(), stream=s1) == _lib.RK_OK and call(o=o2.data_ptr(), masses=dm2.data_ptr(), w=w2.data_ptr(), stream=s2) == _lib.RK_OK
        s1.synchronize()
        s2.synchronize()
        assert (R.bits(o1.cpu().numpy()) == R.bits(want)).all() and (R.bits(o2.cpu().numpy()) == R.bits(want2)).all()
        assert lib.rk_diversity_work_bytes(et.handle, 0, 0) == 0 and lib.rk_diversity_work_bytes(et.handle, 65536, 0) == 0 and lib.rk_diversity_work_bytes(et.handle, S, 9) == 0
        assert lib.rk_diversity_work_bytes(et.handle, 65535, 8) > 0
    finally:
        et.close()


def test_pooled_batch_end_to_end():
    """a pooled batch through rk_place_batch_masses_samples, which leaves the sample buffer on the device in the handle:
    rk_diversity_batch on it equals the host twin on the downloaded buffer"""
    n_nodes, S = 75, 5
    theta = (0.0, 0.5)
    sdb, genome = synth.make_clade_db(k=8, n_branches=n_nodes, genome_len=12_000, mean_row=6, seed=13)
    seq, _ = synth.make_clade_reads(genome, 600, 120, seed=10)
    n = 600
    off = np.arange(n + 1, dtype=np.uint64) * 120
    sample = np.random.default_rng(3).integers(0, S - 1, n).astype(np.uint32)  # sample S - 1 stays empty
    parent, bl = R.random_tree(n_nodes, 5)
    db = ra.PhyloKmerDB.from_synth(sdb, device=0)
    et = ra.EdgeTree(parent, bl)
    try:
        words, flags, _ = ra.PlacementProcess(db).processQueriesMassesSamples(seq, off, S, sample)
        assert (flags & 1).sum() > 100
        got = et.diversity_batch(db, S, theta)                  # the buffer where the call left it
        got2 = et.diversity_batch(db, S, theta, masses=words)   # the host copy, uploaded
        want = ra.diversity_host(parent, bl, words, S, theta)
        assert (R.bits(got.values) == R.bits(want.values)).all() and (R.bits(got2.values) == R.bits(want.values)).all() and got.columns == want.columns
        assert np.isnan(want.values[S - 1]).all() and not np.isnan(want.values[:S - 1]).any() and (want.values[:S - 1, 1] > 0).all()
        with pytest.raises(ra.RkError):
            et.diversity_batch(db, S + 1, theta)                # not the buffer of S + 1 samples
    finally:
        et.close()
        db.close()


def test_the_neighbours_keep_their_bits():
    """KR and k-means on the same buffers and the same tree, run before and after a diversity call, give the bits they gave before"""
    import torch
    B, S = 2049, 67
    parent, bl = R.random_tree(B, 31)
    m = R.special_buffer(B, S, 32)
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)

        def neighbours():
            D, km = et.kr_distances(dm, S), et.kmeans(dm, S, 4, 5)
            torch.cuda.synchronize()
            return D.cpu().numpy(), ra.KMeans(*(None if t is None else t.cpu().numpy() for t in km))

        D0, km0 = neighbours()
        r = et.diversity(dm, S, (1.0, 2.0))
        D1, km1 = neighbours()
        assert (R.bits(r.values.cpu().numpy()) == R.bits(ra.diversity_host(parent, bl, m, S, (1.0, 2.0)).values)).all()
        assert (R.bits(D0) == R.bits(D1)).all() and (R.bits(D0) == R.bits(ra.kr_distances_host(parent, bl, m, S))).all()
        view = lambda r: ra.KMeans(r.assign.view(np.uint32), r.dist, r.sizes.view(np.uint32), r.within, r.info.view(np.uint32), None)
        assert K.same(view(km0), view(km1), centroids=False) and K.same(view(km1), ra.kmeans_host(parent, bl, m, S, 4, 5), centroids=False)
    finally:
        et.close()


def test_drivers_diversity(tmp_path):
    """`--diversity` on a small database with `--sample-sep _`: rk_place (from a database image) and the Python tool write identical
    bytes, the table is diversity_table of the host twin on the per-sample tables' masses, and without --sample-sep it is a usage
    error from both, with the same message"""
    from rappas_amd import build
    from rappas_amd.tools import place
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
        r = subprocess.run(cmd + ["--fasta", str(tmp_path / "q.fasta"), "--logs", str(d)] + args, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT, env=env)
        assert (r.returncode == 0) == ok, r.stderr[-3000:]
        return r

    py, cpp = [sys.executable, "-m", "rappas_amd.tools.place"], [exe]
    jsondb = ["--jsondb", str(tmp_path / "db.json")]
    d = tmp_path / "py"
    run(py, d, jsondb + ["--save-dbimage", str(tmp_path / "db.rkdb"), "--masses-only", str(d / "t"), "--sample-sep", "_", "--diversity", str(d / "div.tsv"),
                         "--diversity-theta", "0.25,1", "--kr", str(d / "kr"), "--kmeans", str(d / "km"), "--kmeans-k", "2"])
    assert (d / "kr").exists() and (d / "km").exists()
    d = tmp_path / "cpp"
    run(cpp, d, ["--dbimage", str(tmp_path / "db.rkdb"), "--masses-only", str(d / "t"), "--sample-sep", "_", "--diversity", str(d / "div.tsv"), "--diversity-theta", "0.25,1"])
    files = [(tmp_path / n / "div.tsv").read_bytes() for n in ("py", "cpp")]
    assert files[0] == files[1]
    errors = []
    for name, cmd in (("py", py), ("cpp", cpp)):
        bad = tmp_path / (name + "_bad")
        r = run(cmd, bad, jsondb + ["--masses-only", str(tmp_path / (name + "_bad_t")), "--diversity", str(tmp_path / (name + "_bad_div"))], ok=False)
        assert place.DIVERSITY_NEEDS_SAMPLE_SEP in r.stderr and not (tmp_path / (name + "_bad_div")).exists()
        errors.append(r.stderr)
    # the table: the host twin over the masses the per-sample tables print, on the database's tree
    tree = hostio.parse_newick(nwk)
    B = len(tree.nodes)
    parent = np.array([nd.parent.id if nd.parent is not None else -1 for nd in tree.nodes], np.int32)
    bl = np.array([nd.bl for nd in tree.nodes], np.float32)
    names, mass = [], []
    for line in (tmp_path / "cpp" / "t").read_text().splitlines():
        f = line.split("\t")
        if f[0] == "#sample":
            names.append(f[1])
            mass.append(np.zeros(2 * B + 4, np.uint64))
        elif f[0].isdigit():
            mass[-1][int(f[0])] = int(f[4])
    assert names == ["a,b", "gut", "sea", "soil", "void"]
    words = np.concatenate(mass + [np.zeros(1, np.uint64)])
    r = ra.diversity_host(parent, bl, words, 5, (0.25, 1.0))
    assert files[0].decode() == hostio.diversity_table(names, (0.25, 1.0), r.values)
    lines = files[0].decode().splitlines()
    assert lines[0] == "#diversity\t5\t2" and lines[1].endswith("\trooted_pd_0.25\tbwpd_0.25\trooted_pd_1\tbwpd_1") and lines[-1] == "#samples_without_mass\t1"
    assert lines[-2] == "void" + "\tnan" * 9
