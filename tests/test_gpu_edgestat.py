"""The edge statistics on the device (rk_edgestat_device) against the host twin, word for word, on shapes on both
sides of a wave, of the crossover between the two ranking forms, of the powers of two the sort pads to and of the two edges a block of
the counting form takes; tie-heavy buffers and metadata; the unusable-column rule; the largest tree; the known answers; two streams
on one tree handle; the workspace and output rules; a pooled batch end to end; the neighbours that run on the same buffers; and the
two drivers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, edgestats as ES, hostio, synth
from tests import edgestat_ref as E
from tests import kr_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300


def to_dev(m):
    import torch
    return torch.from_numpy(np.ascontiguousarray(m).view(np.int64)).cuda()


def check_against_host(parent, m, S, meta):
    import torch
    et = ra.EdgeTree(parent, np.ones(len(parent), np.float32))
    try:
        raw, info = ES.edgestat(et, to_dev(m), S, meta)
        torch.cuda.synchronize()
        raw, info = raw.cpu().numpy().view(np.uint64), info.cpu().numpy().view(np.uint32)
    finally:
        et.close()
    want, want_info = ES.edgestat_host(parent, m, S, meta)
    assert (info == want_info).all(), (info, want_info)
    assert raw.shape == want.shape and (raw == want).all(), (len(parent), S, np.flatnonzero(raw != want)[:8])
    return raw, info


@pytest.mark.parametrize("B,S,F", E.shapes(ES.COUNT_MAX_SAMPLES))
def test_device_equals_host_twin_word_for_word(B, S, F):
    parent, _ = R.random_tree(B, 40 + B)
    _, info = check_against_host(parent, R.sample_buffer(B, S, 50 + S), S, E.metadata(S, F, 60 + S))
    assert info.tolist() == [S, 0]


@pytest.mark.parametrize("kind", ["caterpillar", "random"])
def test_largest_tree(kind):
    B = 65535
    parent, _ = R.caterpillar(B) if kind == "caterpillar" else R.random_tree(B, 9)
    check_against_host(parent, R.sample_buffer(B, 3, 77), 3, E.metadata(3, 1, 78))


@pytest.mark.parametrize("S", [70, 300])
def test_tie_heavy_buffers_and_metadata(S):
    """empty, identical and huge samples; a buffer in which nine edges in ten are zero in nine samples in ten; metadata with repeated
    values, negative values and values up to 1e100 -- in both ranking forms"""
    B = 300
    parent, _ = R.random_tree(B, 13)
    meta = E.metadata(S, 4, 16)
    _, info = check_against_host(parent, R.special_buffer(B, S, 14), S, meta)
    assert info.tolist() == [S - 1, 0]
    check_against_host(parent, E.sparse_buffer(B, S, 15), S, meta)


@pytest.mark.parametrize("S", [12, 200])
def test_unusable_columns_on_the_device(S):
    B = 30
    parent, _ = R.random_tree(B, 31)
    m = R.special_buffer(B, S, 32)  # sample 1 is empty
    meta = E.metadata(S, 3, 33)
    good, _ = check_against_host(parent, m, S, meta)
    for bad_value in (np.nan, np.inf):
        quiet, loud = meta.copy(), meta.copy()
        quiet[1, 1] = bad_value  # in the inactive sample only: usable
        loud[1, 4] = bad_value
        raw, info = check_against_host(parent, m, S, quiet)
        assert info[1] == 0 and (raw == good).all()
        raw, info = check_against_host(parent, m, S, loud)
        assert info[1] == 2 and (raw[B * 18 + 3:B * 18 + 6] == np.array([E.NAN_BITS, E.NAN_BITS, 0], np.uint64)).all()


def test_no_active_sample_on_the_device():
    B, S = 9, 3
    parent, _ = R.random_tree(B, 41)
    raw, info = check_against_host(parent, np.zeros(S * (2 * B + 4) + 1, np.uint64), S, E.metadata(S, 2, 42))
    assert info.tolist() == [0, 0] and not raw.any()


def test_known_answers_on_the_device():
    from tests.test_edgestat_host import check_golden, golden_case
    g, parent, m, S, meta = golden_case()
    check_golden(g, *check_against_host(parent, m, S, meta))


def test_workspace_streams_and_output_rules():
    """two calls on two streams share one tree handle, each with a workspace of its own; nothing is written beyond
    rk_edgestat_work_bytes or round the outputs; a short, NULL or misaligned workspace, a NULL argument, S or F out of range are
    RK_ERR_INVALID, launch nothing and leave the outputs as they were"""
    import torch
    lib = _lib.load()
    B, S, F = 2049, 67, 2
    parent, bl = R.random_tree(B, 31)
    m, m2 = R.special_buffer(B, S, 32), R.sample_buffer(B, S, 33)
    meta = E.metadata(S, F, 34)
    want, want_info = ES.edgestat_host(parent, m, S, meta)
    want2, _ = ES.edgestat_host(parent, m2, S, meta)
    et = ra.EdgeTree(parent, bl)
    try:
        dm, dm2, dmeta = to_dev(m), to_dev(m2), torch.from_numpy(meta).cuda()
        need = lib.rk_edgestat_work_bytes(et.handle, S, F)
        assert need > 0
        guard, out_bytes = 4096, E.out_words(B, F) * 8
        work = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device="cuda")
        out = torch.full((out_bytes + 2 * guard,), 0x6B, dtype=torch.uint8, device="cuda")
        inf = torch.full((8 + 2 * guard,), 0x6B, dtype=torch.uint8, device="cuda")

        def call(work_bytes=need, masses=dm.data_ptr(), w=work.data_ptr(), S=S, F=F, g=dmeta.data_ptr(), o=out.data_ptr() + guard, i=inf.data_ptr() + guard, stream=None,
                 tree=et.handle):
            st = stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream
            return lib.rk_edgestat_device(tree, S, masses, F, g, o, i, w, work_bytes, C.c_void_p(st))

        assert call(work_bytes=need - 1) == _lib.RK_ERR_INVALID and b"rk_edgestat_work_bytes" in lib.rk_last_error()
        for kw in (dict(w=None), dict(w=work.data_ptr() + 8), dict(masses=None), dict(o=None), dict(i=None), dict(g=None), dict(S=0), dict(S=4097), dict(F=9), dict(tree=None)):
            assert call(**kw) == _lib.RK_ERR_INVALID, kw
        torch.cuda.synchronize()
        assert (out == 0x6B).all() and (inf == 0x6B).all() and (work == 0x5A).all()  # nothing was launched
        for again in range(2):  # the second call runs on the workspace the first one left
            assert call() == _lib.RK_OK
            torch.cuda.synchronize()
            whole, iw = out.cpu().numpy(), inf.cpu().numpy()
            assert (whole[guard:guard + out_bytes].view(np.uint64) == want).all() and (iw[guard:guard + 8].view(np.uint32) == want_info).all(), again
            assert (whole[:guard] == 0x6B).all() and (whole[guard + out_bytes:] == 0x6B).all() and (work[need:] == 0x5A).all()
            assert (iw[:guard] == 0x6B).all() and (iw[guard + 8:] == 0x6B).all()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        o1, o2 = (torch.empty((E.out_words(B, F),), dtype=torch.int64, device="cuda") for _ in range(2))
        i1, i2 = (torch.empty((2,), dtype=torch.int32, device="cuda") for _ in range(2))
        w2 = torch.empty((need,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert call(o=o1.data_ptr(), i=i1.data_ptr(), stream=s1) == _lib.RK_OK
        assert call(o=o2.data_ptr(), i=i2.data_ptr(), masses=dm2.data_ptr(), w=w2.data_ptr(), stream=s2) == _lib.RK_OK
        s1.synchronize()
        s2.synchronize()
        assert (o1.cpu().numpy().view(np.uint64) == want).all() and (o2.cpu().numpy().view(np.uint64) == want2).all()
        assert call(F=0, g=None) == _lib.RK_OK  # no column: no metadata is read
        torch.cuda.synchronize()
        assert lib.rk_edgestat_work_bytes(et.handle, 0, 0) == 0 and lib.rk_edgestat_work_bytes(et.handle, 4097, 0) == 0 and lib.rk_edgestat_work_bytes(et.handle, S, 9) == 0
        assert lib.rk_edgestat_work_bytes(et.handle, 4096, 8) > 0
    finally:
        et.close()


def test_pooled_batch_end_to_end():
    """a pooled batch through rk_place_batch_masses_samples, which leaves the sample buffer on the device in the handle:
    rk_edgestat_batch on it, and on the uploaded copy, equals the host twin on the downloaded buffer; metadata that is not finite is
    refused on the host"""
    n_nodes, S = 75, 5
    sdb, genome = synth.make_clade_db(k=8, n_branches=n_nodes, genome_len=12_000, mean_row=6, seed=13)
    seq, _ = synth.make_clade_reads(genome, 600, 120, seed=10)
    n = 600
    off = np.arange(n + 1, dtype=np.uint64) * 120
    sample = np.random.default_rng(3).integers(0, S - 1, n).astype(np.uint32)  # sample S - 1 stays empty
    parent, bl = R.random_tree(n_nodes, 5)
    meta = E.metadata(S, 2, 6)
    db = ra.PhyloKmerDB.from_synth(sdb, device=0)
    et = ra.EdgeTree(parent, bl)
    try:
        words, flags, _ = ra.PlacementProcess(db).processQueriesMassesSamples(seq, off, S, sample)
        assert (flags & 1).sum() > 100
        got = ES.edgestat_batch(et, db, S, meta)                  # the buffer where the call left it
        got2 = ES.edgestat_batch(et, db, S, meta, masses=words)   # the host copy, uploaded
        want = ES.edgestat_host(parent, words, S, meta)
        for g in (got, got2):
            assert (g[0] == want[0]).all() and (g[1] == want[1]).all()
        r = ES.edgestat_finish(n_nodes, S, *got, ("a", "b"))
        assert r.n_active == S - 1 and r.unusable == 0 and (r.table[:, 0] >= 0).all() and (r.table[:, 1] > 0).any()
        assert (np.abs(r.table[:, 8:][~np.isnan(r.table[:, 8:])]) <= 1 + 1e-12).all()
        bad = meta.copy()
        bad[1, S - 1] = np.nan  # even in the empty sample: the drivers never rely on the device rule
        with pytest.raises(ra.RkError, match="not finite"):
            ES.edgestat_batch(et, db, S, bad)
        with pytest.raises(ra.RkError):
            ES.edgestat_batch(et, db, S + 1, E.metadata(S + 1, 2, 6))  # not the buffer of S + 1 samples
    finally:
        et.close()
        db.close()


def test_the_neighbours_keep_their_bits():
    """KR and edge PCA on the same buffers and the same tree, run before and after an edge-statistics call, give the bits they gave"""
    import torch
    B, S = 2049, 67
    parent, bl = R.random_tree(B, 31)
    m = R.special_buffer(B, S, 32)
    meta = E.metadata(S, 2, 34)
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)

        def neighbours():
            D, (raw, info) = et.kr_distances(dm, S), et.epca(dm, S, 3, 4)
            torch.cuda.synchronize()
            return D.cpu().numpy(), raw.cpu().numpy(), info.cpu().numpy()

        before = neighbours()
        raw, info = ES.edgestat(et, dm, S, meta)
        after = neighbours()
        want, want_info = ES.edgestat_host(parent, m, S, meta)
        assert (raw.cpu().numpy().view(np.uint64) == want).all() and (info.cpu().numpy().view(np.uint32) == want_info).all()
        for a, b in zip(before, after):
            assert (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all()
        assert (R.bits(before[0]) == R.bits(ra.kr_distances_host(parent, bl, m, S))).all()
        assert (R.bits(before[1]) == R.bits(ra.epca_host(parent, bl, m, S, 3, 4)[0])).all()
    finally:
        et.close()


def test_drivers_edge_stats(tmp_path):
    """`--edge-stats FILE --metadata TSV` on a small database with `--sample-sep _`: rk_place (from a database image) and the Python
    tool write identical bytes, profile-only and placing; the table is edge_stats_table of the host twin on the per-sample tables'
    masses; without --metadata the table has its fixed columns; a sample of the run without a line ends both drivers with the same
    sentence and no table"""
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
    meta_text = "sample\tpH\tdepth\nsoil\t6.5\t-10\ngut\t7.25\t20\nvoid\t1\t1\nmoon\t0\t0\nsea\t8.125\t-10\na,b\t5\t3e1\n"
    (tmp_path / "meta.tsv").write_text(meta_text)
    (tmp_path / "short.tsv").write_text("sample\tpH\nsoil\t6.5\ngut\t7.25\nsea\t8\nvoid\t1\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(cmd, d, args, ok=True):
        d.mkdir()
        r = subprocess.run(cmd + ["--fasta", str(tmp_path / "q.fasta"), "--logs", str(d / "logs")] + args, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT, env=env)
        assert (r.returncode == 0) == ok, r.stderr[-3000:]
        return r

    py, cpp = [sys.executable, "-m", "rappas_amd.tools.place"], [exe]
    jsondb, image = ["--jsondb", str(tmp_path / "db.json")], ["--dbimage", str(tmp_path / "db.rkdb")]
    with_meta = ["--metadata", str(tmp_path / "meta.tsv")]
    d = tmp_path / "py"
    run(py, d, jsondb + ["--save-dbimage", str(tmp_path / "db.rkdb"), "--masses-only", str(d / "t"), "--sample-sep", "_", "--edge-stats", str(d / "es.tsv")] + with_meta
        + ["--kr", str(d / "kr"), "--diversity", str(d / "div"), "--epca", str(d / "epca"), "--squash", str(d / "sq"), "--kmeans", str(d / "km"), "--kmeans-k", "2"])
    assert all((d / n).exists() for n in ("kr", "div", "epca", "sq", "km"))
    d = tmp_path / "cpp"
    run(cpp, d, image + ["--masses-only", str(d / "t"), "--sample-sep", "_", "--edge-stats", str(d / "es.tsv")] + with_meta)
    d = tmp_path / "cpp_placing"
    run(cpp, d, image + ["--out", str(d / "o.jplace"), "--masses", str(d / "t"), "--sample-sep", "_", "--edge-stats", str(d / "es.tsv")] + with_meta)
    d = tmp_path / "py_placing"
    run(py, d, image + ["--out", str(d / "o.jplace"), "--masses", str(d / "t"), "--sample-sep", "_", "--edge-stats", str(d / "es.tsv")] + with_meta)
    files = [(tmp_path / n / "es.tsv").read_bytes() for n in ("py", "cpp", "cpp_placing", "py_placing")]
    assert files[0] == files[1] == files[2] == files[3]
    plain = []
    for name, cmd in (("py", py), ("cpp", cpp)):
        d = tmp_path / (name + "_plain")
        run(cmd, d, image + ["--masses-only", str(d / "t"), "--sample-sep", "_", "--edge-stats", str(d / "es.tsv")])
        plain.append((d / "es.tsv").read_bytes())
        bad = tmp_path / (name + "_bad")
        r = run(cmd, bad, image + ["--masses-only", str(bad / "t"), "--sample-sep", "_", "--edge-stats", str(bad / "es.tsv"), "--metadata", str(tmp_path / "short.tsv")], ok=False)
        assert r.returncode == 1 and r.stderr.strip().endswith("--metadata: the sample 'a,b' of the run has no line") and os.listdir(bad) == []
    assert plain[0] == plain[1]
    # the table: the host twin over the masses the per-sample tables print, on the database's tree
    tree = hostio.parse_newick(nwk)
    B = len(tree.nodes)
    parent = np.array([nd.parent.id if nd.parent is not None else -1 for nd in tree.nodes], np.int32)
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
    features, rows = hostio.parse_metadata(meta_text)
    meta = hostio.metadata_of_samples(names, (features, rows))
    assert meta.tolist() == [[5.0, 7.25, 8.125, 6.5, 1.0], [30.0, 20.0, -10.0, -10.0, 1.0]]
    r = ES.edgestat_finish(B, 5, *ES.edgestat_host(parent, words, 5, meta), features)
    assert files[0].decode() == hostio.edge_stats_table(names, features, r.n_active, r.table, r.feature_table)
    r0 = ES.edgestat_finish(B, 5, *ES.edgestat_host(parent, words, 5))
    assert plain[0].decode() == hostio.edge_stats_table(names, [], r0.n_active, r0.table, r0.feature_table)
    lines = files[0].decode().splitlines()
    assert lines[0] == f"#edge_stats\t5\t{B}\t2\t4" and lines[1].endswith("\timb_pearson_depth\timb_spearman_depth") and lines[-1] == "#samples_without_mass\t1"
    assert lines[2 + B] == "#features" and lines[3 + B].startswith("pH\t6.71875\t") and len(lines) == B + 6
