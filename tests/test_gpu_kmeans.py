"""The phylogenetic k-means on the device (rk_kmeans_device) against its host twin, word for word -- assign, the bits
of dist, sizes, the bits of within, info and the centroids --, every rung of the distance kernel's ladder, the workspace and output
rules, a pooled batch end to end, and the neighbours that share the profile stage."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, hostio, synth
from tests import kmeans_ref as K
from tests import kr_ref as R
from tests import squash_ref as Q
from tests.test_kmeans_host import PLANTED, is_planted_partition, planted_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300


def to_dev(m):
    import torch
    return torch.from_numpy(np.ascontiguousarray(m).view(np.int64)).cuda()


def download(r):
    import torch
    torch.cuda.synchronize()
    host = lambda t, dt: t.cpu().numpy().view(dt)
    return ra.KMeans(host(r.assign, np.uint32), host(r.dist, np.float64), host(r.sizes, np.uint32), host(r.within, np.float64), host(r.info, np.uint32),
                     None if r.centroids is None else r.centroids.cpu().numpy())


def check_against_host(parent, bl, m, S, k, max_rounds=50, seeds=None):
    et = ra.EdgeTree(parent, bl)
    try:
        got = download(et.kmeans(to_dev(m), S, k, max_rounds, seeds=seeds, centroids=True))
    finally:
        et.close()
    want = ra.kmeans_host(parent, bl, m, S, k, max_rounds, seeds=seeds)
    assert K.same(got, want), (len(parent), S, k, got.info, want.info)
    return got


@pytest.mark.parametrize("B,S,k", [(1, 2, 1), (2, 3, 2), (999, 65, 3), (999, 130, 8), (2049, 65, 9), (2049, 257, 17), (4500, 130, 64), (4500, 257, 2), (300, 4100, 5)])
def test_device_equals_host_twin_word_for_word(B, S, k):
    """B on both sides of a chunk edge and over three chunks, ids out of pre-order; S on both sides of the wave's 64 samples and of the
    update's group of 256, and past RK_SQUASH_MAX_SAMPLES; k on both sides of every rung of the ladder and of a second centroid group"""
    parent, bl = R.random_tree(B, 40 + B)
    got = check_against_host(parent, bl, R.sample_buffer(B, S, 50 + S), S, k)
    assert got.info[0] == min(k, S) and got.info[1] == S and got.sizes.sum() == S


def test_empty_identical_and_huge_samples():
    for B, S, k, seed in ((2049, 65, 4, 12), (300, 6, 3, 14)):
        parent, bl = R.random_tree(B, seed - 1)
        got = check_against_host(parent, bl, R.special_buffer(B, S, seed), S, k)
        assert got.assign[1] == K.NONE and R.bits(got.dist[1]) == 0 and got.info[1] == S - 1
        assert got.assign[2] == got.assign[3] and R.bits(got.dist[2]) == R.bits(got.dist[3])


def test_no_sample_with_mass_and_one():
    B, S, k = 300, 5, 3
    parent, bl = R.random_tree(B, 8)
    m = np.zeros(S * (2 * B + 4) + 1, np.uint64)
    got = check_against_host(parent, bl, m, S, k)
    assert got.info.tolist() == [0, 0, 0, 1] and (got.assign == K.NONE).all() and not got.centroids.any()
    m[3 * (2 * B + 4) + 7] = 99
    got = check_against_host(parent, bl, m, S, k)
    assert got.info.tolist() == [1, 1, 2, 1] and got.sizes.tolist() == [1, 0, 0]


def test_callers_seeds():
    B, S = 999, 70
    parent, bl = R.random_tree(B, 3)
    W = 2 * B + 4
    m = R.sample_buffer(B, S, 6)
    m[4 * W:4 * W + B] = 0
    got = check_against_host(parent, bl, m, S, 3, seeds=[66, 2, 5])
    assert got.info[0] == 3 and got.assign[4] == K.NONE
    got = check_against_host(parent, bl, m, S, 2, seeds=[1, 4])  # sample 4 has no mass: status 1, fillers
    assert got.info.tolist() == [2, S - 1, 0, 3] and (got.assign == K.NONE).all() and not got.dist.any() and not got.sizes.any() and not got.centroids.any()
    m[1 * W:1 * W + B] = m[0 * W:0 * W + B]  # both seeds the same sample: cluster 1 is empty after round one and keeps its profile
    got = check_against_host(parent, bl, m, S, 2, max_rounds=1, seeds=[0, 1])
    assert got.sizes.tolist() == [S - 1, 0] and got.info.tolist() == [2, S - 1, 1, 0]


@pytest.mark.parametrize("kind", ["caterpillar", "random"])
def test_largest_tree(kind):
    B = 65535
    parent, bl = R.caterpillar(B) if kind == "caterpillar" else R.random_tree(B, 9)
    got = check_against_host(parent, bl, R.sample_buffer(B, 3, 77), 3, 2)
    assert got.info.tolist() == [2, 3, 2, 1] and sorted(got.sizes.tolist()) == [1, 2]


def test_planted_partition_on_the_device():
    B, S, k, seed = PLANTED
    parent, bl, m, label = planted_case(B, S, k, seed)
    got = check_against_host(parent, bl, m, S, k)
    assert got.info.tolist() == [k, S, 2, 1] and is_planted_partition(got.assign, label, k)
    one = check_against_host(parent, bl, m, S, k, max_rounds=1)
    assert one.info.tolist() == [k, S, 1, 0] and is_planted_partition(one.assign, label, k)


def test_every_rung_of_the_ladder_gives_the_same_bits(dev_lib, monkeypatch):
    """RK_KMEANS_KC (developer builds) forces the rung: 1, 2, 4 and 8 centroids a block on a shape of 8 centroids, and on one of 9,
    whose last group of every rung above 1 holds fewer centroids than the rung (the call itself picks the rung by the size of the grid:
    on shapes this small it is 1)"""
    for B, S, k in ((2049, 130, 8), (2049, 65, 9)):
        parent, bl = R.random_tree(B, 21)
        m = R.sample_buffer(B, S, 22)
        want = ra.kmeans_host(parent, bl, m, S, k, 50)
        for kc in ("1", "2", "4", "8"):
            monkeypatch.setenv("RK_KMEANS_KC", kc)
            et = ra.EdgeTree(parent, bl)
            try:
                got = download(et.kmeans(to_dev(m), S, k, 50, centroids=True))
            finally:
                et.close()
            assert K.same(got, want), (k, kc)


def test_workspace_and_output_rules():
    """the same call twice and on two streams gives the same bits; nothing is written beyond rk_kmeans_work_bytes or round any output; a
    short workspace, a NULL argument, S, k or max_rounds out of range and bad seeds are RK_ERR_INVALID and leave the outputs as they
    were; d_centroids may be NULL"""
    import torch
    lib = _lib.load()
    B, S, k, rounds = 2049, 67, 5, 50
    parent, bl = R.random_tree(B, 31)
    m = R.special_buffer(B, S, 32)
    want = ra.kmeans_host(parent, bl, m, S, k, rounds)
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)
        need = et.kmeans_work_bytes(S, k)
        assert need < et.kr_work_bytes(S) + S * S * 8 * 3  # no S x S partials
        guard = 4096
        sizes = {"assign": S * 4, "dist": S * 8, "sizes": k * 4, "within": k * 8, "info": 16, "centroids": k * 2 * B * 8}
        work = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device="cuda")

        def fresh():
            return {n: torch.full((b + 2 * guard,), 0x6B, dtype=torch.uint8, device="cuda") for n, b in sizes.items()}

        out = fresh()
        ptr = {n: t.data_ptr() + guard for n, t in out.items()}

        def call(work_bytes=need, masses=dm.data_ptr(), w=work.data_ptr(), S=S, k=k, rounds=rounds, seeds=None, stream=None, p=ptr, **null):
            st = stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream
            a = {n: (None if n in null else v) for n, v in p.items()}
            sd = None if seeds is None else np.asarray(seeds, np.uint32)
            return lib.rk_kmeans_device(et.handle, S, masses, k, rounds, None if sd is None else sd.ctypes.data, a["assign"], a["dist"], a["sizes"], a["within"], a["info"],
                                        a["centroids"], w, work_bytes, C.c_void_p(st))

        assert call(work_bytes=need - 1) == _lib.RK_ERR_INVALID and b"rk_kmeans_work_bytes" in lib.rk_last_error()
        for kw in (dict(assign=1), dict(dist=1), dict(sizes=1), dict(within=1), dict(info=1), dict(masses=None), dict(w=None), dict(S=0), dict(S=65536), dict(k=0),
                   dict(k=65), dict(rounds=0), dict(rounds=1025), dict(seeds=[0, 1, 2, 3, S]), dict(seeds=[0, 1, 2, 1, 4])):
            assert call(**kw) == _lib.RK_ERR_INVALID, kw
        assert lib.rk_kmeans_device(None, S, dm.data_ptr(), k, rounds, None, ptr["assign"], ptr["dist"], ptr["sizes"], ptr["within"], ptr["info"], None, work.data_ptr(),
                                    need, None) == _lib.RK_ERR_INVALID
        torch.cuda.synchronize()
        assert all((t == 0x6B).all() for t in out.values()) and (work == 0x5A).all()  # nothing was launched

        def now(bufs, at=guard):
            b = {n: t.cpu().numpy()[at:at + sizes[n]].copy() for n, t in bufs.items()}
            return ra.KMeans(b["assign"].view(np.uint32), b["dist"].view(np.float64), b["sizes"].view(np.uint32), b["within"].view(np.float64), b["info"].view(np.uint32),
                             b["centroids"].view(np.float64).reshape(k, 2, B))

        for again in range(2):  # the second call runs on the workspace the first one left
            assert call() == _lib.RK_OK
            torch.cuda.synchronize()
            assert K.same(now(out), want), again
            for n, t in out.items():
                whole = t.cpu().numpy()
                assert (whole[:guard] == 0x6B).all() and (whole[guard + sizes[n]:] == 0x6B).all(), n
            assert (work[need:] == 0x5A).all()
        out2 = fresh()
        assert call(p={n: t.data_ptr() + guard for n, t in out2.items()}, centroids=1) == _lib.RK_OK  # no centroids wanted
        torch.cuda.synchronize()
        assert K.same(now(out2), want, centroids=False) and (out2["centroids"] == 0x6B).all()
        s2 = torch.cuda.Stream()
        out3 = fresh()
        work3 = torch.empty((need,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert call(p={n: t.data_ptr() + guard for n, t in out3.items()}, w=work3.data_ptr(), stream=s2) == _lib.RK_OK  # another stream
        s2.synchronize()
        assert K.same(now(out3), want)
        assert lib.rk_kmeans_work_bytes(et.handle, 0, k) == 0 and lib.rk_kmeans_work_bytes(et.handle, 65536, k) == 0 and lib.rk_kmeans_work_bytes(et.handle, S, 65) == 0
        assert lib.rk_kmeans_work_bytes(et.handle, 65535, 64) > 0
    finally:
        et.close()


def test_pooled_batch_end_to_end():
    """a pooled batch through rk_place_batch_masses_samples, which leaves the sample buffer on the device in the handle: rk_kmeans_batch
    on it equals the host twin on the downloaded buffer"""
    n_nodes, S, k = 75, 5, 3
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
        got = et.kmeans_batch(db, S, k, 50, centroids=True)                  # the buffer where the call left it
        got2 = et.kmeans_batch(db, S, k, 50, masses=words, centroids=True)   # the host copy, uploaded
        want = ra.kmeans_host(parent, bl, words, S, k, 50)
        assert K.same(got, want) and K.same(got2, want) and K.same(want, K.kmeans_ref(parent, bl, words, S, k, 50))
        assert want.info[1] == S - 1 and want.assign[S - 1] == K.NONE
        with pytest.raises(ra.RkError):
            et.kmeans_batch(db, S + 1, k, 50)                                # not the buffer of S + 1 samples
    finally:
        et.close()
        db.close()


def test_drivers_kmeans(tmp_path):
    """`--kmeans` on a small database with `--sample-sep _`: rk_place and the Python tool write identical bytes (and rk_place the same with
    --masses), the table is the host twin's on the per-sample tables' masses, alongside --kr and --squash, and without --sample-sep or
    without --kmeans-k it is a usage error from both"""
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
        run(cmd, only, ["--masses-only", str(only / "t"), "--sample-sep", "_", "--kmeans", str(only / "km"), "--kmeans-k", "3", "--kr", str(only / "kr"), "--squash",
                        str(only / "sq")])
        files.append((only / "km").read_bytes())
        assert (only / "kr").exists() and (only / "sq").exists()
        if name == "cpp":  # the buffer summed on the host and uploaded: the same file (one driver is enough: the twins share the call)
            run(cmd, full, ["--out", str(full / "o.jplace"), "--masses", str(full / "t"), "--sample-sep", "_", "--kmeans", str(full / "km"), "--kmeans-k", "3",
                            "--kmeans-rounds", "100"])
            files.append((full / "km").read_bytes())
        r = run(cmd, tmp_path / (name + "_bad"), ["--masses-only", str(tmp_path / (name + "_bad_t")), "--kmeans", str(tmp_path / (name + "_bad_km")), "--kmeans-k", "3"],
                ok=False)
        assert "--kmeans" in r.stderr and "--sample-sep" in r.stderr and not (tmp_path / (name + "_bad_km")).exists()
        r = run(cmd, tmp_path / (name + "_bad2"), ["--masses-only", str(tmp_path / (name + "_bad2_t")), "--sample-sep", "_", "--kmeans", str(tmp_path / (name + "_bad2_km"))],
                ok=False)
        assert "--kmeans-k" in r.stderr and not (tmp_path / (name + "_bad2_km")).exists()
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
    r = ra.kmeans_host(parent, bl, words, 5, 3)
    assert r.info[0] == 3 and r.info[1] == 4
    assert files[0].decode() == hostio.kmeans_table(names, 3, r.assign, r.dist, r.sizes, r.within, r.info)
    lines = files[0].decode().splitlines()
    assert lines[0].startswith("#kmeans\t5\t3\t3\t4\t") and lines[-1] == "#samples_without_mass\t1" and lines[-2] == "void\t-\t0"


def test_the_neighbours_keep_their_bits():
    """KR, squash and edge PCA share the profile stage with k-means: on one buffer each still gives its host twin's bits"""
    import torch
    B, S = 2049, 67
    parent, bl = R.random_tree(B, 31)
    m = R.special_buffer(B, S, 32)
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)
        et.kmeans(dm, S, 4, 5)
        D = et.kr_distances(dm, S)
        merges, n = et.squash(dm, S)
        raw, info = et.epca(dm, S, 3, 10)
        torch.cuda.synchronize()
        assert (R.bits(D.cpu().numpy()) == R.bits(ra.kr_distances_host(parent, bl, m, S))).all()
        want, n_want = ra.squash_host(parent, bl, m, S)
        assert int(n.cpu()[0]) == n_want and Q.same_rows(merges.cpu().numpy().reshape(-1).view(Q.SQUASH_MERGE), want)
        raw_want, info_want = ra.epca_host(parent, bl, m, S, 3, 10)
        assert (R.bits(raw.cpu().numpy()) == R.bits(raw_want)).all() and (info.cpu().numpy().view(np.uint32) == info_want).all()
    finally:
        et.close()
