"""The host twin of the phylogenetic k-means (rk_kmeans_host) against the numpy restatement of the header's definition,
bit for bit, the edge cases of the definition, a known answer, the caller's seeds, the exact run, the planted partition, the refused
arguments and the two kmeans_table writers.  No GPU."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, hostio
from tests import kmeans_ref as K
from tests import kr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TREES = {"random": R.random_tree, "caterpillar": lambda B, seed: R.caterpillar(B, seed), "star": lambda B, seed: R.star(B, seed)}


def host(parent, bl, m, S, k, **kw):
    return ra.kmeans_host(parent, bl, m, S, k, **kw)


@pytest.mark.parametrize("kind,B,S,k", [(kind, B, S, k) for kind in TREES for B, S, k in ((1, 2, 1), (1, 12, 3), (2, 3, 2), (2, 12, 9), (40, 3, 9), (40, 12, 2))]
                         + [("random", 40, 257, 3), ("caterpillar", 40, 600, 9), ("star", 40, 257, 9), ("random", 300, 12, 9), ("star", 300, 257, 2),
                            ("caterpillar", 300, 2, 1), ("random", 2049, 12, 3), ("caterpillar", 2049, 3, 9), ("star", 2049, 2, 2)])
def test_host_twin_equals_the_definition_bit_for_bit(kind, B, S, k):
    """B on both sides of a chunk edge, S on both sides of the update's group of 256 samples (257, 600: three groups), k below, at and
    above the number of samples"""
    parent, bl = TREES[kind](B, 10 + B)
    m = R.sample_buffer(B, S, 20 + S + k)
    want = K.kmeans_ref(parent, bl, m, S, k)
    got = host(parent, bl, m, S, k)
    assert K.same(got, want), (got.info, want.info)
    assert want.info[0] == min(k, S) and want.info[1] == S and want.info[3] == 1 and want.sizes.sum() == S


def test_empty_identical_and_huge_samples():
    for B, S, k, seed in ((2049, 7, 4, 12), (300, 6, 3, 14)):
        parent, bl = R.random_tree(B, seed - 1)
        m = R.special_buffer(B, S, seed)
        got = host(parent, bl, m, S, k)
        assert K.same(got, K.kmeans_ref(parent, bl, m, S, k))
        assert got.assign[1] == K.NONE and R.bits(got.dist[1]) == 0 and got.info[1] == S - 1 and got.sizes.sum() == S - 1
        assert got.assign[2] == got.assign[3] and R.bits(got.dist[2]) == R.bits(got.dist[3])
        # sample 2 as a seed: its copy is at +0.0 from it in round one
        one = host(parent, bl, m, S, 2, max_rounds=1, seeds=[2, 0])
        assert K.same(one, K.kmeans_ref(parent, bl, m, S, 2, 1, [2, 0]))
        assert one.assign[3] == 0 and R.bits(one.dist[3]) == 0 and R.bits(one.dist[2]) == 0 and one.info[3] == 0


def test_fewer_active_samples_than_clusters_none_and_one():
    B, S, k = 300, 5, 4
    parent, bl = R.random_tree(B, 8)
    W = 2 * B + 4
    m = R.sample_buffer(B, S, 3)
    m[0 * W:0 * W + B] = 0
    m[2 * W:2 * W + B] = 0
    m[3 * W:3 * W + B] = 0
    got = host(parent, bl, m, S, k)  # two active samples, four clusters
    assert K.same(got, K.kmeans_ref(parent, bl, m, S, k))
    assert got.info.tolist() == [2, 2, 2, 1] and got.sizes.tolist() == [1, 1, 0, 0] and not got.within.any() and not got.centroids[2:].any()
    assert got.assign.tolist() == [K.NONE, 0, K.NONE, K.NONE, 1]
    m[:] = 0
    got = host(parent, bl, m, S, k)  # none
    assert K.same(got, K.kmeans_ref(parent, bl, m, S, k)) and got.info.tolist() == [0, 0, 0, 1]
    assert (got.assign == K.NONE).all() and not got.dist.any() and not got.sizes.any() and not got.centroids.any()
    m[3 * W + 7] = 99
    got = host(parent, bl, m, S, k)  # one
    assert K.same(got, K.kmeans_ref(parent, bl, m, S, k)) and got.info.tolist() == [1, 1, 2, 1]
    assert got.assign.tolist() == [K.NONE] * 3 + [0, K.NONE] and got.sizes.tolist() == [1, 0, 0, 0] and not got.dist.any()


def test_the_same_bits_from_every_thread_count():
    B, S, k = 300, 70, 5
    parent, bl = R.random_tree(B, 4)
    m = R.special_buffer(B, S, 5)
    want = host(parent, bl, m, S, k, threads=1)
    for threads in (2, 5, 16, 0):
        assert K.same(host(parent, bl, m, S, k, threads=threads), want)


def test_known_answer_by_hand():
    """root 0 with the leaves 1 (edge 1, h = 0.5) and 2 (edge 2, h = 1).  Sample 0 sits on leaf 1, sample 1 on leaf 2, sample 2 has 3/4 on
    leaf 1 and 1/4 on leaf 2.  D(0, 1) = 0.5 + 1 = 1.5, D(0, 2) = (0.5 + 1) / 4 = 0.375, D(1, 2) = 1.125: the seeds are 0, then 1
    (the farthest from 0); round one puts sample 2 with sample 0, their mean has 7/8 on leaf 1, round two finds the same clusters with
    both members at (0.5 + 1) / 8 = 0.1875 from it."""
    parent, bl = np.array([-1, 0, 0], np.int32), np.array([0, 1, 2], np.float32)
    W = 10
    m = np.zeros(3 * W + 1, np.uint64)
    m[0 * W + 1] = 8
    m[1 * W + 2] = 5
    m[2 * W + 1], m[2 * W + 2] = 3, 1
    got = host(parent, bl, m, 3, 2)
    assert got.info.tolist() == [2, 3, 2, 1] and got.assign.tolist() == [0, 1, 0] and got.sizes.tolist() == [2, 1]
    assert got.dist.tolist() == [0.1875, 0.0, 0.1875] and got.within.tolist() == [0.375, 0.0]
    assert got.centroids.tolist() == [[[1.0, 0.875, 0.125], [1.0, 0.0, 0.0]], [[1.0, 0.0, 1.0], [1.0, 0.0, 0.0]]]
    assert K.same(got, K.kmeans_ref(parent, bl, m, 3, 2))
    one = host(parent, bl, m, 3, 2, max_rounds=1)  # the round's distances, the updated centroids
    assert one.info.tolist() == [2, 3, 1, 0] and one.dist.tolist() == [0.0, 0.0, 0.375] and (one.centroids == got.centroids).all()


def test_callers_seeds():
    B, S = 40, 9
    parent, bl = R.random_tree(B, 3)
    W = 2 * B + 4
    m = R.sample_buffer(B, S, 6)
    m[4 * W:4 * W + B] = 0
    for seeds, text in (([0, S], b"seeds[1]=9"), ([3, 5, 3], b"both sample 3")):
        with pytest.raises(ra.RkError) as e:
            host(parent, bl, m, S, len(seeds), seeds=seeds)
        assert e.value.code == _lib.RK_ERR_INVALID and text in _lib.load().rk_last_error()
    got = host(parent, bl, m, S, 3, seeds=[7, 2, 5])
    assert K.same(got, K.kmeans_ref(parent, bl, m, S, 3, seeds=[7, 2, 5])) and got.info[0] == 3 and got.info[3] == 1 and got.assign[4] == K.NONE
    got = host(parent, bl, m, S, 2, seeds=[1, 4])  # sample 4 has no mass
    assert K.same(got, K.kmeans_ref(parent, bl, m, S, 2, seeds=[1, 4])) and got.info.tolist() == [2, S - 1, 0, 3]
    assert (got.assign == K.NONE).all() and not got.dist.any() and not got.sizes.any() and not got.within.any() and not got.centroids.any()


def test_a_cluster_that_loses_every_member_keeps_its_profile():
    """samples 0 and 1 are the same and both are seeds: every tie goes to cluster 0, so cluster 1 is empty after round one; the update
    of that round leaves it its seed's profile (with which it wins its two samples back in round two)"""
    B, S = 40, 6
    parent, bl = R.random_tree(B, 5)
    W = 2 * B + 4
    m = R.sample_buffer(B, S, 9)
    m[1 * W:1 * W + B] = m[0 * W:0 * W + B]
    one = host(parent, bl, m, S, 2, max_rounds=1, seeds=[0, 1])
    assert K.same(one, K.kmeans_ref(parent, bl, m, S, 2, 1, seeds=[0, 1]))
    assert one.sizes.tolist() == [S, 0] and one.info.tolist() == [2, S, 1, 0] and R.bits(one.within[1]) == 0
    _, u, v, _ = K.profiles(parent, bl, m, S)
    assert (R.bits(one.centroids[1, 0]) == R.bits(u[1])).all() and (R.bits(one.centroids[1, 1]) == R.bits(v[1])).all()
    assert not (R.bits(one.centroids[0, 0]) == R.bits(u[0])).all()
    got = host(parent, bl, m, S, 2, seeds=[0, 1])
    assert K.same(got, K.kmeans_ref(parent, bl, m, S, 2, seeds=[0, 1])) and got.assign[0] == got.assign[1]


@pytest.mark.parametrize("B,S,i", [(40, 8, 1), (120, 12, 3), (300, 10, 4)])
def test_order_and_accuracy_against_the_exact_run(B, S, i):
    """Seeds, assignments of every round, the number of rounds and convergence equal the exact run's, and every distance lies within
        (2B + 2) * 2^-52 * exact + (S + 1) * 2^-52 * sum(h)
    of the exact one.  The first part is the bound of the KR pair sum (test_samples_host.test_accuracy_against_exact_rationals) for
    operands that are correctly rounded quotients.  The second is what a centroid adds: its entry is the ordered sum of n <= S entries
    in 0..1 -- n - 1 additions (the first, onto +0.0, is exact), each rounding at most 2^-53 of a partial sum that never exceeds the whole
    sum, however the partials are grouped -- divided by n with one more rounding: at most n * 2^-53 away from the exact mean, on each
    of the two profiles of a term, weighted by h.  A centroid is summed afresh from the samples every round, so nothing accumulates
    over the rounds (the bound first proposed for this test, 8 * (S / 256 + 2) * rounds, counts a rounding a group and a factor a
    round; the derivation gives a rounding a member and none a round.  At these shapes S + 1 is the smaller of the two).
    First the exact run's gaps must decide the run: the farthest and the second-farthest candidate of every seeding step, and the
    nearest and the second-nearest centroid of every sample in every round, differ by more than the two bounds together."""
    k = 3
    parent, bl = R.random_tree(B, 100 + i)
    m = R.sample_buffer(B, S, 200 + i)
    ex = K.kmeans_exact(parent, bl, m, S, k)
    root, _ = R.preorder(parent)
    sum_h = sum(Fraction(float(np.float32(bl[x]))) / 2 for x in range(B) if x != root)
    eps = Fraction(1, 1 << 52)

    def bound(d):
        return (2 * B + 2) * eps * d + (S + 1) * eps * sum_h

    pairs = [g for g in ex.seed_gaps if g[1] is not None] + [g for gaps in ex.round_gaps for g in gaps.values() if g[1] is not None]
    assert len(pairs) >= 2 + 2 * S
    margin = min(abs(a - b) - bound(a) - bound(b) for a, b in pairs)
    print("smallest gap less the two bounds", float(margin), "largest bound", float(max(bound(max(a, b)) for a, b in pairs)))
    assert margin > 0, "a bad input: the exact run does not decide the seeds or an assignment"
    got = host(parent, bl, m, S, k)
    ref = K.kmeans_ref(parent, bl, m, S, k)
    assert K.same(got, ref) and ref.seeds == ex.seeds
    assert got.info.tolist() == [k, S, ex.rounds, ex.converged] and got.assign.tolist() == [ex.assign[s] for s in range(S)]
    worst = max(abs(Fraction(float(got.dist[s])) - ex.dist[s]) - bound(ex.dist[s]) for s in range(S))
    print("largest error less its bound", float(worst))
    assert worst <= 0


def planted_case(B, S, k, seed):
    """a planted buffer on a random tree whose KR matrix (rk_kr_distances_host) separates the planted clusters: the smallest distance
    between two clusters is more than twice the largest inside one.  KR is the L1 norm of the profiles, so the mean of a cluster's
    members lies within the largest within-distance of each of them: farthest-first then seeds one sample a cluster and k-means finds
    the planted partition in round one and confirms it in round two."""
    parent, bl = R.random_tree(B, seed)
    m, _ = K.planted_buffer(B, S, k, seed + 1)
    D = ra.kr_distances_host(parent, bl, m, S)
    label = np.arange(S) % k
    same = label[:, None] == label[None, :]
    between, inside = D[~same].min(), D[same].max()
    print("smallest between", between, "largest within", inside)
    assert between > 2 * inside, "a bad input: the planted clusters are not separated"
    return parent, bl, m, label


def is_planted_partition(assign, label, k):
    """the labels compared up to the order of the seeds"""
    seen = {}
    for a, l in zip(assign.tolist(), label.tolist()):
        if seen.setdefault(a, l) != l:
            return False
    return len(seen) == k and len(set(seen.values())) == k


PLANTED = (60, 23, 4, 7)


def test_planted_partition():
    B, S, k, seed = PLANTED
    parent, bl, m, label = planted_case(B, S, k, seed)
    got = host(parent, bl, m, S, k)
    assert got.info.tolist() == [k, S, 2, 1] and is_planted_partition(got.assign, label, k)
    one = host(parent, bl, m, S, k, max_rounds=1)
    assert one.info.tolist() == [k, S, 1, 0] and is_planted_partition(one.assign, label, k)
    assert (one.assign == got.assign).all() and sorted(got.sizes.tolist()) == sorted(np.bincount(label).tolist())


def table_cases():
    """(names, k, assign, dist, sizes, within, info): a run of a few samples with names that hold tabs' neighbours, a run without any
    active sample, and one without samples with mass but k = 1"""
    B, S, k = 40, 6, 3
    parent, bl = R.random_tree(B, 2)
    r = host(parent, bl, R.special_buffer(B, S, 3), S, k)
    yield ["a", "b b", "c'1", "d(x)", "e,f", "g:h;[i]"], k, r.assign, r.dist, r.sizes, r.within, r.info
    tiny = np.array([1e-300, 0.1, 2.5])
    yield ["w", "x", "y z"], 2, np.array([1, K.NONE, 0], np.uint32), tiny, np.array([1, 1], np.uint32), np.array([2.5, 1e-300]), np.array([2, 2, 7, 0], np.uint32)
    yield ["p", "q"], 4, np.full(2, K.NONE, np.uint32), np.zeros(2), np.zeros(4, np.uint32), np.zeros(4), np.array([0, 0, 0, 1], np.uint32)
    yield ["p"], 1, np.full(1, K.NONE, np.uint32), np.zeros(1), np.zeros(1, np.uint32), np.zeros(1), np.array([1, 0, 0, 3], np.uint32)


def test_kmeans_table_text():
    cases = list(table_cases())
    tiny = "%.17g" % 1e-300
    assert hostio.kmeans_table(*cases[1]) == ("#kmeans\t3\t2\t2\t2\t7\t0\n#clusters\n0\t1\t2.5\n1\t1\t" + tiny + "\n#samples\nw\t1\t" + tiny + "\nx\t-\t0\n"
                                              "y z\t0\t2.5\n#samples_without_mass\t1\n")
    assert hostio.kmeans_table(*cases[2]) == ("#kmeans\t2\t4\t0\t0\t0\t1\n#clusters\n0\t0\t0\n1\t0\t0\n2\t0\t0\n3\t0\t0\n#samples\np\t-\t0\nq\t-\t0\n"
                                              "#samples_without_mass\t2\n")
    assert hostio.kmeans_table(*cases[3]) == "#kmeans\t1\t1\t1\t0\t0\t1\n#clusters\n0\t0\t0\n#samples\np\t-\t0\n#samples_without_mass\t1\n"
    lines = hostio.kmeans_table(*cases[0]).splitlines()
    names, k, assign, dist, sizes, within, info = cases[0]
    assert lines[0] == "#kmeans\t6\t3\t3\t5\t%d\t1" % info[2] and lines[1] == "#clusters" and lines[5] == "#samples" and lines[-1] == "#samples_without_mass\t1"
    assert lines[7] == "b b\t-\t0" and lines[8].split("\t")[:2] == ["c'1", str(assign[2])] and float(lines[8].split("\t")[2]) == dist[2]  # %.17g round-trips
    assert [int(l.split("\t")[1]) for l in lines[2:5]] == sizes.tolist() and [float(l.split("\t")[2]) for l in lines[2:5]] == within.tolist()


def test_kmeans_table_twins_are_byte_identical(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.skip("no C++ compiler (g++)")
    exe = str(tmp_path / "kmeans_table")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rappas_amd", "csrc"), os.path.join(ROOT, "tests", "kmeans_table.cpp"),
                    "-o", exe], check=True)
    for i, (names, k, assign, dist, sizes, within, info) in enumerate(table_cases()):
        d = tmp_path / str(i)
        d.mkdir()
        (d / "names.txt").write_bytes("".join(nm + "\n" for nm in names).encode())
        raw = b"".join(np.ascontiguousarray(a, dtype=dt).tobytes() for a, dt in ((assign, "<u4"), (sizes, "<u4"), (info, "<u4"), (dist, "<f8"), (within, "<f8")))
        (d / "run.bin").write_bytes(raw)
        got = subprocess.run([exe, str(d / "names.txt"), str(k), str(d / "run.bin")], capture_output=True, check=True, timeout=60).stdout
        assert got == hostio.kmeans_table(names, k, assign, dist, sizes, within, info).encode(), i


def test_bad_arguments():
    lib = _lib.load()
    B, S, k = 3, 4, 2
    p, b = np.array([-1, 0, 0], np.int32), np.array([0, 1, 1], np.float32)
    m = R.sample_buffer(B, S, 1)
    assign, dist = np.full(S, 7, np.uint32), np.full(S, 7.0)
    sizes, within, info = np.full(k, 7, np.uint32), np.full(k, 7.0), np.full(4, 7, np.uint32)

    def call(S=S, k=k, rounds=5, masses=m.ctypes.data, a=assign.ctypes.data, d=dist.ctypes.data, n=sizes.ctypes.data, w=within.ctypes.data, i=info.ctypes.data,
             parent=p.ctypes.data):
        return lib.rk_kmeans_host(B, parent, b.ctypes.data, S, masses, k, rounds, None, a, d, n, w, i, None, 1)

    big = np.zeros(8, np.uint64)
    for kw, text in ((dict(S=0), b"1..65535"), (dict(S=65536, masses=big.ctypes.data), b"1..65535"), (dict(k=0), b"1..64"), (dict(k=65), b"1..64"),
                     (dict(rounds=0), b"1..1024"), (dict(rounds=1025), b"1..1024"), (dict(masses=None), b"null"), (dict(a=None), b"null"), (dict(d=None), b"null"),
                     (dict(n=None), b"null"), (dict(w=None), b"null"), (dict(i=None), b"null"), (dict(parent=None), b"null")):
        assert call(**kw) == _lib.RK_ERR_INVALID and text in lib.rk_last_error(), kw
    assert (assign == 7).all() and (dist == 7).all() and (sizes == 7).all() and (within == 7).all() and (info == 7).all()  # nothing was written
    assert call() == _lib.RK_OK and info[1] == S  # the centroids are optional
