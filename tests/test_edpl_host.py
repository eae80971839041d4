"""The EDPL on the host (rk_edpl_host, rk_tree_distance_host) against its definition restated in tests/edpl_ref.py:
the golden file, bit parity with the restatement on stars, caterpillars and random trees, every thread count, all pairs of a tree
against the exact rational distance, the known cases, the refused arguments, and the two edpl_table writers.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, hostio
from rappas_amd._lib import rk_result

from tests import edpl_ref as E
from tests import kr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREES = list(E.trees((1, 2, 3, 300, 2049)))


def test_golden_file_comes_out_exactly_from_all_three():
    g = E.golden()
    K = g["keep_at_most"]
    t = E.Tree(g["parent"], g["branch_len"])
    assert t.D == g["D"] and t.pos == g["pos"]
    want = g["edpl"]
    assert E.same(E.edpl_ref(g["parent"], g["branch_len"], K, g["n_rows"], g["branch"], g["lwr"]), want)
    assert E.same(ra.edpl_host(g["parent"], g["branch_len"], K, g["n_rows"], g["branch"], g["lwr"]), want)
    a, b, d = (np.array([row[i] for row in g["distances"]]) for i in range(3))
    assert E.same(ra.tree_distance_host(g["parent"], g["branch_len"], a, b), d.astype(np.float64))
    assert [t.distance(int(x), int(y)) for x, y in zip(a, b)] == d.tolist()
    # read A from the distances: 2 * (w5 w1 d(5,1) + w5 w4 d(5,4) + w1 w4 d(1,4))
    assert 2.0 * (0.5 * 0.25 * 1.125 + 0.5 * 0.25 * 2.625 + 0.25 * 0.25 * 2.5) == want[0] == 1.25


@pytest.mark.parametrize("name,tree", TREES, ids=[n for n, _ in TREES])
def test_host_twins_are_edpl_ref_bit_for_bit(name, tree):
    parent, bl = tree
    B = len(parent)
    t = E.Tree(parent, bl)
    rng = np.random.default_rng(B)
    a, b = rng.integers(0, B, 400).astype(np.uint16), rng.integers(0, B, 400).astype(np.uint16)
    a[:8], b[:8] = t.root, rng.integers(0, B, 8)  # pairs with the root, and the root with itself
    a[8], b[8] = t.root, t.root
    got = ra.tree_distance_host(parent, bl, a, b)
    assert E.same(got, np.array([t.distance(int(x), int(y)) for x, y in zip(a, b)], np.float64)), name
    for K in (1, 2, 7, 16):
        n_rows, branch, lwr = E.result_set(B, K, 30, seed=7 * B + K)
        want = E.edpl_ref(parent, bl, K, n_rows, branch, lwr)
        assert E.same(ra.edpl_host(parent, bl, K, n_rows, branch, lwr), want), (name, K)
        if K == 1:
            assert (R.bits(want) == 0).all()  # one row at the most: +0.0


def test_every_thread_count_gives_the_same_bits():
    """a thread takes a range of reads once there are 4 096 a thread: 16 x 4 096 reads and one more bring all 16 out"""
    parent, bl = R.random_tree(300, 360)
    K, n = 7, 16 * 4096 + 1
    n_rows, branch, lwr = E.result_set(300, K, n, seed=5)
    one = ra.edpl_host(parent, bl, K, n_rows, branch, lwr, threads=1)
    assert E.same(one[:200], E.edpl_ref(parent, bl, K, n_rows[:200], branch[:200], lwr[:200]))
    assert E.same(one[-50:], E.edpl_ref(parent, bl, K, n_rows[-50:], branch[-50:], lwr[-50:]))
    for threads in list(range(2, 17)) + [0, 99]:
        assert E.same(ra.edpl_host(parent, bl, K, n_rows, branch, lwr, threads=threads), one), threads


def test_all_pairs_of_a_tree_against_the_exact_distance():
    """symmetric, zero on the diagonal, and within (depth + 4) * 2^-52 * max D of the rational distance: one rounding per add along
    the root path of either end, three in the final expression"""
    B = 300
    parent, bl = R.random_tree(B, 360)
    t = E.Tree(parent, bl)
    a, b = (v.reshape(-1).astype(np.uint16) for v in np.meshgrid(np.arange(B), np.arange(B), indexing="ij"))
    d = ra.tree_distance_host(parent, bl, a, b).reshape(B, B)
    assert (R.bits(d) == R.bits(d.T)).all() and (R.bits(np.diagonal(d)) == 0).all()
    D, pos = t.exact()
    bound = Fraction(max(t.depth) + 4) * Fraction(1, 2 ** 52) * max(D)
    worst = Fraction(0)
    for x in range(B):
        for y in range(x + 1, B):
            exact = t.distance_exact(x, y, D, pos)
            assert exact >= 0
            worst = max(worst, abs(Fraction(float(d[x, y])) - exact), abs(Fraction(t.distance(x, y)) - exact))  # the engine and the restatement
    print(f"largest error {float(worst):.3e}, bound {float(bound):.3e}")
    assert worst <= bound


def test_known_cases():
    parent, bl = R.random_tree(300, 360)
    K = 7
    # all weight on one branch: 0, however the rows split it
    n_rows = np.array([K, 1, 3], np.uint8)
    branch = np.full((3, K), 17, np.uint16)
    lwr = np.full((3, K), 1.0 / K)
    assert (R.bits(ra.edpl_host(parent, bl, K, n_rows, branch, lwr)) == 0).all()
    # two rows of weight 0.5 on a and b: 2 * 0.25 * d = 0.5 * d(a, b), exactly
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, 300, 64).astype(np.uint16), rng.integers(0, 300, 64).astype(np.uint16)
    branch = np.full((64, K), 0xFFFF, np.uint16)
    branch[:, 0], branch[:, 1] = a, b
    lwr = np.zeros((64, K))
    lwr[:, :2] = 0.5
    got = ra.edpl_host(parent, bl, K, np.full(64, 2, np.uint8), branch, lwr)
    assert E.same(got, 0.5 * ra.tree_distance_host(parent, bl, a, b))
    # weights are not renormalised: doubling every weight gives four times the value
    n_rows, branch, lwr = E.result_set(300, K, 50, seed=9, plant=False)
    assert E.same(ra.edpl_host(parent, bl, K, n_rows, branch, 2.0 * lwr), 4.0 * ra.edpl_host(parent, bl, K, n_rows, branch, lwr))
    # an ancestor pair is not the third line of the table with l = a: that would be off by 2 h[a]
    t = E.Tree(parent, bl)
    x = next(x for x in range(300) if t.depth[x] >= 2 and t.len[t.parent[x]] > 0)
    up = t.parent[x]
    d = ra.tree_distance_host(parent, bl, [up], [x])[0]
    assert d == t.pos[x] - t.pos[up] and d != (t.pos[up] - t.D[up]) + (t.pos[x] - t.D[up])


def test_refused_arguments_write_nothing():
    lib = _lib.load()
    B, K, n = 5, 3, 4
    parent, bl = np.array([-1, 0, 0, 1, 1], np.int32), np.ones(5, np.float32)
    n_rows, branch, lwr = E.result_set(B, K, n, seed=1)
    out = np.full(n, 7.0)
    P = lambda a: a.ctypes.data  # noqa: E731

    def edpl(parent_p=P(parent), bl_p=P(bl), B=B, K=K, n=n, rows=P(n_rows), br=P(branch), lw=P(lwr), o=P(out), res=True):
        r = rk_result(rows, br, None, lw, None)
        return lib.rk_edpl_host(B, parent_p, bl_p, K, n, C.byref(r) if res else None, o, 1)

    assert edpl() == _lib.RK_OK and not (out == 7.0).any()
    out[:] = 7.0
    for kw, text in ((dict(K=0), b"keep_at_most"), (dict(K=17), b"keep_at_most"), (dict(n=1 << 32), b"n_reads"), (dict(rows=None), b"null result"),
                     (dict(br=None), b"null result"), (dict(lw=None), b"null result"), (dict(res=False), b"null result"), (dict(o=None), b"null output"),
                     (dict(parent_p=None), b"null parent"), (dict(bl_p=None), b"null branch_len"), (dict(B=0), b"n_branches"), (dict(B=65536), b"n_branches")):
        assert edpl(**kw) == _lib.RK_ERR_INVALID and text in lib.rk_last_error(), kw
    for bad_parent in ([1, 2, 0, 0, 0], [-1, -1, 0, 0, 0]):
        assert edpl(parent_p=P(np.array(bad_parent, np.int32))) == _lib.RK_ERR_INVALID
    assert (out == 7.0).all()
    assert edpl(n=0, rows=None, br=None, lw=None, o=None) == _lib.RK_OK  # nothing to do, nothing touched

    a, b, d = np.array([0, 1, 4], np.uint16), np.array([3, 2, 5], np.uint16), np.full(3, 7.0)

    def dist(parent_p=P(parent), bl_p=P(bl), B=B, n=3, a_p=P(a), b_p=P(b), d_p=P(d)):
        return lib.rk_tree_distance_host(B, parent_p, bl_p, n, a_p, b_p, d_p)

    assert dist() == _lib.RK_ERR_INVALID and b"pair 2" in lib.rk_last_error()  # a branch >= B in the last pair: the first two are not written either
    for kw in (dict(a_p=None), dict(b_p=None), dict(d_p=None), dict(parent_p=None), dict(bl_p=None), dict(B=0)):
        assert dist(**kw) == _lib.RK_ERR_INVALID, kw
    assert (d == 7.0).all()
    assert dist(n=2) == _lib.RK_OK and d[2] == 7.0 and d[0] == 1.5 and d[1] == 1.0
    assert dist(n=0, a_p=None, b_p=None, d_p=None) == _lib.RK_OK
    with pytest.raises(ra.RkError):
        ra.edpl_host(parent, bl, 17, np.zeros(1, np.uint8), np.zeros((1, 17), np.uint16), np.zeros((1, 17)))
    assert lib.rk_edpl_lds_bytes(None) == 0 and b"null tree" in lib.rk_last_error()
    r = rk_result(P(n_rows), P(branch), None, P(lwr), None)
    assert lib.rk_edpl_device(None, K, n, C.byref(r), P(out), None) == _lib.RK_ERR_INVALID and b"null tree" in lib.rk_last_error()
    assert lib.rk_edpl_batch(None, None, K, n, C.byref(r), P(out)) == _lib.RK_ERR_INVALID and b"null handle" in lib.rk_last_error()


def table_case():
    records = [("s1|a first", "ACGT"), ("s1|b", "AC-GT"), ("s2|c", "TTTT"), ("s2|d x y", "GGGA"), ("s1|e", "TTTT")]
    unique, _ = hostio.dedup_reads(records)
    n_rows = np.array([2, 0, 7], np.uint8)  # ACGT placed, TTTT not, GGGA placed
    edpl = np.array([1 / 3, 99.0, 1e-300])
    return records, unique, n_rows, edpl


def test_edpl_table_text():
    records, unique, n_rows, edpl = table_case()
    assert len(unique) == 3
    text = hostio.edpl_table(records, unique, n_rows, edpl)
    assert text == "#edpl\t3\ns1|a first\t" + "%.17g" % (1 / 3) + "\ns1|b\t" + "%.17g" % (1 / 3) + "\ns2|d x y\t" + "%.17g" % 1e-300 + "\n"
    assert float(text.splitlines()[1].split("\t")[1]) == 1 / 3  # %.17g round-trips
    assert hostio.edpl_table(records, unique, np.zeros(3, np.uint8), edpl) == "#edpl\t0\n"


def test_edpl_table_twins_are_byte_identical(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.skip("no C++ compiler (g++)")
    exe = str(tmp_path / "edpl_table")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rappas_amd", "csrc"), os.path.join(ROOT, "tests", "edpl_table.cpp"),
                    "-o", exe], check=True)
    records, unique, n_rows, edpl = table_case()
    rng = np.random.default_rng(4)
    big = [(f"r{i} tail", "".join(rng.choice(list("ACGT"), 12))) for i in range(300)]
    big += [(f"dup{i}", big[i][1]) for i in range(0, 300, 7)]
    big_unique, _ = hostio.dedup_reads(big)
    vals = rng.random(len(big_unique)) * 10.0 ** rng.integers(-20, 3, len(big_unique))
    vals[:5] = [0.0, 1.25, 0.984375, 5e-324, 1.7976931348623157e308]
    for i, (recs, uniq, rows, v) in enumerate(((records, unique, n_rows, edpl), (big, big_unique, rng.integers(0, 3, len(big_unique)).astype(np.uint8), vals))):
        d = tmp_path / str(i)
        d.mkdir()
        index = {seq.replace("-", ""): u for u, (_, seq) in enumerate(uniq)}
        (d / "headers.txt").write_text("".join(h + "\n" for h, _ in recs))
        np.array([index[s.replace("-", "")] for _, s in recs], np.uint32).tofile(d / "uniq.bin")
        rows.tofile(d / "rows.bin")
        np.asarray(v, np.float64).tofile(d / "edpl.bin")
        got = subprocess.run([exe, str(d / "headers.txt"), str(d / "uniq.bin"), str(d / "rows.bin"), str(d / "edpl.bin")], check=True, capture_output=True).stdout
        assert got == hostio.edpl_table(recs, uniq, rows, v).encode(), i
