"""The squash clustering on the host (rk_squash_host) against its definition restated in tests/squash_ref.py: bit
parity with the numpy restatement, the special samples, every thread count, a known answer, the order and the accuracy against exact
rationals, the refused arguments, and the two squash_table writers.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, hostio

from tests import kr_ref as R
from tests import squash_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def trees():
    for B in (1, 2, 300, 2049):
        yield f"star-{B}", R.star(B, B)
        yield f"caterpillar-{B}", R.caterpillar(B, B)
        yield f"random-{B}", R.random_tree(B, 60 + B)


def check_rows(merges, n, S):
    """what the definition promises of any run: fillers behind n_merges, a < b, sizes that add up"""
    assert len(merges) == S - 1 and 0 <= n <= S - 1
    for k in range(n, S - 1):
        assert tuple(merges[k])[:4] == (Q.NONE, Q.NONE, 0, 0) and R.bits(merges[k]["distance"]) == 0
    size, gone = {}, set()
    for k in range(n):
        a, b = int(merges[k]["a"]), int(merges[k]["b"])
        assert a < b < S and merges[k]["reserved"] == 0 and a not in gone and b not in gone
        size[a] = size.get(a, 1) + size.get(b, 1)
        gone.add(b)
        assert merges[k]["size"] == size[a]
    if n:
        assert merges[n - 1]["size"] == n + 1


@pytest.mark.parametrize("name,tree", list(trees()), ids=[n for n, _ in trees()])
def test_host_twin_is_squash_ref_bit_for_bit(name, tree):
    parent, bl = tree
    B = len(parent)
    for S in (2, 3, 6):
        m = R.sample_buffer(B, S, seed=3 * B + S)
        want, n_want = Q.squash_ref(parent, bl, m, S)
        got, n = ra.squash_host(parent, bl, m, S)
        assert n == n_want == S - 1, (name, S)
        assert Q.same_rows(got, want), (name, S, got, want)
        check_rows(got, n, S)


@pytest.mark.parametrize("B,S", [(300, 6), (2049, 5), (5, 7)])
def test_special_buffer_tie_rule_empty_sample_and_fillers(B, S):
    """samples 2 and 3 are identical: D = +0.0 is the smallest, and the first of the smallest; sample 1 is empty and is in no row"""
    parent, bl = R.random_tree(B, 70 + B)
    m = R.special_buffer(B, S, 71)
    got, n = ra.squash_host(parent, bl, m, S)
    want, n_want = Q.squash_ref(parent, bl, m, S)
    assert n == n_want == S - 2 and Q.same_rows(got, want)
    assert tuple(got[0])[:4] == (2, 3, 2, 0) and R.bits(got[0]["distance"]) == 0
    assert 1 not in set(got["a"][:n]) | set(got["b"][:n])
    check_rows(got, n, S)


def test_every_sample_empty_and_one_sample_with_mass():
    B, S = 40, 5
    parent, bl = R.random_tree(B, 5)
    m = np.zeros(S * (2 * B + 4) + 1, np.uint64)
    got, n = ra.squash_host(parent, bl, m, S)
    assert n == 0
    check_rows(got, 0, S)
    m[3 * (2 * B + 4) + 7] = 99
    got, n = ra.squash_host(parent, bl, m, S)
    assert n == 0
    check_rows(got, 0, S)
    m[0 * (2 * B + 4) + 2] = 5
    got, n = ra.squash_host(parent, bl, m, S)
    assert n == 1 and tuple(got[0])[:4] == (0, 3, 2, 0) and got[0]["distance"] > 0
    check_rows(got, 1, S)


def test_the_same_bits_from_every_thread_count():
    B, S = 2049, 20
    parent, bl = R.random_tree(B, 81)
    m = R.special_buffer(B, S, 82)
    want, n_want = ra.squash_host(parent, bl, m, S, threads=1)
    assert n_want == S - 2
    for threads in list(range(2, 17)) + [0]:
        got, n = ra.squash_host(parent, bl, m, S, threads=threads)
        assert n == n_want and Q.same_rows(got, want), threads


def test_known_answer_by_hand():
    """The five-node tree of test_samples_host.test_known_answer_exact: A all on 1, B all on 3, C half on 1 and half on 4, with
    D(A,B) = 4.5, D(A,C) = 2.75, D(B,C) = 3.75.  A and C merge first, at 2.75.  The cluster holds 0.75 on 1 and 0.25 on 4; against B
    edge 1 gives 0.5 * 0.75, edge 2 gives 1.5 * 0.75 twice, edge 3 gives 1 * 1, edge 4 gives 2 * 0.25: 4.125 (the transport reading
    agrees: 0.75 travels 4.5, 0.25 travels 3).  Every value is exact in binary64."""
    parent = np.array([-1, 0, 0, 2, 2], np.int32)
    bl = np.array([0, 1, 3, 2, 4], np.float32)
    W = 14
    m = np.zeros(3 * W + 1, np.uint64)
    m[0 * W + 1] = 1 << 30
    m[1 * W + 3] = 1 << 30
    m[2 * W + 1] = 1 << 29
    m[2 * W + 4] = 1 << 29
    got, n = ra.squash_host(parent, bl, m, 3)
    assert n == 2
    assert tuple(got[0]) == (0, 2, 2, 0, 2.75)
    assert tuple(got[1]) == (0, 1, 3, 0, 4.125)
    rows = Q.squash_exact(parent, bl, m, 3)
    assert [r[:4] for r in rows] == [(0, 2, 2, Fraction(11, 4)), (0, 1, 3, Fraction(33, 8))]


@pytest.mark.parametrize("B,S,i", [(40, 8, 1), (120, 12, 3), (300, 10, 4)])
def test_order_and_accuracy_against_the_exact_run(B, S, i):
    """The sequence (a, b, size) equals the exact run's, and every distance lies within
        (2B + 2) * 2^-52 * exact + 8 * S * 2^-52 * sum(h)
    of the exact one: the bound of the KR pair sum (test_samples_host.test_accuracy_against_exact_rationals) plus four roundings per
    profile entry per merge level (two products, a sum, a quotient: each at most 2^-53 relative on entries <= 1, so 2^-51 per level
    on each of the two profiles of a term, weighted by h), at most S - 1 levels.  First the exact run's gaps must decide the order: at
    every step the best and the second-best exact distance differ by more than the two bounds together."""
    parent, bl = R.random_tree(B, 100 + i)
    m = R.sample_buffer(B, S, 200 + i)
    rows = Q.squash_exact(parent, bl, m, S)
    root, _ = R.preorder(parent)
    sum_h = sum(Fraction(float(np.float32(bl[x]))) / 2 for x in range(B) if x != root)
    eps = Fraction(1, 1 << 52)

    def bound(d):
        return (2 * B + 2) * eps * d + 8 * S * eps * sum_h

    gaps = [(second - d) / second for _, _, _, d, second in rows if second is not None]
    need = [(bound(d) + bound(second)) / second for _, _, _, d, second in rows if second is not None]
    print("smallest relative gap", float(min(gaps)), "largest relative bound", float(max(need)))
    assert all(g > n for g, n in zip(gaps, need)), "a bad input: the exact run does not decide the order"
    got, n = ra.squash_host(parent, bl, m, S)
    assert n == len(rows) == S - 1
    assert [(int(r["a"]), int(r["b"]), int(r["size"])) for r in got] == [r[:3] for r in rows]
    worst = max(abs(Fraction(float(g["distance"])) - r[3]) / r[3] for g, r in zip(got, rows))
    print("worst relative error", float(worst))
    for g, r in zip(got, rows):
        assert abs(Fraction(float(g["distance"])) - r[3]) <= bound(r[3]), (g, float(r[3]))


def test_bad_arguments():
    lib = _lib.load()
    B = 3
    p, b = np.array([-1, 0, 0], np.int32), np.array([0, 1, 1], np.float32)
    m = R.sample_buffer(B, 4, 1)
    rows = np.full(3, 7, Q.SQUASH_MERGE)
    n = C.c_uint32(77)

    def call(B=B, parent=p.ctypes.data, lens=b.ctypes.data, S=4, masses=m.ctypes.data, out=rows.ctypes.data, count=C.byref(n)):
        return lib.rk_squash_host(B, parent, lens, S, masses, out, count, 1)

    assert call() == _lib.RK_OK and n.value == 3
    rows[:] = 7
    n.value = 77
    big = np.zeros(4097 * (2 * B + 4) + 1, np.uint64)
    for kw, text in ((dict(S=1), b"2..4096"), (dict(S=0), b"2..4096"), (dict(S=4097, masses=big.ctypes.data), b"2..4096"), (dict(parent=None), b"null"),
                     (dict(lens=None), b"null"), (dict(masses=None), b"null mass buffer"), (dict(out=None), b"null output"), (dict(count=None), b"null output"),
                     (dict(B=0), b"1..65535")):
        assert call(**kw) == _lib.RK_ERR_INVALID and text in lib.rk_last_error(), kw
    for parent, lens in (([1, 2, 0], [1, 1, 1]), ([-1, -1, 0], [1, 1, 1]), ([-1, 2, 1], [1, 1, 1]), ([-1, 0, 0], [0, -1, 1]), ([-1, 0, 0], [0, 1, float("nan")])):
        pp, bb = np.array(parent, np.int32), np.array(lens, np.float32)
        assert call(parent=pp.ctypes.data, lens=bb.ctypes.data) == _lib.RK_ERR_INVALID
    assert n.value == 77 and (rows["a"] == 7).all() and (rows["distance"] == 7).all()  # nothing is written
    assert lib.rk_squash_work_bytes(None, 3) == 0 and b"null tree" in lib.rk_last_error()
    with pytest.raises(ra.RkError):
        ra.squash_host(p, b, R.sample_buffer(B, 1, 1), 1)


def table_cases():
    """(names, merges, n_merges, with_mass): a real run with an empty sample and names that need quoting; a made-up run with a negative
    edge; one sample with mass; none"""
    parent, bl = R.random_tree(40, 3)
    m = R.special_buffer(40, 6, 4)
    merges, n = ra.squash_host(parent, bl, m, 6)
    yield ["a", "b b", "c'1", "d(x)", "e,f", "g:h;[i]"], merges, n, [True, False, True, True, True, True]
    inv = np.zeros(3, Q.SQUASH_MERGE)
    inv[0] = (1, 2, 2, 0, 3.0)
    inv[1] = (0, 1, 3, 0, 2.5)   # below the first merge: the edge above (1, 2) is negative
    inv[2] = (0, 3, 4, 0, 1e-300)
    yield ["w", "x", "y\tz", "it's"], inv, 3, [True] * 4
    none = np.zeros(2, Q.SQUASH_MERGE)
    none["a"] = none["b"] = Q.NONE
    yield ["p", "q r", "s"], none, 0, [False, True, False]
    yield ["p", "q", "s"], none, 0, [False, False, False]


def test_squash_table_text():
    cases = list(table_cases())
    text = hostio.squash_table(*cases[1])
    tiny, half = "%.17g" % 1e-300, "%.17g" % (1e-300 / 2)
    assert text == ("#squash\t4\t3\n0\t1\t2\t3\t2\n1\t0\t1\t2.5\t3\n2\t0\t3\t" + tiny + "\t4\n"
                    "#newick\t((w:1.25,(x:1.5,'y\tz':1.5):-0.25):-1.25,'it''s':" + half + ");\n#inversions\t2\n#samples_without_mass\t0\n")
    assert hostio.squash_table(*cases[2]) == "#squash\t3\t0\n#newick\t'q r';\n#inversions\t0\n#samples_without_mass\t2\n"
    assert hostio.squash_table(*cases[3]) == "#squash\t3\t0\n#newick\t;\n#inversions\t0\n#samples_without_mass\t3\n"
    lines = hostio.squash_table(*cases[0]).splitlines()
    assert lines[0] == "#squash\t6\t4" and lines[1].split("\t") == ["0", "2", "3", "0", "2"] and lines[-1] == "#samples_without_mass\t1"
    assert lines[5].startswith("#newick\t(") and "'c''1'" in lines[5] and "'d(x)'" in lines[5] and "'e,f'" in lines[5] and "'g:h;[i]'" in lines[5]
    assert "b b" not in lines[5]
    names, merges, n, with_mass = cases[0]
    assert hostio.squash_table(names, merges, n) == hostio.squash_table(names, merges, n, with_mass)  # the merges name the samples with mass
    assert float(lines[2].split("\t")[3]) == merges[1]["distance"]  # %.17g round-trips


def test_squash_table_twins_are_byte_identical(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.skip("no C++ compiler (g++)")
    exe = str(tmp_path / "squash_table")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rappas_amd", "csrc"), os.path.join(ROOT, "tests", "squash_table.cpp"),
                    "-o", exe], check=True)
    for i, (names, merges, n, with_mass) in enumerate(table_cases()):
        d = tmp_path / str(i)
        d.mkdir()
        (d / "names.txt").write_bytes("".join(nm + "\n" for nm in names).encode())
        np.ascontiguousarray(merges).tofile(str(d / "merges.bin"))
        (d / "mass.txt").write_text("".join("1\n" if f else "0\n" for f in with_mass))
        got = subprocess.run([exe, str(d / "names.txt"), str(d / "merges.bin"), str(n), str(d / "mass.txt")], capture_output=True, check=True, timeout=60).stdout
        assert got == hostio.squash_table(names, merges, n, with_mass).encode(), i
