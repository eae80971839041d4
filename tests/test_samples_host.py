"""The sample-level host calls (rk_tree_validate, rk_clade_masses_host, rk_kr_distances_host) against their definition
restated in tests/kr_ref.py: known answers, bit parity with the numpy restatement, accuracy against exact rationals, the clade column
of the per-edge table, the refused trees, and the two kr_table writers.  No GPU."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, hostio
from rappas_amd.placement import tree_validate

from tests import kr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 1 << 30


def known_tree():
    """root 0; 1 and 2 under 0 with lengths 1 and 3; 3 and 4 under 2 with lengths 2 and 4.  A all on 1, B all on 3, C half on 1, half on 4"""
    parent = np.array([-1, 0, 0, 2, 2], np.int32)
    bl = np.array([0, 1, 3, 2, 4], np.float32)
    W = 2 * 5 + 4
    m = np.zeros(3 * W + 1, np.uint64)
    m[0 * W + 1] = Q
    m[1 * W + 3] = Q
    m[2 * W + 1] = Q // 2
    m[2 * W + 4] = Q // 2
    return parent, bl, m


def test_known_answer_exact():
    """D(A,B) = 4.5 and D(A,C) = 2.75.  D(B,C) worked from the definition: edge 1 gives 0.5 * 0.5, edge 2 gives 1.5 * 0.5 twice,
    edge 3 gives 1 * 1, edge 4 gives 2 * 0.5: 3.75 (the transport reading agrees: half of C travels 4.5, half travels 3; 2.75 is
    D(A,C), not D(B,C)).  Every value is exact in binary64, so equality is asked for, against the numbers and the rationals."""
    parent, bl, m = known_tree()
    D = ra.kr_distances_host(parent, bl, m, 3)
    assert D[0, 1] == 4.5 and D[0, 2] == 2.75 and D[1, 2] == 3.75
    assert D[1, 0] == 4.5 and D[2, 0] == 2.75 and D[2, 1] == 3.75
    assert (R.bits(np.diagonal(D)) == 0).all()  # +0.0
    E = R.kr_exact(parent, bl, m, 3)
    assert E[0][1] == Fraction(9, 2) and E[0][2] == Fraction(11, 4) and E[1][2] == Fraction(15, 4)
    for s in range(3):
        for t in range(3):
            assert Fraction(float(D[s, t])) == E[s][t]
    assert (R.bits(D) == R.bits(R.kr_ref(parent, bl, m, 3))).all()


def trees():
    yield "random-1", R.random_tree(1, 1)
    yield "random-2", R.random_tree(2, 2)
    yield "random-999", R.random_tree(999, 3)
    yield "random-2047", R.random_tree(2047, 4)
    yield "random-2048", R.random_tree(2048, 5)
    yield "random-2049", R.random_tree(2049, 6)
    yield "random-4097", R.random_tree(4097, 7)
    yield "caterpillar-2049", R.caterpillar(2049)
    yield "star-2049", R.star(2049)


@pytest.mark.parametrize("name,tree", list(trees()), ids=[n for n, _ in trees()])
def test_host_twin_is_kr_ref_bit_for_bit(name, tree):
    parent, bl = tree
    B = len(parent)
    for S in (1, 2, 3):
        m = R.sample_buffer(B, S, seed=B + S)
        want = R.kr_ref(parent, bl, m, S)
        got = ra.kr_distances_host(parent, bl, m, S)
        assert (R.bits(got) == R.bits(want)).all(), (name, S)
        assert (ra.clade_masses_host(parent, m, S) == R.clade_ref(parent, m, S)).all()


def test_many_samples_empty_identical_and_huge_masses_every_thread_count():
    """S = 65 on a tree that spans two chunks: an empty sample (NaN row and column, NaN diagonal), two identical samples (+0.0),
    2^62 on one branch; the same bits from 1..16 threads"""
    parent, bl = R.random_tree(2049, 11)
    S = 65
    m = R.special_buffer(2049, S, 12)
    want = R.kr_ref(parent, bl, m, S)
    R.check_special(want)
    for threads in range(1, 17):
        got = ra.kr_distances_host(parent, bl, m, S, threads=threads)
        assert (R.bits(got) == R.bits(want)).all(), threads
    assert (R.bits(ra.kr_distances_host(parent, bl, m, S)) == R.bits(want)).all()
    assert (ra.clade_masses_host(parent, m, S) == R.clade_ref(parent, m, S)).all()


@pytest.mark.parametrize("B", [1, 2, 5, 33, 64])
def test_accuracy_against_exact_rationals(B):
    """|D - exact| <= (2B + 2) * 2^-52 * exact: 2B non-negative terms of two roundings each (a difference of two rounded quotients
    needs the margin the factor 2 in 2^-52 = 2 * 2^-53 leaves), at most 2B - 1 adds at unit roundoff 2^-53 -- derived, not measured"""
    for seed, (parent, bl) in enumerate([R.random_tree(B, 20 + B), R.caterpillar(B, 1), R.star(B, 2)]):
        S = 4
        m = R.sample_buffer(B, S, 30 + seed, fill=0.6)
        D = ra.kr_distances_host(parent, bl, m, S)
        E = R.kr_exact(parent, bl, m, S)
        for s in range(S):
            for t in range(S):
                assert abs(Fraction(float(D[s, t])) - E[s][t]) <= (2 * B + 2) * Fraction(1, 1 << 52) * E[s][t], (B, seed, s, t)


def test_clade_masses_are_the_clade_column_of_the_table():
    tree = hostio.parse_newick("((A:1,B:2)X:0.5,((C:1,D:3)Y:0.25,E:2)Z:1,F:0.125)R;")
    B = len(tree.nodes)
    parent = np.array([n.parent.id if n.parent is not None else -1 for n in tree.nodes], np.int32)
    m = R.sample_buffer(B, 1, 5, fill=0.8)[:2 * B + 4]  # an ordinary mass buffer: S = 1, no last word
    clade = ra.clade_masses_host(parent, m, 1)
    lines = hostio.masses_table(tree, m).splitlines()[1:1 + B]
    assert [int(line.split("\t")[7]) for line in lines] == [int(x) for x in clade[0]]
    assert (clade == R.clade_ref(parent, m, 1)).all()
    m3 = R.sample_buffer(B, 3, 6)
    assert (ra.clade_masses_host(parent, m3, 3) == R.clade_ref(parent, m3, 3)).all()
    assert (ra.clade_masses_host(parent, m3[:-1], 3) == R.clade_ref(parent, m3, 3)).all()  # the last word is never read


BAD_TREES = [
    ("no root", [1, 2, 0], [1, 1, 1], "no root"),
    ("two roots", [-1, -1, 0], [1, 1, 1], "one root"),
    ("parent beyond B", [-1, 3, 0], [1, 1, 1], "outside"),
    ("parent below -1", [-1, -2, 0], [1, 1, 1], "outside"),
    ("own parent", [-1, 1, 0], [1, 1, 1], "itself"),
    ("cycle", [-1, 2, 1, 0], [1, 1, 1, 1], "does not reach the root"),
    ("negative length", [-1, 0, 0], [0, -1, 1], "branch_len[1]"),
    ("NaN length", [-1, 0, 0], [0, 1, float("nan")], "branch_len[2]"),
    ("infinite length", [-1, 0, 0], [0, float("inf"), 1], "branch_len[1]"),
]


@pytest.mark.parametrize("what,parent,bl,text", BAD_TREES, ids=[b[0] for b in BAD_TREES])
def test_bad_trees_are_refused_with_a_message(what, parent, bl, text):
    with pytest.raises(ra.RkError) as e:
        tree_validate(parent, bl)
    assert e.value.code == _lib.RK_ERR_INVALID and text in str(e.value)
    S, B = 2, len(parent)
    out = np.full((S, S), 7.0)
    m = R.sample_buffer(B, S, 1)
    with pytest.raises(ra.RkError) as e:
        lib = _lib.load()
        p, b = np.array(parent, np.int32), np.array(bl, np.float32)
        _lib.check(lib.rk_kr_distances_host(B, p.ctypes.data, b.ctypes.data, S, m.ctypes.data, out.ctypes.data, 1))
    assert e.value.code == _lib.RK_ERR_INVALID and (out == 7.0).all()  # nothing is written


def test_bad_arguments_of_the_tree_calls():
    lib = _lib.load()
    p, b = np.array([-1, 0], np.int32), np.array([0, 1], np.float32)
    assert lib.rk_tree_validate(2, p.ctypes.data, b.ctypes.data) == _lib.RK_OK
    assert lib.rk_tree_validate(2, None, b.ctypes.data) == _lib.RK_ERR_INVALID and b"null" in lib.rk_last_error()
    assert lib.rk_tree_validate(2, p.ctypes.data, None) == _lib.RK_ERR_INVALID and b"null" in lib.rk_last_error()
    assert lib.rk_tree_validate(0, p.ctypes.data, b.ctypes.data) == _lib.RK_ERR_INVALID and b"1..65535" in lib.rk_last_error()
    assert lib.rk_tree_validate(65536, p.ctypes.data, b.ctypes.data) == _lib.RK_ERR_INVALID
    tree_validate([-1, 0, 0], [float("nan"), 1, 1])  # the root's entry is ignored
    lib.rk_tree_destroy(None)  # a no-op
    assert lib.rk_kr_work_bytes(None, 3) == 0 and b"null tree" in lib.rk_last_error()


def test_kr_table_twins_are_byte_identical(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.skip("no C++ compiler (g++)")
    exe = str(tmp_path / "kr_table")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rappas_amd", "csrc"), os.path.join(ROOT, "tests", "kr_table.cpp"),
                    "-o", exe], check=True)
    parent, bl = R.random_tree(40, 3)
    m = R.special_buffer(40, 6, 4)
    D = ra.kr_distances_host(parent, bl, m, 6)
    D[0, 5] = D[5, 0] = 1e-300
    D[2, 4] = -np.nan  # a NaN prints as nan whatever its sign
    names = ["a", "b b", "c_1", "d", "e", "f"]
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names))
    D.tofile(str(tmp_path / "D.bin"))
    got = subprocess.run([exe, str(tmp_path / "names.txt"), str(tmp_path / "D.bin")], capture_output=True, check=True).stdout
    want = hostio.kr_table(names, D)
    assert got == want.encode()
    lines = want.splitlines()
    assert lines[0] == "#kr\t6" and lines[-1] == "#samples_without_mass\t1" and len(lines) == 8
    assert lines[1].split("\t")[0] == "a" and float(lines[1].split("\t")[3]) == D[0, 2]  # %.17g round-trips
