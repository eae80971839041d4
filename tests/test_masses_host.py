"""CPU: the edge masses on the host -- rk_masses_accumulate_host against the numpy restatement of the definition
(tests/masses_ref.py) on hand-made result sets, for equality (the sums are integers), its error paths, and the table writers
(`rk_place --masses-table` against hostio.masses_table, byte for byte).  No GPU, no handle."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, build, hostio
from tests import masses_ref as MR

POISON = np.uint64(0xA5A5A5A5DEADBEEF)


def host(B, s, weights=None, masses=None, threads=0):
    return ra.accumulate_masses_host(B, s, weights=weights, masses=masses, threads=threads)


def test_the_reference_rounds_as_the_definition_says():
    assert np.array_equal(MR.q30(MR.SPECIAL_LWR), MR.SPECIAL_Q30)
    assert ra.masses_words(999) == 2002 and ra.masses_words(65535) == 131074 and ra.masses_words(1) == 6
    assert ra.masses_words(0) == 0 and ra.masses_words(65536) == 0


@pytest.mark.parametrize("K", [1, 7, 16])
@pytest.mark.parametrize("B", [1, 999, 65535])
def test_host_call_equals_the_reference(B, K):
    for n in (0, 1, 63, 65, 10007):
        s = MR.make_set(B, K, n, seed=n)
        kinds = (None, "zero", "one", "max", "mixed") if n <= 65 else (None, "mixed")
        for kind in kinds:
            w = MR.make_weights(n, kind, seed=K)
            want = MR.masses_ref(B, s.n_rows, s.branch, s.lwr, w)
            got = host(B, s, w)
            assert got.dtype == np.uint64 and got.shape == (2 * B + 4,)
            assert np.array_equal(got, want), (n, kind, np.flatnonzero(got != want)[:8])
        if n >= 63:  # the planted rows are there: branch ids >= B were met and counted, B - 1 was hit
            assert want[2 * B + 3] > 0 and want[B + B - 1] > 0


@pytest.mark.parametrize("B", [999, 20001])
def test_every_row_on_one_branch(B):
    K, n = 16, 10007
    s = MR.make_set(B, K, n, shape="one_branch")
    got = host(B, s)
    want = np.zeros(2 * B + 4, np.uint64)
    want[7], want[B + 7] = n * K * 2 ** 29, n
    want[2 * B:] = [n, n, n * K, 0]
    assert np.array_equal(got, want) and np.array_equal(MR.masses_ref(B, s.n_rows, s.branch, s.lwr), want)


def test_rows_with_a_branch_beyond_the_tree_move_nothing_but_their_counter():
    B, K = 999, 7
    s = MR.make_set(B, K, 200, seed=5)
    s.n_rows[:] = K
    s.branch[:] = (np.arange(200)[:, None] * 3 + np.arange(K)[None, :]) % B
    base = host(B, s)
    assert base[2 * B + 3] == 0
    t = MR.SimpleNamespace(n_rows=s.n_rows.copy(), branch=s.branch.copy(), lwr=s.lwr.copy())
    t.branch[10, 0] = B        # row 0: the read adds nothing to best
    t.branch[20, 3] = 0xFFFF   # a later row
    got = host(B, t)
    want = MR.masses_ref(B, t.n_rows, t.branch, t.lwr)
    assert np.array_equal(got, want)
    # against the set without them: the two rows are gone from their bins, from best and from the row count -- nothing else moved
    moved = base.copy()
    q = MR.q30(s.lwr)
    moved[s.branch[10, 0]] -= q[10, 0]
    moved[B + int(s.branch[10, 0])] -= np.uint64(1)
    moved[s.branch[20, 3]] -= q[20, 3]
    moved[2 * B + 2] -= np.uint64(2)
    moved[2 * B + 3] = 2
    assert np.array_equal(got, moved)


def test_n_rows_zero_hides_garbage_and_n_rows_beyond_K_is_clipped():
    B, K = 50, 4
    s = MR.SimpleNamespace(n_rows=np.array([0, 200, 2], np.uint8), branch=np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 0xFFFF, 11]], np.uint16),
                           lwr=np.array([[np.nan, 1e9, 0.5, 0.5], [0.5, 0.25, 0.125, 0.0625], [1.0, 0.5, 0.5, 0.5]]))
    got = host(B, s, np.array([3, 2, 5], np.uint32))
    want = np.zeros(2 * B + 4, np.uint64)
    for x, l in zip((5, 6, 7, 8), (0.5, 0.25, 0.125, 0.0625)):
        want[x] = int(2 * l * 2 ** 30)
    want[9], want[10] = 5 * 2 ** 30, 5 * 2 ** 29
    want[B + 5], want[B + 9] = 2, 5
    want[2 * B:] = [10, 7, 2 * 4 + 5 * 2, 0]
    assert np.array_equal(got, want)


def test_two_calls_into_one_buffer_equal_one_call_over_the_concatenation():
    B, K = 999, 7
    a, b = MR.make_set(B, K, 700, seed=1), MR.make_set(B, K, 333, seed=2)
    wa, wb = MR.make_weights(700, "mixed", 1), MR.make_weights(333, "mixed", 2)
    m = host(B, a, wa)
    m2 = host(B, b, wb, masses=m)
    assert m2 is m
    both = MR.concat(a, b)
    w = np.concatenate([wa, wb])
    assert np.array_equal(m, host(B, both, w)) and np.array_equal(m, MR.masses_ref(B, both.n_rows, both.branch, both.lwr, w))
    # the buffer is added to, whatever it holds
    start = np.arange(2 * B + 4, dtype=np.uint64) * np.uint64(3)
    assert np.array_equal(host(B, a, wa, masses=start.copy()), MR.masses_ref(B, a.n_rows, a.branch, a.lwr, wa, masses=start))


@pytest.mark.parametrize("B", [999, 65535])
def test_one_and_sixteen_threads_give_the_same_words(B):
    K, n = 7, 100003
    s = MR.make_set(B, K, n, seed=9)
    w = MR.make_weights(n, "mixed", 9)
    one = host(B, s, w, threads=1)
    assert np.array_equal(one, host(B, s, w, threads=16)) and np.array_equal(one, host(B, s, w, threads=0)) and np.array_equal(one, host(B, s, w, threads=3))
    assert np.array_equal(one, MR.masses_ref(B, s.n_rows, s.branch, s.lwr, w))


def test_errors_leave_a_poisoned_buffer_untouched():
    lib = _lib.load()
    B, K, n = 999, 7, 100
    s = MR.make_set(B, K, n, seed=4)
    m = np.full(2 * B + 4, POISON, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = dict(n_rows=p(s.n_rows), branch=p(s.branch), lwr=p(s.lwr))

    def call(B=B, K=K, n=n, masses=m, **kw):
        f = dict(good, **kw)
        res = _lib.rk_result(f["n_rows"], f["branch"], None, f["lwr"], None)
        return lib.rk_masses_accumulate_host(B, K, n, C.byref(res), None, None if masses is None else p(masses), 0)

    for kw in (dict(n_rows=None), dict(branch=None), dict(lwr=None), dict(masses=None), dict(K=0), dict(K=17), dict(n=2 ** 32), dict(n=2 ** 40),
               dict(B=0), dict(B=65536)):
        assert call(**kw) == _lib.RK_ERR_INVALID, kw
        assert lib.rk_last_error() != b"", kw
        assert (m == POISON).all(), kw
    assert lib.rk_masses_accumulate_host(B, K, n, None, None, p(m), 0) == _lib.RK_ERR_INVALID and (m == POISON).all()
    # no reads: fine, nothing is touched (not even looked at)
    assert lib.rk_masses_accumulate_host(B, K, 0, None, None, None, 0) == _lib.RK_OK
    assert call(n=0) == _lib.RK_OK and (m == POISON).all()
    # score and flags are not read: the good call passes with both NULL
    m[:] = 0
    assert call() == _lib.RK_OK and np.array_equal(m, MR.masses_ref(B, s.n_rows, s.branch, s.lwr))


# ---- the table ----
NEWICK = "((A:0.1,B:0.2,C:0.3)inner1:0.05,(D:0.1,(E:0.2,F:0.1):0.3,G:0.2,H:0.01)poly:0.1,I:0.4,(J:1,K:2)jk:0.5);"


def table_case():
    tree = hostio.parse_newick(NEWICK)
    B = len(tree.nodes)
    rng = np.random.default_rng(12)
    m = rng.integers(0, 2 ** 40, 2 * B + 4).astype(np.uint64)
    m[1] = 2 ** 53 + 1             # beyond what a double holds exactly
    m[3] = 2 ** 62 + 12345
    m[5] = 0
    m[B - 1] = 2 ** 63 + 2 ** 10 + 1
    m[B + 2] = 2 ** 54 + 3
    m[2 * B] = 2 ** 64 - 1
    return tree, B, m


def test_both_table_writers_agree_byte_for_byte(tmp_path):
    exe = build.build_host_tools()
    tree, B, m = table_case()
    assert any(len(n.children) > 2 for n in tree.nodes) and any(n.children and not n.label for n in tree.nodes)
    (tmp_path / "t.nwk").write_text(NEWICK + "\n")
    m.astype("<u8").tofile(tmp_path / "m.bin")
    r = subprocess.run([exe, "--masses-table", str(tmp_path / "t.nwk"), str(tmp_path / "m.bin"), str(tmp_path / "out.tsv")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    text = hostio.masses_table(tree, m)
    assert (tmp_path / "out.tsv").read_bytes() == text.encode()
    lines = text.split("\n")
    assert lines[0] == "node_id\tedge_num\tlabel\tbest_reads\tmass_q30\tmass\tclade_best_reads\tclade_mass_q30\tclade_mass"
    assert len(lines) == B + 3 and lines[-1] == "" and lines[-2] == "#total\t" + "\t".join(str(int(x)) for x in m[2 * B:])
    row1 = lines[2].split("\t")
    assert row1[0] == "1" and row1[4] == str(2 ** 53 + 1) and row1[5] == "%.9f" % (float(2 ** 53 + 1) / 2 ** 30)
    assert lines[1].split("\t")[1] == "-1"  # the root has no edge
    # a buffer of the wrong size is refused by both
    m[:-1].astype("<u8").tofile(tmp_path / "short.bin")
    r = subprocess.run([exe, "--masses-table", str(tmp_path / "t.nwk"), str(tmp_path / "short.bin"), str(tmp_path / "o2.tsv")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "masses_table" in r.stderr
    with pytest.raises(ValueError):
        hostio.masses_table(tree, m[:-1])


def test_clade_columns_equal_a_brute_force_subtree_sum():
    tree, B, m = table_case()
    rows = [ln.split("\t") for ln in hostio.masses_table(tree, m).split("\n")[1:B + 1]]

    def subtree(n):
        out = [n.id]
        for c in n.children:
            out += subtree(c)
        return out

    for n in tree.nodes:
        ids = subtree(n)
        row = rows[n.id]
        assert int(row[0]) == n.id and row[2] == n.label and int(row[1]) == (-1 if n is tree.root else n.jplace_edge)
        assert int(row[3]) == int(m[B + n.id]) and int(row[4]) == int(m[n.id])
        assert int(row[6]) == sum(int(m[B + i]) for i in ids) % 2 ** 64
        assert int(row[7]) == sum(int(m[i]) for i in ids) % 2 ** 64
        assert row[8] == "%.9f" % (float(int(row[7])) / 2 ** 30)
    assert sorted(subtree(tree.root)) == list(range(B))
