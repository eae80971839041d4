"""The edge PCA on the host (rk_epca_host, rk_epca_finish_host) against its definition restated in tests/epca_ref.py:
bit parity with the numpy restatement, the special samples, the k_eff rule, every thread count, the eigenvalues against
numpy.linalg.eigvalsh on a planted buffer, what the projections and the loadings must satisfy there, the finish, the refused
arguments, and the two epca_table writers.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, hostio

from tests import epca_ref as E
from tests import kr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def trees():
    for B in (1, 2, 300, 2049):
        yield f"star-{B}", R.star(B, B)
        yield f"caterpillar-{B}", R.caterpillar(B, B)
        yield f"random-{B}", R.random_tree(B, 60 + B)


@pytest.mark.parametrize("name,tree", list(trees()), ids=[n for n, _ in trees()])
def test_host_twin_is_epca_ref_bit_for_bit(name, tree):
    """S on both sides of the 64-lane edge; k below, at and above S - 1; iters = 1 shows G itself"""
    parent, bl = tree
    B = len(parent)
    for S in (2, 3, 65, 130):
        m = R.sample_buffer(B, S, seed=3 * B + S)
        prep = E.prepare(parent, bl, m, S)  # (steps 1 - 4 depend on neither k nor iters: once a shape)
        for k in (1, 5, 8):
            for iters in (1, 3):
                want, want_info = E.iterate(prep, k, iters)
                got, info = ra.epca_host(parent, bl, m, S, k, iters)
                assert info.tolist() == want_info.tolist() == [S, min(k, S - 1)], (name, S, k, iters)
                assert E.same(got, want), (name, S, k, iters, np.nonzero(R.bits(got) != R.bits(want))[0][:8])


@pytest.mark.parametrize("B,S", [(300, 6), (2049, 5), (5, 7)])
def test_special_buffer_empty_sample_and_identical_samples(B, S):
    """sample 1 is empty: it is not counted and its q entries are zeros (their sign is the sign of the column's divisor: +0.0 / -x is
    -0.0 by IEEE, so the definition as written gives a zero of either sign, and the projection with it); samples 2 and 3 are
    identical: G is bitwise symmetric, which shows as the same bits in their projections"""
    parent, bl = R.random_tree(B, 70 + B)
    m = R.special_buffer(B, S, 71)
    k = 3
    got, info = ra.epca_host(parent, bl, m, S, k, 20)
    want, want_info = E.epca_ref(parent, bl, m, S, k, 20)
    assert info.tolist() == want_info.tolist() == [S - 1, min(k, S - 2)] and E.same(got, want)
    q = E.split(got, B, S, k)[4]
    assert (q[:, 1] == 0.0).all()
    f = ra.epca_finish(B, S, k, got, info)
    assert (f.projection[1] == 0.0).all() and E.same(f.projection[2], f.projection[3])
    _, _, _, _, G, _ = E.prepare(parent, bl, m, S)
    assert (R.bits(G) == R.bits(G.T)).all() and (R.bits(G[1]) == 0).all() and (R.bits(G[:, 1]) == 0).all()


def test_every_sample_empty_and_one_sample_with_mass():
    B, S, k = 40, 5, 4
    parent, bl = R.random_tree(B, 5)
    m = np.zeros(S * (2 * B + 4) + 1, np.uint64)
    for n in (0, 1):
        if n:
            m[3 * (2 * B + 4) + 7] = 99
        got, info = ra.epca_host(parent, bl, m, S, k, 3)
        want, want_info = E.epca_ref(parent, bl, m, S, k, 3)
        assert info.tolist() == want_info.tolist() == [n, 0]
        assert len(got) == E.out_doubles(B, S, k) and (R.bits(got) == 0).all() and (R.bits(want) == 0).all()


def test_three_samples_eight_components():
    B, S, k = 300, 3, 8
    parent, bl = R.random_tree(B, 17)
    got, info = ra.epca_host(parent, bl, R.sample_buffer(B, S, 18), S, k, 30)
    assert info.tolist() == [3, 2]
    trace, lam, nn, rr, q, w = E.split(got, B, S, k)
    assert (lam[:2] > 0).all() and (nn[:2] >= 1).all()
    for part in (lam[2:], nn[2:], rr[2:], q[2:], w[2:]):
        assert (R.bits(part) == 0).all()
    f = ra.epca_finish(B, S, k, got, info)
    assert (R.bits(f.projection[:, 2:]) == 0).all() and (R.bits(f.loading[:, 2:]) == 0).all() and (R.bits(f.eigenvalue[2:]) == 0).all()


def test_the_same_bits_from_every_thread_count():
    B, S, k = 2049, 20, 5
    parent, bl = R.random_tree(B, 81)
    m = R.special_buffer(B, S, 82)
    want, want_info = ra.epca_host(parent, bl, m, S, k, 5, threads=1)
    for threads in list(range(2, 17)) + [0]:
        got, info = ra.epca_host(parent, bl, m, S, k, 5, threads=threads)
        assert info.tolist() == want_info.tolist() and E.same(got, want), threads


@pytest.fixture(scope="module")
def planted():
    """B = 300, S = 9, three planted groups; k = 2, iters = 128: the run, its finish, and the restatement's Xc and G"""
    B, S, k, iters = 300, 9, 2, 128
    parent, bl = R.random_tree(B, 91)
    m = E.planted_buffer(B, S, 5)
    raw, info = ra.epca_host(parent, bl, m, S, k, iters)
    _, _, n, Xc, G, trace = E.prepare(parent, bl, m, S)
    assert info.tolist() == [9, 2] and n == 9
    return B, S, k, raw, ra.epca_finish(B, S, k, raw, info), Xc, G


def test_eigenvalues_against_eigvalsh(planted):
    """for j < 2: min_i |eigenvalue_j - w_i| <= residual_j + 64 * S * 2^-53 * w_0 -- the residual bound of a symmetric matrix, and slack
    for the rounding of the length-S dots themselves -- and residual_j <= 1e-12 * eigenvalue_0"""
    B, S, k, raw, f, Xc, G = planted
    assert (R.bits(G) == R.bits(G.T)).all()
    w = np.linalg.eigvalsh(G)[::-1]
    for j in range(k):
        gap = np.abs(f.eigenvalue[j] - w).min()
        print("component", j, "eigenvalue", f.eigenvalue[j], "nearest eigvalsh", gap, "residual", f.residual[j], "share", f.share[j])
        assert gap <= f.residual[j] + 64 * S * 2.0 ** -53 * w[0]
        assert f.residual[j] <= 1e-12 * f.eigenvalue[0]
    assert f.eigenvalue[0] > f.eigenvalue[1] > 0 and abs(f.share[0] - f.eigenvalue[0] / E.split(raw, B, S, k)[0]) == 0


def test_projections_split_the_planted_groups(planted):
    """component 0: equal within a group to 1e-3 of the spread, distinct across at least two groups"""
    B, S, k, raw, f, Xc, G = planted
    p = f.projection[:, 0]
    spread = p.max() - p.min()
    centre = [p[g::3].mean() for g in range(3)]
    for g in range(3):
        assert np.abs(p[g::3] - centre[g]).max() <= 1e-3 * spread
    assert max(abs(centre[a] - centre[b]) for a in range(3) for b in range(a)) > 0.1 * spread
    assert len({round(c / spread, 2) for c in centre}) >= 2


def test_loadings_are_unit_orthogonal_and_give_the_projections(planted):
    """the loadings columns are unit and orthogonal to 1e-9; projection = Xc-rows . loading to 1e-9 relative"""
    B, S, k, raw, f, Xc, G = planted
    L = f.loading
    gram = L.T @ L
    assert np.abs(gram - np.eye(k)).max() <= 1e-9
    back = Xc.T @ L  # [S, k]
    assert np.abs(back - f.projection).max() <= 1e-9 * np.abs(f.projection).max()


def test_finish_against_numpy_and_its_zero_rule():
    B, S, k = 300, 6, 5
    parent, bl = R.random_tree(B, 33)
    raw, info = ra.epca_host(parent, bl, R.special_buffer(B, S, 34), S, k, 25)
    f = ra.epca_finish(B, S, k, raw, info)
    ev, share, res, proj, load = E.finish_ref(B, S, k, raw)
    assert (f.n_active, f.k_eff) == (5, 4)
    for got, want in ((f.eigenvalue, ev), (f.share, share), (f.residual, res), (f.projection, proj), (f.loading, load)):
        assert got.shape == want.shape and np.allclose(got, want, rtol=4e-16, atol=0)  # (numpy's sqrt and / are correctly rounded too: an ulp for the order of the operations)
    assert (R.bits(f.eigenvalue[4:]) == 0).all() and (R.bits(f.projection[:, 4]) == 0).all() and (R.bits(f.loading[:, 4]) == 0).all()
    # the zero rule: a component with lambda <= 0 or nn == 0 is all +0.0, whatever else the raw output holds
    bad = raw.copy()
    bad[1 + 0] = -1.0       # lambda_0 <= 0
    bad[1 + k + 1] = 0.0    # nn_1 == 0
    g = ra.epca_finish(B, S, k, bad)
    for arr in (g.eigenvalue, g.share, g.residual):
        assert (R.bits(arr[:2]) == 0).all()
    assert (R.bits(g.projection[:, :2]) == 0).all() and (R.bits(g.loading[:, :2]) == 0).all()
    assert E.same(g.projection[:, 2:4].copy(), f.projection[:, 2:4].copy()) and not np.isnan(g.loading).any()


def test_bad_arguments():
    lib = _lib.load()
    B = 3
    p, b = np.array([-1, 0, 0], np.int32), np.array([0, 1, 1], np.float32)
    m = R.sample_buffer(B, 4, 1)
    n_out = 1 + 2 * (3 + 4 + B)
    assert lib.rk_epca_out_doubles(B, 4, 2) == n_out
    raw = np.full(n_out, 7.0)
    info = np.full(2, 77, np.uint32)

    def call(B=B, parent=p.ctypes.data, lens=b.ctypes.data, S=4, masses=m.ctypes.data, k=2, iters=3, out=raw.ctypes.data, inf=info.ctypes.data):
        return lib.rk_epca_host(B, parent, lens, S, masses, k, iters, out, inf, 1)

    assert call() == _lib.RK_OK and info.tolist() == [4, 2]
    raw[:] = 7.0
    info[:] = 77
    big = np.zeros(4097 * (2 * B + 4) + 1, np.uint64)
    for kw, text in ((dict(S=1), b"2..4096"), (dict(S=0), b"2..4096"), (dict(S=4097, masses=big.ctypes.data), b"2..4096"), (dict(k=0), b"1..8"), (dict(k=9), b"1..8"),
                     (dict(iters=0), b"1..10000"), (dict(iters=10001), b"1..10000"), (dict(parent=None), b"null"), (dict(lens=None), b"null"),
                     (dict(masses=None), b"null mass buffer"), (dict(out=None), b"null output"), (dict(inf=None), b"null output"), (dict(B=0), b"1..65535")):
        assert call(**kw) == _lib.RK_ERR_INVALID and text in lib.rk_last_error(), kw
    for parent, lens in (([1, 2, 0], [1, 1, 1]), ([-1, -1, 0], [1, 1, 1]), ([-1, 0, 0], [0, -1, 1])):
        pp, bb = np.array(parent, np.int32), np.array(lens, np.float32)
        assert call(parent=pp.ctypes.data, lens=bb.ctypes.data) == _lib.RK_ERR_INVALID
    assert (raw == 7.0).all() and info.tolist() == [77, 77]  # nothing is written
    assert lib.rk_epca_work_bytes(None, 3, 2) == 0 and b"null tree" in lib.rk_last_error()
    for args in ((B, 1, 2), (B, 4097, 2), (B, 4, 0), (B, 4, 9), (0, 4, 2), (65536, 4, 2)):
        assert lib.rk_epca_out_doubles(*args) == 0
    ev = np.zeros(2)
    pr, ld = np.zeros((4, 2)), np.zeros((B, 2))
    ok = lambda **kw: lib.rk_epca_finish_host(kw.get("B", B), kw.get("S", 4), kw.get("k", 2), kw.get("raw", raw.ctypes.data), ev.ctypes.data, ev.ctypes.data,
                                              kw.get("res", ev.ctypes.data), pr.ctypes.data, kw.get("ld", ld.ctypes.data))
    assert ok() == _lib.RK_OK
    for kw in (dict(raw=None), dict(res=None), dict(ld=None), dict(S=1), dict(k=9), dict(B=0)):
        assert ok(**kw) == _lib.RK_ERR_INVALID, kw
    with pytest.raises(ra.RkError):
        ra.epca_host(p, b, R.sample_buffer(B, 1, 1), 1, 2, 3)


def table_cases():
    """(names, B, k, iters, n_active, k_eff, eigenvalue, share, residual, projection, loading): a real run with an empty sample and names
    with blanks; no sample with mass; made-up values with tiny and negative numbers"""
    B, S, k = 40, 6, 3
    parent, bl = R.random_tree(B, 3)
    raw, info = ra.epca_host(parent, bl, R.special_buffer(B, S, 4), S, k, 40)
    f = ra.epca_finish(B, S, k, raw, info)
    yield ["a", "b b", "c'1", "d(x)", "e,f", "g:h"], B, k, 40, f.n_active, f.k_eff, f.eigenvalue, f.share, f.residual, f.projection, f.loading
    raw, info = ra.epca_host(parent, bl, np.zeros(S * (2 * B + 4) + 1, np.uint64), S, k, 2)
    f = ra.epca_finish(B, S, k, raw, info)
    yield ["p", "q", "r", "s", "t", "u"], B, k, 2, f.n_active, f.k_eff, f.eigenvalue, f.share, f.residual, f.projection, f.loading
    yield (["w", "x y"], 2, 2, 7, 2, 1, np.array([1e-300, 0.0]), np.array([1.0, 0.0]), np.array([0.1, 0.0]), np.array([[-1 / 3, 0.0], [1 / 3, -0.0]]),
           np.array([[0.5, 0.0], [-2.5e17, 0.0]]))


def test_epca_table_text():
    cases = list(table_cases())
    text = hostio.epca_table(*cases[2])
    tiny, third = "%.17g" % 1e-300, "%.17g" % (1 / 3)
    assert text == ("#epca\t2\t2\t2\t2\t1\t7\n#eigenvalue\t" + tiny + "\t0\n#share\t1\t0\n#residual\t0.10000000000000001\t0\n#projections\nw\t-" + third +
                    "\t0\nx y\t" + third + "\t-0\n#loadings\n0\t0.5\t0\n1\t-2.5e+17\t0\n#samples_without_mass\t0\n")
    lines = hostio.epca_table(*cases[0]).splitlines()
    assert lines[0] == "#epca\t6\t40\t3\t5\t3\t40" and lines[-1] == "#samples_without_mass\t1" and lines[4] == "#projections" and lines[11] == "#loadings"
    assert len(lines) == 13 + 40 and lines[6].split("\t")[0] == "b b" and all(float(v) == 0 for v in lines[6].split("\t")[1:])
    assert float(lines[1].split("\t")[1]) == cases[0][6][0]  # %.17g round-trips
    empty = hostio.epca_table(*cases[1])
    assert "nan" not in empty and "nan" not in "\n".join(lines) and empty.splitlines()[0] == "#epca\t6\t40\t3\t0\t0\t2" and empty.endswith("#samples_without_mass\t6\n")


def test_epca_table_twins_are_byte_identical(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.skip("no C++ compiler (g++)")
    exe = str(tmp_path / "epca_table")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "rappas_amd", "csrc"), os.path.join(ROOT, "tests", "epca_table.cpp"),
                    "-o", exe], check=True)
    for i, (names, B, k, iters, n_active, k_eff, ev, share, res, proj, load) in enumerate(table_cases()):
        d = tmp_path / str(i)
        d.mkdir()
        (d / "names.txt").write_bytes("".join(nm + "\n" for nm in names).encode())
        np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in (ev, share, res, proj, load)]).tofile(str(d / "values.bin"))
        got = subprocess.run([exe, str(d / "names.txt"), str(B), str(k), str(iters), str(n_active), str(k_eff), str(d / "values.bin")], capture_output=True,
                             check=True, timeout=60).stdout
        want = hostio.epca_table(names, B, k, iters, n_active, k_eff, ev, share, res, proj, load).encode()
        assert got == want and b"nan" not in got, i
