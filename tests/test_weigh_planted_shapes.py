"""No GPU: the line trees of tests/weighplant.py hold what tests/test_gpu_weigh_planted.py needs -- the census of every (tree,
keep_at_most) it runs, counted from the oracle's score vectors alone -- and the three CPU statements of the weigh stage agree on
every read: tests/weigh_ref.py (mpmath, 100 digits), the oracle and tests/pyref.py, for every keep_at_most of planted.K_EDGES, keep_factor
0.0 / 0.01 / 0.5 / 1.0 and the ns_bound triple: n_rows and the BELOW_NSBOUND flag equal, LWR within tests/util.py: LWR_RTOL of
weigh_ref, +0.0 where it says +0.0, no cut decision of weigh_ref closer than 1e-12.  Prints the oracle's largest relative deviation."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import planted as P
from tests import pyref
from tests import weigh_ref as WR
from tests import weighplant as W
from tests.util import LWR_RTOL

CASES = [(name, None) for name in W.TREES] + [(name, amb) for name, modes in W.ASCII.items() for amb in modes]
IDS = [name + (f"-{amb}" if amb else "") for name, amb in CASES]
# An ambiguity code for the last symbol breaks no census count: its k-mer is the read's last one, which is no key; in "skip" it is left
# out (a read of one k-mer then touches nothing: more "none"), in "max" / "mean" an alternative is a key only by chance, which moves a few reads.


def test_every_line_tree_is_run_and_sized_like_a_planted_tree():
    assert set(W.ROUTES) == set(W.TREES) and set(W.ASCII) <= set(W.TREES)
    like = {"line999": "dna999", "lineaa399": "aa399", "line2801": "dna2801", "line9001": "dna9001", "linewg13301": "wg13301"}
    for name, (alphabet, k, nb, _, _, kw) in W.TREES.items():
        assert (alphabet, k, nb) == P.TREES[like[name]][:3] and kw.items() <= P.TREES[like[name]][6].items()


def test_the_palette_lands_on_the_line():
    """one hit at T with Q = 56 is -308.0f, at T + 2**-15 the float above it; Q = 57 with a hit at T + 5.5 - 2**-15 the float below"""
    f = np.float32
    assert f(56) * W.T + (f(W.T) - W.T) == W.LINE
    assert f(f(56) * W.T) + f(f(float(W.T) + W.STEP) - W.T) == W.LINE_ABOVE
    assert f(f(57) * W.T) + f(f(-W.STEP) - W.T) == W.LINE_BELOW
    assert [float(f(q) * W.T) for q in W.Q_ALL] == [-5.5, -44.0, -302.5, -308.0, -313.5, -396.0, -775.5]


@pytest.mark.parametrize("name,amb", CASES, ids=IDS)
def test_census(name, amb):
    vectors = W.vectors_of(name, amb)
    for K in P.K_EDGES:
        print(name, amb, K, W.assert_census(vectors, K, f"{name} {amb or ''}"))
    print(name, amb, "ns_bound", W.ns_bounds(vectors))


def pyref_db(sdb):
    off = sdb.row_offsets.astype(np.int64)
    rows = {int(c): list(zip(sdb.branch_ids[off[i]:off[i + 1]].tolist(), sdb.scores[off[i]:off[i + 1]]))
            for i, c in enumerate(sdb.key_codes)}
    return dict(alphabet=sdb.alphabet, k=sdb.k, n_branches=sdb.n_branches, T=sdb.thr_log10, P=sdb.thr, rows=rows)


@pytest.mark.parametrize("name,amb", CASES, ids=IDS)
def test_the_three_references_agree(name, amb):
    sdb, odb, seq, off, _ = W.tree(name)
    if amb is not None:
        seq, _ = W.ambiguous(name, amb)
    vectors = W.vectors_of(name, amb)
    pydb = pyref_db(sdb)
    scored = []
    for r, (order, bits) in enumerate(vectors):
        py = pyref.place_read(pydb, bytes(seq[int(off[r]):int(off[r + 1])]).decode(), amb_mode=amb or "mean")
        assert sorted(py["L"]) == sorted(order.tolist()), (name, r)
        assert all(np.float32(py["S"][b]).view(np.uint32) == s for b, s in zip(order.tolist(), bits.tolist())), (name, r)
        # the whole of place_read once a read, below; for the other calls its select and weigh on the 17 best touched branches, in the
        # order they were touched in (the same kept scores: this file is about what follows the select, and L has up to 50 000 entries)
        first = set(order[:17].tolist())
        scored.append((py, [b for b in py["L"] if b in first]))
    worst, closest = 0.0, 1.0
    for K, kf, bound in W.calls(name, amb):
        ref = W.oracle_place(name, K, kf, amb, bound)
        for r, (order, bits) in enumerate(vectors):
            n, lwr, below, margin = WR.weigh(bits[:K].view(np.float32), kf, bound)
            what = (name, amb, K, kf, bound, r)
            if margin is not None:
                closest = min(closest, margin)
                assert margin >= WR.UNDECIDED, what
            py, kept = scored[r]
            flags = set()
            if (K, kf, bound) == (7, 0.01, float("-inf")):  # place_read's defaults
                rows, flags = py["rows"], py["flags"]
            elif len(order):
                rows = pyref.select_and_weigh(py["S"], kept, flags, K, kf, bound)
            else:
                rows = []
            assert n == len(rows) == int(ref["n_rows"][r]), what + (n, len(rows), int(ref["n_rows"][r]))
            assert below == ("below_nsbound" in flags) == bool(ref["flags"][r] & O.RO_FLAG_BELOW_NSBOUND), what
            for i in range(n):
                for got in (float(ref["lwr"][r, i]), rows[i][2]):
                    if lwr[i] == 0.0:
                        assert got == 0.0 and not np.signbit(got), what + (i, got)
                    else:
                        assert abs(got - lwr[i]) <= LWR_RTOL * lwr[i], what + (i, got, lwr[i])
                if lwr[i] != 0.0:
                    worst = max(worst, abs(float(ref["lwr"][r, i]) - lwr[i]) / lwr[i])
    print(f"{name} {amb or ''}: the oracle's largest relative LWR deviation from weigh_ref {worst:.3g}; closest cut decision {closest:.3g}")
