"""No GPU: the planted databases and reads of tests/test_gpu_tie_order.py hold every adversarial shape -- counted in each kernel family's
own layout (tests/planted.py) -- that can occur on their tree, for every (tree, kernel, keep_at_most list) the GPU file runs; and the
plain-sort reference of the engine's order agrees with the oracle on every read's score row.  A shape that went missing (another seed,
fewer reads, a changed generator) is found here, without a GPU."""
import numpy as np
import pytest

from tests import planted as P

TREES_USED = sorted({c[0] for c in P.CASES})


def test_every_planted_tree_is_used_and_known():
    assert set(TREES_USED) == set(P.TREES)


@pytest.mark.parametrize("name,route,Ks,amb", P.CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_every_shape_is_met(name, route, Ks, amb):
    sdb, _, _, _, vectors = P.tree(name)
    if amb is not None:
        _, vectors = P.ambiguous(name, amb)
    fam = P.family(route, sdb.n_branches, sdb.bits)
    P.assert_census(vectors, Ks, fam, sdb.n_branches, f"{name} {route}")


@pytest.mark.parametrize("name", TREES_USED)
def test_the_window_rows_follow_the_image_windows(name):
    """the windows planted_db cut the tree into are those rk_geometry.h's window_plan gives the image"""
    alphabet, _, nb, _, _, _, kw, _ = P.TREES[name]
    if "window" in kw:
        bits = 5 if alphabet == 20 else 2
        assert kw["window"] == P.window_plan(nb, bits, bits == 5 or nb > 4500)[1]


def _check_rows(ref, vectors, K):
    for r, (order, bits) in enumerate(vectors):
        n = int(ref["n_rows"][r])
        assert n <= min(K, len(order)) and (n > 0) == (len(order) > 0), (r, K, n, len(order))
        assert np.array_equal(ref["score"][r, :n].view(np.uint32), bits[:n]), (r, K, ref["score"][r, :n], bits[:K].view(np.float32))
        # the oracle's branches are true (branch, score) pairs of the sorted vector; where no score repeats they are its order itself
        rank = {int(b): i for i, b in enumerate(order)}
        for i in range(n):
            b = int(ref["branch"][r, i])
            assert b in rank and bits[rank[b]] == bits[i], (r, K, i, b)
        if len(set(bits[:n + 1].tolist())) == len(bits[:n + 1]):
            assert np.array_equal(ref["branch"][r, :n].astype(np.int64), order[:n]), (r, K)


@pytest.mark.parametrize("name", TREES_USED)
def test_plain_sort_and_oracle_agree_on_the_score_rows(name):
    _, _, _, _, vectors = P.tree(name)
    for K in (1, 8, 16):
        for kf in (0.0, 0.01):
            _check_rows(P.oracle_place(name, K, kf), vectors, K)


@pytest.mark.parametrize("amb", ["skip", "max", "mean"])
@pytest.mark.parametrize("name", sorted({c[0] for c in P.CASES if c[3]}))
def test_plain_sort_and_oracle_agree_with_ambiguity_codes(name, amb):
    _, vectors = P.ambiguous(name, amb)
    for K in (1, 8, 16):
        _check_rows(P.oracle_place(name, K, 0.01, amb), vectors, K)
