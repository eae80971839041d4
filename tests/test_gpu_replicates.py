"""The per-sample calls on the device (rk_squash_device, rk_kmeans_device, rk_epca_device) on replicate samples (tests/replicates.py),
at shapes where the device's geometry meets the ties: S = 600 on B <= 601, the smallest S at which tied pairs share a thread of
squash_pick_kernel (b apart by 256) and a block (a apart by 512), tied seeds and centroids spread over the one block of
kmeans_seed_kernel and the centroid groups of kmeans_dist_kernel, and edge-PCA pivots tie across the threads of epca_orth_kernel.
Every output equals the host twin's word for word, twice on one handle and on a second stream; the small families also equal the
numpy restatements directly; the edge-PCA output on low-rank input meets the eigvalsh conditions of tests/test_replicates_host.py."""
import functools

import numpy as np
import pytest

import rappas_amd as ra
from tests import epca_ref as E
from tests import kmeans_ref as K
from tests import kr_ref as R
from tests import replicates as P
from tests import squash_ref as Q

pytestmark = pytest.mark.gpu

S_BIG, N_PROFILES, EMPTIES = 600, 40, (3, 250, 257, 511, 598)


def to_dev(m):
    import torch
    return torch.from_numpy(np.ascontiguousarray(m).view(np.int64)).cuda()


@functools.lru_cache(maxsize=None)
def big_case(kind):
    """(parent, bl, buffer, labels, near, S, census arguments) of the three S = 600 families; made once"""
    if kind == "star":
        parent, bl, m = P.star_singletons(S_BIG, 5)
        return parent, bl, m, P.star_labels(S_BIG), None, S_BIG, dict(all_pairs_tie=True)
    parent, bl = R.random_tree(300, 77)
    m, labels = P.replicate_buffer(300, S_BIG, N_PROFILES, kind, 21, EMPTIES)
    near = P.near_sample(labels)
    return parent, bl, m, labels, near, S_BIG, dict(near=near)


def on_two_streams(call, same):
    """`call(stream)` twice on the current stream and once on a second one (the handle's workspace is one: the device is idle at every
    change of stream); `same(first, other)` must hold.  Returns the first result."""
    import torch
    first = call(None)
    assert same(first, call(None)), "the same call again on the handle"
    torch.cuda.synchronize()
    s2 = torch.cuda.Stream()
    other = call(s2.cuda_stream)
    s2.synchronize()
    assert same(first, other), "a second stream"
    return first


# ------------------------------------------------------------------------------------------------
# squash
# ------------------------------------------------------------------------------------------------
def squash_rows(et, dm, S, stream=None):
    import torch
    merges, n = et.squash(dm, S, stream=stream)
    torch.cuda.synchronize()
    return merges.cpu().numpy().reshape(-1).view(Q.SQUASH_MERGE), int(n.cpu().numpy()[0])


@pytest.mark.parametrize("kind", ["interleaved", "blocked", "star"])
def test_squash_equals_host_twin_on_tied_pairs(kind):
    parent, bl, m, labels, near, S, kw = big_case(kind)
    c = P.census(labels, **kw)
    print(kind, c)
    assert c["tied_pairs"] > 1000 and c["blocks"] > 256 and c["block_later_stride"] > 0  # other blocks; the same block, a later row
    if kind != "blocked":
        assert c["row_later_stride"] > 0     # the same row, a later pass of the thread loop
    if kind == "star":
        assert c["same_thread"] > 0          # ... and in the same thread
    want, n_want = ra.squash_host(parent, bl, m, S)
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)
        got, n = on_two_streams(lambda st: squash_rows(et, dm, S, st), lambda x, y: x[1] == y[1] and Q.same_rows(x[0], y[0]))
    finally:
        et.close()
    assert n == n_want == np.count_nonzero(np.asarray(labels) >= 0) - 1 and Q.same_rows(got, want), np.nonzero(got != want)[0][:4]
    if kind != "star":
        assert R.bits(got[0]["distance"]) == 0 and np.count_nonzero(R.bits(got["distance"][:n]) == 0) >= 200


def test_the_three_kinds_of_tie_are_all_there():
    total = {}
    for kind in ("interleaved", "blocked", "star"):
        _, _, _, labels, _, _, kw = big_case(kind)
        for name, v in P.census(labels, **kw).items():
            total[name] = total.get(name, 0) + v
    assert total["same_thread"] > 0 and total["block_later_stride"] > 0 and total["blocks"] > 3 * 256 and total["row_later_stride"] > 0


# ------------------------------------------------------------------------------------------------
# k-means
# ------------------------------------------------------------------------------------------------
def download(r):
    import torch
    torch.cuda.synchronize()
    host = lambda t, dt: t.cpu().numpy().view(dt)
    return ra.KMeans(host(r.assign, np.uint32), host(r.dist, np.float64), host(r.sizes, np.uint32), host(r.within, np.float64), host(r.info, np.uint32),
                     None if r.centroids is None else r.centroids.cpu().numpy())


def kmeans_on_device(et, dm, S, k, max_rounds, seeds=None, stream=None):
    return download(et.kmeans(dm, S, k, max_rounds, seeds=seeds, centroids=True, stream=stream))


def check_kmeans(parent, bl, m, S, k, max_rounds, seeds=None, et=None, dm=None, streams=False):
    own = et is None
    et = ra.EdgeTree(parent, bl) if own else et
    dm = to_dev(m) if dm is None else dm
    try:
        if streams:
            got = on_two_streams(lambda st: kmeans_on_device(et, dm, S, k, max_rounds, seeds, st), K.same)
        else:
            got = kmeans_on_device(et, dm, S, k, max_rounds, seeds)
    finally:
        if own:
            et.close()
    want = ra.kmeans_host(parent, bl, m, S, k, max_rounds, seeds=seeds)
    assert K.same(got, want), (k, max_rounds, got.info, want.info)
    empty = got.sizes == 0
    assert (R.bits(got.within[empty]) == 0).all()  # an empty cluster: size 0 and within +0.0
    return got


@pytest.mark.parametrize("kind", ["interleaved", "blocked"])
@pytest.mark.parametrize("k", [8, 41, 64])
def test_kmeans_equals_host_twin_on_replicates(kind, k):
    """k below the 40 profiles, one above (the near copy may or may not be a profile of its own) and far above: duplicate seeds taken
    by index, samples at +0.0 from two centroids, clusters that end empty"""
    parent, bl, m, labels, near, S, kw = big_case(kind)
    c = P.census(labels, k=k, **kw)
    assert c["seed_ties"] >= 2 and (k <= N_PROFILES + 1 or c["equidistant"] >= 2)
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)
        one = check_kmeans(parent, bl, m, S, k, 1, et=et, dm=dm, streams=True)
        got = check_kmeans(parent, bl, m, S, k, 50, et=et, dm=dm, streams=True)
    finally:
        et.close()
    assert one.info.tolist()[:3] == [k, S - len(EMPTIES), 1] and got.sizes.sum() == S - len(EMPTIES)
    if k > N_PROFILES + 1:  # round one: a copy is at +0.0 from its profile's first seed and from the duplicates behind it: the smaller j
        assert np.count_nonzero(one.sizes == 0) >= k - N_PROFILES - 1
    print(kind, k, "rounds", got.info[2], "sizes", got.sizes.tolist())


def test_kmeans_on_the_star_and_callers_seeds_of_one_profile():
    parent, bl, m, labels, _, S, kw = big_case("star")
    c = P.census(labels, k=8, **kw)
    assert c["seed_ties"] >= S - 7 and c["equidistant"] == S - 8
    for max_rounds in (1, 50):
        got = check_kmeans(parent, bl, m, S, 8, max_rounds, streams=True)
        assert got.info[0] == 8 and got.sizes.sum() == S
    one = check_kmeans(parent, bl, m, S, 8, 1)
    assert one.sizes.tolist() == [S - 7] + [1] * 7  # seeds 0..7 by index; every other sample at one distance from all of them: the smaller j
    parent, bl, m, labels, near, S, _ = big_case("interleaved")
    copies = [int(s) for s in np.nonzero(labels == 1)[0][[0, 5, 11]]]
    for max_rounds in (1, 50):
        got = check_kmeans(parent, bl, m, S, 3, max_rounds, seeds=copies, streams=True)
    one = check_kmeans(parent, bl, m, S, 3, 1, seeds=copies)
    assert one.sizes.tolist() == [S - len(EMPTIES), 0, 0]


def test_kmeans_every_rung_of_the_ladder_on_replicates(dev_lib, monkeypatch):
    """RK_KMEANS_KC (developer builds) forces the rung: k = 9 on 6 profiles, so that tied centroids sit in one group and in two"""
    B, S, k = 300, 130, 9
    parent, bl = R.random_tree(B, 21)
    m, labels = P.replicate_buffer(B, S, 6, "interleaved", 22, (7, 64))
    assert P.census(labels, near=P.near_sample(labels), k=k)["equidistant"] >= 2
    want = ra.kmeans_host(parent, bl, m, S, k, 50)
    for kc in ("1", "2", "4", "8"):
        monkeypatch.setenv("RK_KMEANS_KC", kc)
        et = ra.EdgeTree(parent, bl)
        try:
            dm = to_dev(m)
            got = on_two_streams(lambda st: kmeans_on_device(et, dm, S, k, 50, stream=st), K.same)
        finally:
            et.close()
        assert K.same(got, want), kc


# ------------------------------------------------------------------------------------------------
# edge PCA
# ------------------------------------------------------------------------------------------------
def keep_only(S, keep):
    return tuple(s for s in range(S) if s not in keep)


# (name, B, S, n_profiles, layout, empties, planted rank): the families of tests/replicates.py at S up to 300, where a column spans
# more than one pass of the block's 256 threads
BIG_RANK = [("rank0-n4-of-300", 300, 300, 1, "blocked", keep_only(300, (7, 100, 200, 299)), 0), ("noise-n3-of-300", 300, 300, 1, "blocked", keep_only(300, (0, 64, 257)), 0),
            ("rank1-300", 601, 300, 2, "interleaved", (3, 64, 250, 257, 299), 1), ("rank2-300", 300, 300, 3, "interleaved", (), 2),
            ("rank2-blocked-257", 300, 257, 3, "blocked", (0, 256), 2)]


@functools.lru_cache(maxsize=None)
def rank_case(name):
    _, B, S, n_profiles, layout, empties, rank = next(c for c in P.rank_families() + BIG_RANK if c[0] == name)
    parent, bl = R.random_tree(B, 91)
    m, labels = P.replicate_buffer(B, S, n_profiles, layout, 13 + S, empties, triple=False)
    return parent, bl, m, labels, B, S, rank, E.prepare(parent, bl, m, S)


def epca_raw(et, dm, S, k, iters, stream=None):
    import torch
    raw, info = et.epca(dm, S, k, iters, stream=stream)
    torch.cuda.synchronize()
    return raw.cpu().numpy(), info.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", [c[0] for c in P.rank_families() + BIG_RANK])
def test_epca_on_low_rank_input(name):
    """k = rank + 2 and k = 8: raw output and info equal the host twin's bit for bit -- zero columns from the first iteration on (rank
    0: epca_orth_kernel's zero branch with nothing applied, and n_j == 0 in epca_results_kernel) and columns the zero rule catches
    behind their projections --, and after 200 iterations the device's output meets the eigvalsh conditions; the small families
    equal the numpy restatement as well"""
    parent, bl, m, labels, B, S, rank, prep = rank_case(name)
    n, G = prep[2], prep[4]
    if name.startswith("rank0"):
        assert (R.bits(G) == 0).all()
    if name == "rank1-300":
        c = P.census(labels)
        assert c["pivot_ties"] >= 100 and c["pivot_threads"] >= 100  # the pivot of a column comes once per copy, over many threads
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)
        for k in (rank + 2, 8):
            for iters in (2, 200):
                same = lambda x, y: E.same(x[0], y[0]) and x[1].tolist() == y[1].tolist()
                call = lambda st: epca_raw(et, dm, S, k, iters, st)
                got, info = on_two_streams(call, same)
                want, want_info = ra.epca_host(parent, bl, m, S, k, iters)
                assert info.tolist() == want_info.tolist() == [n, min(k, n - 1)], (name, k, iters)
                assert E.same(got, want), (name, k, iters, np.nonzero(R.bits(got) != R.bits(want))[0][:8])
                if S <= 48 and iters == 2:
                    ref, ref_info = E.iterate(prep, k, iters)
                    assert E.same(got, ref) and info.tolist() == ref_info.tolist(), (name, k)
            f = ra.epca_finish(B, S, k, got, info)
            P.check_epca_against_eigvalsh(f, got, B, S, k, G, rank, noise=name.startswith("noise"))
    finally:
        et.close()


# ------------------------------------------------------------------------------------------------
# the small families against the restatements, with nothing of the engine in the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,n_profiles,layout,empties", [(300, 26, 6, "interleaved", (3, 17)), (40, 48, 5, "blocked", (0, 47))])
def test_small_families_equal_the_restatements(B, S, n_profiles, layout, empties):
    parent, bl = R.random_tree(B, 7 + B)
    m, labels = P.replicate_buffer(B, S, n_profiles, layout, 11 + S, empties)
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)
        got, n = squash_rows(et, dm, S)
        want, n_want = Q.squash_ref(parent, bl, m, S)
        assert n == n_want and Q.same_rows(got, want)
        for k, max_rounds in ((3, 50), (n_profiles + 3, 1), (n_profiles + 3, 50)):
            assert K.same(kmeans_on_device(et, dm, S, k, max_rounds), K.kmeans_ref(parent, bl, m, S, k, max_rounds)), (k, max_rounds)
    finally:
        et.close()
    parent, bl, m = P.star_singletons(24, 5)
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)
        got, n = squash_rows(et, dm, 24)
        want, n_want = Q.squash_ref(parent, bl, m, 24)
        assert n == n_want and Q.same_rows(got, want)
        assert K.same(kmeans_on_device(et, dm, 24, 8, 50), K.kmeans_ref(parent, bl, m, 24, 8, 50))
    finally:
        et.close()


@pytest.mark.parametrize("B,tree_seed,S,seed,k,dead", [(5, 138, 13, 38, 3, ()), (40, 280, 14, 180, 3, ()), (40, 280, 14, 180, 8, ()), (40, 242, 5, 142, 3, (0,))])
def test_epca_columns_that_came_back_tiny(B, tree_seed, S, seed, k, dead):
    """the draws of tests/test_replicates_host.py on which the blown-up rounding of iteration one came back tiny in every later
    product and stayed: the device equals the host twin and the restatement, and meets the eigvalsh conditions"""
    parent, bl = R.random_tree(B, tree_seed)
    m, _ = P.replicate_buffer(B, S, 2, "interleaved", seed, (), triple=False)
    prep = E.prepare(parent, bl, m, S)
    assert P.dead_columns(prep[4], S, min(k, S - 1)) == dead
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)
        for iters in (40, 200):
            got, info = epca_raw(et, dm, S, k, iters)
            want, want_info = ra.epca_host(parent, bl, m, S, k, iters)
            assert E.same(got, want) and info.tolist() == want_info.tolist(), iters
            if iters == 40:
                ref, _ = E.iterate(prep, k, iters)
                assert E.same(got, ref)
            P.check_epca_against_eigvalsh(ra.epca_finish(B, S, k, got, info), got, B, S, k, prep[4], 1, dead=dead, iters=iters)
    finally:
        et.close()


@pytest.mark.parametrize("S,a,b", [(2, 0, 1), (300, 7, 263), (300, 100, 299), (600, 300, 556)])
def test_epca_pivot_tie_of_opposite_signs_goes_to_the_smaller_index(S, a, b):
    """two samples with mass on a star: Y[0][b] == -Y[0][a] bit for bit, so only 'the smallest index among equals' decides the sign of
    the component -- a reduction that took the other one would give q[a] = -1.0.  a and b in one thread of epca_orth_kernel's search
    (b = a + 256), in different waves, and in one lane of different waves' later passes"""
    parent, bl, m = P.star_singletons(S, 5, only=(a, b))
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)
        for iters in (1, 3):
            got, info = epca_raw(et, dm, S, 2, iters)
            want, want_info = ra.epca_host(parent, bl, m, S, 2, iters)
            assert info.tolist() == want_info.tolist() == [2, 1] and E.same(got, want)
            q = E.split(got, S + 1, S, 2)[4]
            assert q[0, a] == 1.0 and q[0, b] == -1.0 and np.count_nonzero(q) == 2
    finally:
        et.close()
