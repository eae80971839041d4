"""The host twins of the per-sample calls (rk_squash_host, rk_kmeans_host, rk_epca_host) against the numpy restatements on replicate
samples (tests/replicates.py): buffers in which every selection step -- the squash pick, the farthest-first seed, the nearest
centroid, the edge-PCA pivot -- runs on ties, where the other sample tests choose inputs on which every choice is decided.  The
header's tie rules are the specification.  For edge PCA also the finished output against numpy.linalg.eigvalsh(G) when the samples
hold fewer distinct profiles than components were asked for: components beyond the rank are +0.0, not a second copy of a leading
one.  No GPU."""
import numpy as np
import pytest

import rappas_amd as ra

from tests import epca_ref as E
from tests import kmeans_ref as K
from tests import kr_ref as R
from tests import replicates as P
from tests import squash_ref as Q

# (name, B, S, n_profiles, layout, empties): small shapes of both layouts, with and without samples that have no mass
SMALL = [("interleaved-26", 300, 26, 6, "interleaved", (3, 17)), ("blocked-26", 300, 26, 6, "blocked", (3, 17)), ("interleaved-48", 40, 48, 6, "interleaved", ()),
         ("blocked-48", 40, 48, 5, "blocked", (0, 47))]


def small_case(name):
    _, B, S, n_profiles, layout, empties = next(c for c in SMALL if c[0] == name)
    parent, bl = R.random_tree(B, 7 + B)
    m, labels = P.replicate_buffer(B, S, n_profiles, layout, 11 + S, empties)
    return parent, bl, m, labels, S, n_profiles


# ------------------------------------------------------------------------------------------------
# squash
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in SMALL])
def test_squash_twin_is_squash_ref_on_replicates(name):
    parent, bl, m, labels, S, _ = small_case(name)
    c = P.census(labels, near=P.near_sample(labels))
    assert c["tied_pairs"] >= 20 and c["blocks"] >= 4
    want, n_want = Q.squash_ref(parent, bl, m, S)
    got, n = ra.squash_host(parent, bl, m, S)
    assert n == n_want == np.count_nonzero(labels >= 0) - 1 and Q.same_rows(got, want)
    zero = int(np.count_nonzero(R.bits(want["distance"][:n]) == 0))
    print(name, "tied pairs at the first step", c["tied_pairs"], "merges at +0.0", zero, "of", n)
    assert zero >= 6 and tuple(want[0])[:2] == min((a, b) for a in range(S) for b in range(a + 1, S) if labels[a] == labels[b] >= 0 and P.near_sample(labels) not in (a, b))


def test_squash_twin_is_squash_ref_on_the_star():
    """every pair at one distance, exactly: the first merge is (0, 1) by the tie rule alone, and most later steps pick among ties"""
    S = 24
    parent, bl, m = P.star_singletons(S, 5)
    assert P.census(P.star_labels(S), all_pairs_tie=True)["tied_pairs"] == S * (S - 1) // 2
    want, n_want = Q.squash_ref(parent, bl, m, S)
    got, n = ra.squash_host(parent, bl, m, S)
    assert n == n_want == S - 1 and Q.same_rows(got, want)
    assert tuple(want[0])[:3] == (0, 1, 2) and want[0]["distance"] == np.float64(bl[1])


@pytest.mark.parametrize("n_profiles,layout,empties", [(6, "interleaved", ()), (4, "interleaved", (5,)), (4, "blocked", ())])
def test_squash_zero_distance_prefix_is_the_exact_runs(n_profiles, layout, empties):
    """S = 12, no near copy (in exact rationals it is at distance 0, in binary64 it need not be): the merges at +0.0 come first, every
    copy joins its profile by them, and their (a, b) sequence is the one the exact run picks by (distance, a, b)"""
    B, S = 40, 12
    parent, bl = R.random_tree(B, 3)
    m, labels = P.replicate_buffer(B, S, n_profiles, layout, 9, empties, triple=False)
    got, n = ra.squash_host(parent, bl, m, S)
    exact = Q.squash_exact(parent, bl, m, S)
    prefix = 0
    while prefix < n and R.bits(got[prefix]["distance"]) == 0:
        prefix += 1
    assert prefix == np.count_nonzero(labels >= 0) - n_profiles and len(exact) == n
    assert [(int(r["a"]), int(r["b"])) for r in got[:prefix]] == [(a, b) for a, b, _, _, _ in exact[:prefix]]
    assert all(d == 0 for _, _, _, d, _ in exact[:prefix]) and exact[prefix][3] > 0


# ------------------------------------------------------------------------------------------------
# k-means
# ------------------------------------------------------------------------------------------------
def check_kmeans(parent, bl, m, S, k, max_rounds, seeds=None):
    want = K.kmeans_ref(parent, bl, m, S, k, max_rounds, seeds)
    got = ra.kmeans_host(parent, bl, m, S, k, max_rounds, seeds=seeds)
    assert K.same(got, want), (k, max_rounds, got.info, want.info)
    empty = want.sizes == 0
    assert (R.bits(want.within[empty]) == 0).all() and (R.bits(got.within[empty]) == 0).all()
    return want


@pytest.mark.parametrize("name", [c[0] for c in SMALL[:3]])
def test_kmeans_twin_is_kmeans_ref_on_replicates(name):
    """k below, at and above the number of distinct profiles (the near copy counts as one more); one round and many"""
    parent, bl, m, labels, S, n_profiles = small_case(name)
    near = P.near_sample(labels)
    assert P.census(labels, near=near)["seed_ties"] >= 2
    for k in (3, n_profiles, n_profiles + 3):
        for max_rounds in (1, 50):
            want = check_kmeans(parent, bl, m, S, k, max_rounds)
            if k > n_profiles + 1:  # farthest-first ran out of distinct profiles: duplicates by index, without members after round one
                assert P.census(labels, near=near, k=k)["equidistant"] >= 2
                assert len({int(labels[s]) for s in want.seeds}) == n_profiles
                assert max_rounds > 1 or np.count_nonzero(want.sizes[:k] == 0) >= k - n_profiles - 1
                print(name, "k", k, "seeds", want.seeds, "sizes", want.sizes, "rounds", want.info[2], "converged", want.info[3])


def test_kmeans_callers_seeds_are_copies_of_one_profile():
    parent, bl, m, labels, S, n_profiles = small_case("interleaved-26")
    copies = [int(s) for s in np.nonzero(labels == 1)[0][:3]]
    for max_rounds in (1, 50):
        want = check_kmeans(parent, bl, m, S, 3, max_rounds, seeds=copies)
        assert want.sizes[0] == np.count_nonzero(labels >= 0) or max_rounds == 50  # round one: every sample is at one distance from all three
    one = K.kmeans_ref(parent, bl, m, S, 3, 1, copies)
    assert one.sizes.tolist() == [np.count_nonzero(labels >= 0), 0, 0]


@pytest.mark.parametrize("k", [3, 8])
def test_kmeans_twin_is_kmeans_ref_on_the_star(k):
    S = 24
    parent, bl, m = P.star_singletons(S, 5)
    c = P.census(P.star_labels(S), all_pairs_tie=True, k=k)
    assert c["seed_ties"] >= S - k + 1 and c["equidistant"] == S - k
    for max_rounds in (1, 50):
        want = check_kmeans(parent, bl, m, S, k, max_rounds)
        assert want.seeds == list(range(k))  # every candidate at one distance: the smaller sample
    one = K.kmeans_ref(parent, bl, m, S, k, 1)
    assert one.sizes.tolist() == [S - k + 1] + [1] * (k - 1)  # every other sample at one distance from all seeds: the smaller j


# ------------------------------------------------------------------------------------------------
# edge PCA
# ------------------------------------------------------------------------------------------------
def rank_case(name):
    _, B, S, n_profiles, layout, empties, rank = next(c for c in P.rank_families() if c[0] == name)
    parent, bl = R.random_tree(B, 91)
    m, labels = P.replicate_buffer(B, S, n_profiles, layout, 13 + S, empties, triple=False)
    return parent, bl, m, labels, B, S, rank


@pytest.mark.parametrize("name", [c[0] for c in P.rank_families()])
def test_epca_twin_is_epca_ref_and_eigvalsh_on_low_rank(name):
    """k = rank + 2: bit parity with the restatement, then 200 iterations (the drivers' default) against eigvalsh(G)"""
    parent, bl, m, labels, B, S, rank = rank_case(name)
    k = rank + 2
    prep = E.prepare(parent, bl, m, S)
    _, _, n, Xc, G, trace = prep
    assert n == np.count_nonzero(labels >= 0)
    if name.startswith("rank0"):
        assert (R.bits(G) == 0).all()  # (the family is exact: its mean is the sample itself)
    for iters in (1, 2, 40):
        want, want_info = E.iterate(prep, k, iters)
        got, info = ra.epca_host(parent, bl, m, S, k, iters)
        assert info.tolist() == want_info.tolist() == [n, min(k, n - 1)] and E.same(got, want), (name, iters)
    for k in (rank + 2, 8):
        raw, info = ra.epca_host(parent, bl, m, S, k, 200)
        f = ra.epca_finish(B, S, k, raw, info)
        P.check_epca_against_eigvalsh(f, raw, B, S, k, G, rank, noise=name.startswith("noise"))


@pytest.mark.parametrize("name", ["rank1-2x5", "rank2-3x4", "rank2-blocked-47"])
def test_epca_no_second_copy_of_a_leading_eigenvalue(name):
    """k = 4 and k = 8 at 40 iterations, where a column beyond the rank used to come back as the leading vector (rank2-3x4, k = 4:
    eigenvalue [1.1275, 0.7891, 3.4e-16, 1.1275], shares that sum to 1.59): whatever the iterations have reached, the components
    beyond the rank are +0.0 and the shares sum to 1 within the rounding of a length-S sum"""
    parent, bl, m, labels, B, S, rank = rank_case(name)
    for k in (4, 8):
        raw, info = ra.epca_host(parent, bl, m, S, k, 40)
        f = ra.epca_finish(B, S, k, raw, info)
        print(name, k, "eigenvalue", f.eigenvalue, "share", f.share)
        assert (f.eigenvalue[:rank] > 0).all() and f.share.sum() <= 1 + 64 * S * 2.0 ** -53
        for part in (f.eigenvalue[rank:], f.share[rank:], f.residual[rank:], f.projection[:, rank:], f.loading[:, rank:]):
            assert (R.bits(part) == 0).all()




def sweep_draws(n):
    """random small draws: S = 5 .. 20, B in {5, 40, 300}, two or three profiles, both layouts -- few samples and few profiles, where the
    rounding that the first iteration blows up lies almost in the null space of G and comes back tiny in every later product"""
    for seed in range(n):
        rng = np.random.default_rng(seed)
        B, S, n_profiles = int(rng.choice([5, 40, 300])), int(rng.integers(5, 21)), int(rng.integers(2, 4))
        yield seed, B, S, n_profiles, ("interleaved", "blocked")[seed % 2]


def test_epca_sweep_of_small_replicate_draws():
    """120 draws x k = rank + 2 and 8 x 40 and 200 iterations on the host twin (every fifth draw also bit for bit against the
    restatement): a column beyond the rank is all +0.0 whatever the draw -- not only on the seeds of rank_families -- and the
    components meet the eigvalsh bars; the residual bar where 200 iterations can have reached it.  A draw on B = 5 may have fewer
    distinct profiles than planted: the rank is eigvalsh's.  Columns whose first product is exactly zero are dead by the definition
    (P.dead_columns) and the components sit in the others."""
    failures, dead_seen = [], 0
    for seed, B, S, n_profiles, layout in sweep_draws(120):
        parent, bl = R.random_tree(B, 100 + seed)
        m, _ = P.replicate_buffer(B, S, n_profiles, layout, seed, (), triple=False)
        prep = E.prepare(parent, bl, m, S)
        G = prep[4]
        for k in (n_profiles + 1, 8):
            dead = P.dead_columns(G, S, min(k, S - 1))
            dead_seen += bool(dead)
            for iters in (40, 200):
                raw, info = ra.epca_host(parent, bl, m, S, k, iters)
                if seed % 5 == 0 and iters == 40:
                    want, want_info = E.iterate(prep, k, iters)
                    assert E.same(raw, want) and info.tolist() == want_info.tolist(), (seed, k)
                f = ra.epca_finish(B, S, k, raw, info)
                try:
                    P.check_epca_against_eigvalsh(f, raw, B, S, k, G, n_profiles - 1, dead=dead, at_most=True, iters=iters)
                except AssertionError as e:
                    failures.append((seed, B, S, n_profiles, layout, k, iters, f.eigenvalue.tolist(), str(e)[:80]))
    print("draws with a dead column:", dead_seen)
    assert not failures, failures[:5]


@pytest.mark.parametrize("B,tree_seed,S,seed,k,want_dead", [(5, 138, 13, 38, 3, ()), (40, 280, 14, 180, 3, ()), (40, 280, 14, 180, 8, ()), (40, 242, 5, 142, 3, (0,))])
def test_epca_columns_that_came_back_tiny(B, tree_seed, S, seed, k, want_dead):
    """two profiles on few samples: measured against its own delivered size alone, the blown-up rounding of iteration one stayed a
    fixed point (eigenvalue [3.2308, 0, 1.24e-16] on the first of these, [3.645, 1.94e-16, 0] on the second); against the largest
    delivered size of the live columns before it, it is caught.  The last case is the one where G takes the affine start vector of
    column 0 to zero exactly: that column is dead and the one component sits in column 1."""
    parent, bl = R.random_tree(B, tree_seed)
    m, _ = P.replicate_buffer(B, S, 2, "interleaved", seed, (), triple=False)
    prep = E.prepare(parent, bl, m, S)
    assert P.dead_columns(prep[4], S, min(k, S - 1)) == want_dead
    for iters in (40, 200):
        raw, info = ra.epca_host(parent, bl, m, S, k, iters)
        want, want_info = E.iterate(prep, k, iters)
        assert E.same(raw, want) and info.tolist() == want_info.tolist()
        P.check_epca_against_eigvalsh(ra.epca_finish(B, S, k, raw, info), raw, B, S, k, prep[4], 1, dead=want_dead, iters=iters)


def small_component_buffer(B, S, seed, eps_log2=11):
    """three profiles x S / 3 copies of which the third is the second plus 2^-eps_log2 of its total on one branch it has no mass on: a
    second component whose eigenvalue is about 2^-2 eps_log2 of the leading one times a few -- small, and real"""
    rng = np.random.default_rng(seed)
    W = 2 * B + 4
    a = rng.integers(1, 1 << 30, B, dtype=np.uint64) * (rng.random(B) < 0.3)
    b = rng.integers(1, 1 << 30, B, dtype=np.uint64) * (rng.random(B) < 0.3)
    c = b.copy()
    c[int(np.nonzero(b == 0)[0][0])] = np.uint64(int(b.sum()) >> eps_log2)
    m = np.zeros(S * W + 1, np.uint64)
    for s in range(S):
        m[s * W:s * W + B] = (a, b, c)[s % 3] * np.uint64(P.FACTORS[(s // 3) % 3])
    return m


def test_epca_rule_leaves_a_small_real_component_alone():
    """the figures round the factor of step 6, from the restatement's own trace (E.iterate(trace_to=...)): a second component at an
    eigenvalue ratio between 2^-20, what the header claims to resolve, and 2^-12 is never taken for rounding -- at its turn it
    stands far above the bound --, while the third and fourth columns, beyond the rank, are from the second iteration on; all four
    meet the eigvalsh conditions"""
    B, S, k = 300, 12, 4
    parent, bl = R.random_tree(B, 91)
    m = small_component_buffer(B, S, 3)
    prep = E.prepare(parent, bl, m, S)
    G = prep[4]
    w = np.linalg.eigvalsh(G)[::-1]
    print("eigvalsh", w[:4], "ratio of the second", w[1] / w[0])
    assert 2.0 ** -20 <= w[1] / w[0] <= 2.0 ** -12 and w[2] <= 64 * S * 2.0 ** -53 * w[0]
    trace = []
    want, want_info = E.iterate(prep, k, 40, trace_to=trace)
    raw, info = ra.epca_host(parent, bl, m, S, k, 40)
    assert E.same(raw, want) and info.tolist() == want_info.tolist()
    second = [top / against for it, j, p, top, against, zero in trace if j == 1 and it >= 1]
    zeroed = [top / against / (S * p) for it, j, p, top, against, zero in trace if zero and p and against]
    print("second column: top / scale at least", min(second), "against a bound of", S * 2.0 ** -40, "; zeroed columns: top / scale per projection and sample at most",
          max(zeroed) / 2.0 ** -53, "* 2^-53")
    assert not any(zero for it, j, p, top, against, zero in trace if j <= 1)
    assert all(zero for it, j, p, top, against, zero in trace if j >= 2 and it >= 1) and zeroed
    raw, info = ra.epca_host(parent, bl, m, S, k, 200)
    P.check_epca_against_eigvalsh(ra.epca_finish(B, S, k, raw, info), raw, B, S, k, G, 2, iters=200)


@pytest.mark.parametrize("S,a,b", [(2, 0, 1), (300, 7, 263), (300, 100, 300 - 1)])
def test_epca_pivot_tie_of_opposite_signs_goes_to_the_smaller_index(S, a, b):
    """two samples with mass on a star (P.star_singletons, only=): Y[0][b] == -Y[0][a] bit for bit in the first product, so only the
    rule 'the smallest index among equals' decides the sign of the component: q[a] = +1.0, q[b] = -1.0.  a and b in one thread of
    epca_orth_kernel's search (263 = 7 + 256) and in different waves"""
    parent, bl, m = P.star_singletons(S, 5, only=(a, b))
    prep = E.prepare(parent, bl, m, S)
    G = prep[4]
    assert G[a, a] == 0.5 and G[a, b] == -0.5 and G[b, b] == 0.5 and np.count_nonzero(G) == 4
    for iters in (1, 3):
        raw, info = ra.epca_host(parent, bl, m, S, 2, iters)
        want, want_info = E.iterate(prep, 2, iters)
        assert info.tolist() == want_info.tolist() == [2, 1] and E.same(raw, want)
        q = E.split(raw, S + 1, S, 2)[4]
        assert q[0, a] == 1.0 and q[0, b] == -1.0 and np.count_nonzero(q) == 2
