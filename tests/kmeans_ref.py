"""The phylogenetic k-means of include/rappas_place.h restated in numpy, operation by operation in the order the header fixes (the KR
pair sum of tests/squash_ref.py, Python loops for the ordered sums of the update), and in exact rationals with the gaps that decide
every choice of the run -- the nearest and the second-nearest centroid of every sample in every round, the farthest and the
second-farthest candidate of every seeding step -- so that a test can tell whether the run is decided.  Also the planted buffers.
Trees, buffers and the clade sums come from tests/kr_ref.py."""
import collections
from fractions import Fraction

import numpy as np

from tests import kr_ref as R
from tests import squash_ref as Q

NONE = 0xFFFFFFFF
GROUP = 256
KMeansRef = collections.namedtuple("KMeansRef", "assign dist sizes within info centroids seeds")


def profiles(parent, bl, m, S):
    """(h [B], u [S, B], v [S, B], active [S]) in binary64 as the KR block defines them"""
    B = len(parent)
    root, _ = R.preorder(parent)
    mass, c = R.masses_of(m, B, S), R.clade_ref(parent, m, S)
    h = np.asarray(bl, np.float32).astype(np.float64) * 0.5
    h[root] = 0.0
    with np.errstate(all="ignore"):
        T = c[:, root].astype(np.float64)
        u = c.astype(np.float64) / T[:, None]
        v = (c - mass).astype(np.float64) / T[:, None]
    return h, u, v, [int(c[s, root]) != 0 for s in range(S)]


def fillers(B, S, k, k_eff, n_active, status, seeds=()):
    return KMeansRef(np.full(S, NONE, np.uint32), np.zeros(S), np.zeros(k, np.uint32), np.zeros(k), np.array([k_eff, n_active, 0, 1 | status << 1], np.uint32),
                     np.zeros((k, 2, B)), list(seeds))


def ordered_mean(rows, members):
    """the update rule: one partial per group of 256 sample indices from +0.0, member after member; the partials of the groups that hold
    a member added in group order, the first one as it is; then the division"""
    total = None
    for g0 in range(min(members) // GROUP * GROUP, max(members) + 1, GROUP):
        inside = [s for s in members if g0 <= s < g0 + GROUP]
        if not inside:
            continue
        p = np.zeros(rows.shape[1])
        for s in inside:
            p = p + rows[s]
        total = p if total is None else total + p
    return total / np.float64(len(members))


def kmeans_ref(parent, bl, m, S, k, max_rounds=100, seeds=None):
    B = len(parent)
    h, u, v, active = profiles(parent, bl, m, S)
    act = [s for s in range(S) if active[s]]
    n_active = len(act)
    if seeds is not None:
        k_eff, status = k, int(any(not active[s] for s in seeds))
        seeds = [int(s) for s in seeds]
    else:
        k_eff, status = min(k, n_active), 0
    if n_active == 0 or status:
        return fillers(B, S, k, k_eff, n_active, status, seeds or ())
    with np.errstate(all="ignore"):
        if seeds is None:  # farthest-first
            seeds, mind = [act[0]], {}
            for j in range(1, k_eff):
                t = seeds[-1]
                best = None
                for s in act:
                    d = Q.pair_ref(h, u[t], v[t], u[s], v[s])
                    mind[s] = d if j == 1 or d < mind[s] else mind[s]
                    if s not in seeds and (best is None or mind[s] > mind[best]):
                        best = s
                seeds.append(best)
        cu, cv = u[seeds].copy(), v[seeds].copy()
        assign, dist = np.full(S, NONE, np.uint32), np.zeros(S)
        rounds = converged = 0
        while rounds < max_rounds and not converged:
            changed = 0
            for s in act:
                best, bd = 0, None
                for j in range(k_eff):
                    d = Q.pair_ref(h, cu[j], cv[j], u[s], v[s])
                    if bd is None or d < bd:
                        best, bd = j, d
                changed += int(assign[s] != best)
                assign[s], dist[s] = best, bd
            rounds += 1
            if changed == 0:
                converged = 1
                break
            for j in range(k_eff):
                members = [s for s in act if assign[s] == j]
                if members:
                    cu[j], cv[j] = ordered_mean(u, members), ordered_mean(v, members)
    sizes, within = np.zeros(k, np.uint32), np.zeros(k)
    for s in act:
        sizes[assign[s]] += 1
        within[assign[s]] = within[assign[s]] + dist[s]
    cen = np.zeros((k, 2, B))
    cen[:k_eff, 0], cen[:k_eff, 1] = cu, cv
    return KMeansRef(assign, dist, sizes, within, np.array([k_eff, n_active, rounds, converged], np.uint32), cen, seeds)


KMeansExact = collections.namedtuple("KMeansExact", "seeds seed_gaps round_gaps assign dist rounds converged")


def kmeans_exact(parent, bl, m, S, k, max_rounds=100, seeds=None):
    """the same run without rounding (every active sample, at least one of them).  seed_gaps: per seeding step (best, second), the
    largest and the second-largest mind among the candidates (second None with one candidate).  round_gaps: per round a dict s ->
    (best, second), the smallest and the second-smallest centroid distance of sample s (second None with one centroid).  assign and
    dist (Fractions) as they stand at the end."""
    B = len(parent)
    root, _ = R.preorder(parent)
    mass, c = R.masses_of(m, B, S), R.clade_ref(parent, m, S)
    h = [Fraction(float(np.float32(bl[x]))) / 2 if x != root else Fraction(0) for x in range(B)]
    act = [s for s in range(S) if int(c[s, root]) != 0]
    u = {s: [Fraction(int(c[s, x]), int(c[s, root])) for x in range(B)] for s in act}
    v = {s: [Fraction(int(c[s, x]) - int(mass[s, x]), int(c[s, root])) for x in range(B)] for s in act}

    def d_of(au, av, bu, bv):
        return sum(h[x] * (abs(au[x] - bu[x]) + abs(av[x] - bv[x])) for x in range(B))

    seed_gaps = []
    if seeds is None:
        k_eff = min(k, len(act))
        seeds, mind = [act[0]], {}
        for j in range(1, k_eff):
            t = seeds[-1]
            for s in act:
                d = d_of(u[t], v[t], u[s], v[s])
                mind[s] = d if j == 1 else min(d, mind[s])
            cands = sorted(((-mind[s], s) for s in act if s not in seeds))
            seed_gaps.append((-cands[0][0], -cands[1][0] if len(cands) > 1 else None))
            seeds.append(cands[0][1])
    else:
        k_eff, seeds = k, [int(s) for s in seeds]
    cu, cv = [list(u[s]) for s in seeds], [list(v[s]) for s in seeds]
    assign, dist, round_gaps = {s: None for s in act}, {}, []
    rounds = converged = 0
    while rounds < max_rounds and not converged:
        changed, gaps = 0, {}
        for s in act:
            ds = sorted((d_of(cu[j], cv[j], u[s], v[s]), j) for j in range(k_eff))
            gaps[s] = (ds[0][0], ds[1][0] if k_eff > 1 else None)
            changed += assign[s] != ds[0][1]
            assign[s], dist[s] = ds[0][1], ds[0][0]
        round_gaps.append(gaps)
        rounds += 1
        if changed == 0:
            converged = 1
            break
        for j in range(k_eff):
            members = [s for s in act if assign[s] == j]
            if members:
                cu[j] = [sum(u[s][x] for s in members) / len(members) for x in range(B)]
                cv[j] = [sum(v[s][x] for s in members) / len(members) for x in range(B)]
    return KMeansExact(seeds, seed_gaps, round_gaps, assign, dist, rounds, converged)


def planted_buffer(B, S, k, seed, spread=1 << 10, top=1 << 34):
    """a sample mass buffer in which sample s belongs to cluster s mod k: nearly all of its mass (about `top`) on that cluster's home
    branch -- the homes are k distinct branches drawn at random -- and a little (below `spread` a branch) on about a tenth of the
    others.  Returns (buffer, homes)."""
    rng = np.random.default_rng(seed)
    W = 2 * B + 4
    homes = rng.choice(B, size=k, replace=False)
    m = np.zeros(S * W + 1, np.uint64)
    for s in range(S):
        mass = rng.integers(1, spread, B, dtype=np.uint64) * (rng.random(B) < 0.1)
        mass[homes[s % k]] = top + int(rng.integers(0, spread))
        m[s * W:s * W + B] = mass
    return m, homes


def same(got, want, centroids=True):
    """word for word: assign, the bits of dist, sizes, the bits of within, info and, when asked, the bits of the centroids"""
    ok = (np.asarray(got.assign).view(np.uint32) == want.assign).all() and (R.bits(got.dist) == R.bits(want.dist)).all()
    ok = ok and (np.asarray(got.sizes).view(np.uint32) == want.sizes).all() and (R.bits(got.within) == R.bits(want.within)).all()
    ok = ok and (np.asarray(got.info).view(np.uint32) == want.info).all()
    if centroids:
        ok = ok and (R.bits(got.centroids) == R.bits(want.centroids)).all()
    return bool(ok)
