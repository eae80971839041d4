"""The squash clustering of include/rappas_place.h restated in numpy, in the order of the sum tests/kr_ref.py fixes for a pair, and
in exact rationals (with the gap between the best and the second-best distance of every step, so that a test can tell whether the
order of the merges is decided).  Trees, buffers and the clade sums come from tests/kr_ref.py."""
from fractions import Fraction

import numpy as np

from tests import kr_ref as R

SQUASH_MERGE = np.dtype([("a", "<u4"), ("b", "<u4"), ("size", "<u4"), ("reserved", "<u4"), ("distance", "<f8")])
NONE = 0xFFFFFFFF


def pair_ref(h, us, vs, ut, vt):
    """the KR pair sum: +0.0, then term after term in ascending id, a partial per KR_CHUNK ids, the partials added in chunk order"""
    B = len(h)
    terms = np.empty(2 * B, np.float64)
    terms[0::2] = h * np.abs(us - ut)
    terms[1::2] = h * np.abs(vs - vt)
    d = None
    for x0 in range(0, B, R.KR_CHUNK):
        p = np.cumsum(np.concatenate([[0.0], terms[2 * x0:2 * (x0 + R.KR_CHUNK)]]))[-1]
        d = p if d is None else d + p
    return d


def pick(D, active):
    """the active pair a < b with the smallest D[a][b]: plain <, rows and columns ascending, so ties go to the smaller a, then b"""
    best = None
    S = len(active)
    for a in range(S):
        if not active[a]:
            continue
        for b in range(a + 1, S):
            if active[b] and (best is None or D[a][b] < best[0]):
                best = (D[a][b], a, b)
    return best


def squash_ref(parent, bl, m, S):
    """(merges SQUASH_MERGE [S - 1], n_merges) as the header defines them, operation by operation in binary64"""
    B = len(parent)
    root, _ = R.preorder(parent)
    mass, c = R.masses_of(m, B, S), R.clade_ref(parent, m, S)
    h = np.asarray(bl, np.float32).astype(np.float64) * 0.5
    h[root] = 0.0
    merges = np.zeros(S - 1, SQUASH_MERGE)
    merges["a"] = merges["b"] = NONE
    with np.errstate(all="ignore"):
        T = c[:, root].astype(np.float64)
        u = c.astype(np.float64) / T[:, None]
        v = (c - mass).astype(np.float64) / T[:, None]
        active = [int(c[s, root]) != 0 for s in range(S)]
        D = np.full((S, S), np.nan)
        for s in range(S):
            for t in range(s + 1, S):
                if active[s] and active[t]:
                    D[s, t] = D[t, s] = pair_ref(h, u[s], v[s], u[t], v[t])
        size = [1] * S
        n = 0
        while True:
            best = pick(D, active)
            if best is None:
                break
            d, a, b = best
            wa, wb, w = np.float64(size[a]), np.float64(size[b]), np.float64(size[a] + size[b])
            u[a] = (wa * u[a] + wb * u[b]) / w
            v[a] = (wa * v[a] + wb * v[b]) / w
            size[a] += size[b]
            active[b] = False
            merges[n] = (a, b, size[a], 0, d)
            n += 1
            for t in range(S):
                if active[t] and t != a:
                    D[a, t] = D[t, a] = pair_ref(h, u[a], v[a], u[t], v[t])
    return merges, n


def squash_exact(parent, bl, m, S):
    """the same run without rounding: a list of (a, b, size, distance, second) per merge, distance and second (the second-best
    distance of that step in the (distance, a, b) order, None when the step had one pair only) as Fractions"""
    B = len(parent)
    root, _ = R.preorder(parent)
    mass, c = R.masses_of(m, B, S), R.clade_ref(parent, m, S)
    h = [Fraction(float(np.float32(bl[x]))) / 2 if x != root else Fraction(0) for x in range(B)]
    active = [int(c[s, root]) != 0 for s in range(S)]
    u = [[Fraction(int(c[s, x]), int(c[s, root])) for x in range(B)] if active[s] else None for s in range(S)]
    v = [[Fraction(int(c[s, x]) - int(mass[s, x]), int(c[s, root])) for x in range(B)] if active[s] else None for s in range(S)]

    def dist(s, t):
        return sum(h[x] * (abs(u[s][x] - u[t][x]) + abs(v[s][x] - v[t][x])) for x in range(B))

    D = [[None] * S for _ in range(S)]
    for s in range(S):
        for t in range(s + 1, S):
            if active[s] and active[t]:
                D[s][t] = D[t][s] = dist(s, t)
    size = [1] * S
    rows = []
    while True:
        cands = sorted((D[a][b], a, b) for a in range(S) for b in range(a + 1, S) if active[a] and active[b])
        if not cands:
            break
        d, a, b = cands[0]
        na, nb = size[a], size[b]
        u[a] = [(na * u[a][x] + nb * u[b][x]) / (na + nb) for x in range(B)]
        v[a] = [(na * v[a][x] + nb * v[b][x]) / (na + nb) for x in range(B)]
        size[a] += nb
        active[b] = False
        rows.append((a, b, size[a], d, cands[1][0] if len(cands) > 1 else None))
        for t in range(S):
            if active[t] and t != a:
                D[a][t] = D[t][a] = dist(a, t)
    return rows


def same_rows(got, want):
    """word for word: the 24 bytes of every row"""
    g = np.ascontiguousarray(got).view(np.uint8)
    w = np.ascontiguousarray(want).view(np.uint8)
    return g.shape == w.shape and bool((g == w).all())
