"""The sample-level definitions of include/rappas_place.h restated in numpy and in exact rationals: clade sums of a sample mass
buffer and the pairwise KR distances, in the order of the sum the header fixes (np.cumsum and Python loops add one term after the
other; np.sum is pairwise and is not that order).  Also the trees and buffers the sample tests share."""
from fractions import Fraction

import numpy as np

KR_CHUNK = 2048


# ------------------------------------------------------------------------------------------------
# trees: parent arrays (-1 = root) and float32 lengths of the edges above the nodes
# ------------------------------------------------------------------------------------------------
def random_tree(B, seed, shuffle=True):
    """a random recursive tree of B nodes; shuffle: the ids relabelled at random, so that they are in no pre-order and the root is anywhere"""
    rng = np.random.default_rng(seed)
    parent = np.full(B, -1, np.int64)
    for x in range(1, B):
        parent[x] = rng.integers(max(0, x - 40), x) if rng.random() < 0.7 else rng.integers(0, x)
    bl = (rng.random(B) * 2).astype(np.float32)
    if shuffle:
        perm = rng.permutation(B)  # old id -> new id
        new_parent = np.full(B, -1, np.int64)
        new_parent[perm] = np.where(parent >= 0, perm[np.maximum(parent, 0)], -1)
        new_bl = np.zeros(B, np.float32)
        new_bl[perm] = bl
        parent, bl = new_parent, new_bl
    return parent.astype(np.int32), bl


def caterpillar(B, seed=0):
    """depth B - 1: node x hangs under x - 1"""
    rng = np.random.default_rng(seed)
    return np.arange(-1, B - 1, dtype=np.int32), (rng.random(B) + 0.25).astype(np.float32)


def star(B, seed=0):
    rng = np.random.default_rng(seed)
    parent = np.zeros(B, np.int32)
    parent[0] = -1
    return parent, (rng.random(B) + 0.25).astype(np.float32)


def sample_buffer(B, S, seed, fill=0.3, top=1 << 34):
    """a sample mass buffer (S * (2B + 4) + 1 words) with random masses on about `fill` of the branches; best and totals are filled
    with other numbers, which no sample-level call may read as masses"""
    rng = np.random.default_rng(seed)
    W = 2 * B + 4
    m = np.zeros(S * W + 1, np.uint64)
    for s in range(S):
        mass = rng.integers(1, top, B, dtype=np.uint64) * (rng.random(B) < fill)
        if not mass.any():
            mass[rng.integers(0, B)] = 1 << 30
        m[s * W:s * W + B] = mass
        m[s * W + B:s * W + W] = rng.integers(0, 1000, B + 4, dtype=np.uint64)
    m[-1] = 7
    return m


def special_buffer(B, S, seed):
    """S >= 5 samples: sample 1 empty, sample 3 a copy of sample 2, sample 4 with 2^62 on one branch"""
    m = sample_buffer(B, S, seed)
    W = 2 * B + 4
    m[1 * W:1 * W + B] = 0
    m[3 * W:3 * W + B] = m[2 * W:2 * W + B]
    m[4 * W:4 * W + B] = 0
    m[4 * W + (B // 2)] = 1 << 62
    m[4 * W + B - 1] += 12345
    return m


def check_special(D):
    S = D.shape[0]
    assert np.isnan(D[1]).all() and np.isnan(D[:, 1]).all()  # the empty sample: row, column, diagonal
    ok = np.array([s for s in range(S) if s != 1])
    assert not np.isnan(D[np.ix_(ok, ok)]).any()
    assert bits(D[2, 3]) == 0 and bits(D[3, 2]) == 0  # identical samples: +0.0
    assert (bits(D[ok, ok]) == 0).all()
    assert (bits(D) == bits(D.T)).all()


def masses_of(m, B, S):
    W = 2 * B + 4
    return np.stack([m[s * W:s * W + B] for s in range(S)])


# ------------------------------------------------------------------------------------------------
# the definitions
# ------------------------------------------------------------------------------------------------
def preorder(parent):
    """(root, the nodes in pre-order, children in ascending id)"""
    B = len(parent)
    kids = [[] for _ in range(B)]
    root = -1
    for x in range(B):
        if parent[x] < 0:
            root = x
        else:
            kids[parent[x]].append(x)
    order, stack = [], [root]
    while stack:
        x = stack.pop()
        order.append(x)
        stack.extend(reversed(kids[x]))
    assert len(order) == B
    return root, order


def clade_ref(parent, m, S):
    """uint64 [S, B]: the sum of the masses over every node's subtree (children hand their finished sums up)"""
    B = len(parent)
    _, order = preorder(parent)
    c = masses_of(m, B, S).copy()
    for x in reversed(order[1:]):
        c[:, parent[x]] += c[:, x]
    return c


def kr_ref(parent, bl, m, S):
    """float64 [S, S] as the header defines it, term by term and in its order"""
    B = len(parent)
    root, _ = preorder(parent)
    mass, c = masses_of(m, B, S), clade_ref(parent, m, S)
    h = np.asarray(bl, np.float32).astype(np.float64) * 0.5
    h[root] = 0.0
    with np.errstate(all="ignore"):
        T = c[:, root].astype(np.float64)
        u = c.astype(np.float64) / T[:, None]
        v = (c - mass).astype(np.float64) / T[:, None]
        D = np.zeros((S, S), np.float64)
        for s in range(S):
            for t in range(s, S):
                terms = np.empty(2 * B, np.float64)
                terms[0::2] = h * np.abs(u[s] - u[t])
                terms[1::2] = h * np.abs(v[s] - v[t])
                d = None
                for x0 in range(0, B, KR_CHUNK):
                    p = np.cumsum(np.concatenate([[0.0], terms[2 * x0:2 * (x0 + KR_CHUNK)]]))[-1]  # +0.0, then term after term
                    d = p if d is None else d + p
                D[s, t] = D[t, s] = d
    return D


def kr_exact(parent, bl, m, S):
    """[S][S] Fractions: the KR integral itself (no rounding anywhere); None where a sample is empty"""
    B = len(parent)
    root, _ = preorder(parent)
    mass, c = masses_of(m, B, S), clade_ref(parent, m, S)
    h = [Fraction(float(np.float32(bl[x]))) / 2 if x != root else Fraction(0) for x in range(B)]
    D = [[None] * S for _ in range(S)]
    for s in range(S):
        for t in range(S):
            Ts, Tt = int(c[s, root]), int(c[t, root])
            if Ts == 0 or Tt == 0:
                continue
            d = Fraction(0)
            for x in range(B):
                cs, ct, ms, mt = int(c[s, x]), int(c[t, x]), int(mass[s, x]), int(mass[t, x])
                d += h[x] * abs(Fraction(cs, Ts) - Fraction(ct, Tt)) + h[x] * abs(Fraction(cs - ms, Ts) - Fraction(ct - mt, Tt))
            D[s][t] = d
    return D


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
