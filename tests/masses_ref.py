"""The numpy reference of the edge masses (include/rappas_place.h) and the hand-made result sets the host and the
GPU tests share.  A direct restatement of the definition with np.add.at on uint64; nothing here comes from the engine.

A mass buffer of a tree of B branches is 2 * B + 4 uint64 words: mass_q30[B] | best[B] | sum w | sum w over reads with a counted
row | sum w * counted rows | rows skipped for a branch id >= B.  uint64 arithmetic wraps modulo 2^64, as the engine's does."""
from types import SimpleNamespace

import numpy as np


def q30(l):
    """q(l) = rint(min(l, 1) * 2^30) for l >= 0 (ties to even), 0 for negatives and NaN"""
    l = np.asarray(l, np.float64)
    with np.errstate(invalid="ignore"):
        q = np.rint(np.minimum(l, 1.0) * 2.0 ** 30)
        ok = l >= 0
    return np.where(ok, q, 0.0).astype(np.uint64)


def masses_ref(B, n_rows, branch, lwr, weights=None, masses=None):
    n_rows = np.asarray(n_rows, np.uint8)
    n = n_rows.shape[0]
    branch = np.asarray(branch, np.uint16).reshape(n, -1) if n else np.zeros((0, 1), np.uint16)
    K = branch.shape[1]
    lwr = np.asarray(lwr, np.float64).reshape(n, K) if n else np.zeros((0, 1), np.float64)
    m = np.zeros(2 * B + 4, np.uint64) if masses is None else np.array(masses, dtype=np.uint64)
    w = np.ones(n, np.uint64) if weights is None else np.asarray(weights, np.uint32).astype(np.uint64)
    rows = np.minimum(n_rows.astype(np.int64), K)
    valid = np.arange(K)[None, :] < rows[:, None]
    inside = branch.astype(np.int64) < B
    counted, skipped = valid & inside, valid & ~inside
    W = np.broadcast_to(w[:, None], (n, K))
    np.add.at(m, branch[counted].astype(np.int64), (W * q30(lwr))[counted])
    first = counted[:, 0]
    np.add.at(m, B + branch[first, 0].astype(np.int64), w[first])
    cnt = counted.sum(axis=1).astype(np.uint64)
    m[2 * B + 0] += w.sum(dtype=np.uint64)
    m[2 * B + 1] += w[cnt > 0].sum(dtype=np.uint64)
    m[2 * B + 2] += (w * cnt).sum(dtype=np.uint64)
    m[2 * B + 3] += np.uint64(skipped.sum())
    return m


# LWRs every set carries: 0, 1, just above 1 (clipped), -0.0, a negative, NaN, and products with 2^30 that end in exactly .5
# (0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 12345.5 -> 12346, 12346.5 -> 12346: ties to even)
SPECIAL_LWR = np.array([0.0, 1.0, 1.0 + 2.0 ** -52, -0.0, -0.25, np.nan, 0.5 / 2 ** 30, 1.5 / 2 ** 30, 2.5 / 2 ** 30, 12345.5 / 2 ** 30,
                        12346.5 / 2 ** 30, 2.0, np.inf, -np.inf], np.float64)
SPECIAL_Q30 = np.array([0, 2 ** 30, 2 ** 30, 0, 0, 0, 0, 2, 2, 12346, 12346, 2 ** 30, 2 ** 30, 0], np.uint64)


def make_set(B, K, n, seed=0, shape="mixed"):
    """a hand-made result set (n_rows u8 [n], branch u16 [n, K], lwr f64 [n, K]) as a namespace.
    "mixed": random branches below B (the K rows of a read distinct where B allows), n_rows 0 .. K + 3 (beyond K: clipped), about one
    read in eight with n_rows == 0; behind n_rows garbage (branch ids at or above B, NaN / huge LWRs); planted every few reads: branch
    B - 1, a branch >= B in row 0, a branch >= B in a later row, the special LWRs.
    "one_branch": every row of every read on one branch with LWR 0.5 and n_rows == K: the contention case, sum known in closed form."""
    rng = np.random.default_rng([seed, B, K, n])
    if shape == "one_branch":
        x = min(B - 1, 7)
        return SimpleNamespace(n_rows=np.full(n, K, np.uint8), branch=np.full((n, K), x, np.uint16), lwr=np.full((n, K), 0.5, np.float64))
    n_rows = rng.integers(0, K + 4, n).astype(np.uint8)
    n_rows[rng.random(n) < 0.125] = 0
    branch = ((rng.integers(0, B, n)[:, None] + np.arange(K)[None, :] * max(1, B // 17)) % B).astype(np.uint16)
    lwr = rng.random((n, K))
    lwr[rng.random((n, K)) < 0.2] *= 1e-6
    sp = rng.random((n, K)) < 0.15
    lwr[sp] = SPECIAL_LWR[rng.integers(0, len(SPECIAL_LWR), int(sp.sum()))]
    r = np.arange(n)
    branch[r % 5 == 1, 0] = B - 1
    if B < 65535:  # (ids are 16 bits: with B = 65535 the only id at or above B is 0xFFFF)
        branch[r % 11 == 3, 0] = min(B + (seed % 3), 65535)
        branch[r % 7 == 2, K - 1] = 65535
    else:
        branch[r % 11 == 3, 0] = 65535
        branch[r % 7 == 2, K - 1] = 65535
    behind = np.arange(K)[None, :] >= n_rows[:, None].astype(np.int64)
    g = int(behind.sum())
    branch[behind] = rng.choice(np.array([0xFFFF, min(B, 65535), 0, B - 1], np.uint16), g)
    lwr[behind] = rng.choice(np.array([np.nan, 1e300, 0.75, -1.0]), g)
    return SimpleNamespace(n_rows=n_rows, branch=branch, lwr=lwr)


def make_weights(n, kind, seed=0):
    """None | "zero" | "one" | "max" (2^32 - 1 each) | "mixed" (those three and random ones)"""
    if kind is None:
        return None
    if kind == "zero":
        return np.zeros(n, np.uint32)
    if kind == "one":
        return np.ones(n, np.uint32)
    if kind == "max":
        return np.full(n, 2 ** 32 - 1, np.uint32)
    rng = np.random.default_rng([seed, n, 77])
    w = rng.integers(0, 1000, n).astype(np.uint32)
    pick = rng.integers(0, 8, n)
    w[pick == 0] = 0
    w[pick == 1] = 1
    w[pick == 2] = 2 ** 32 - 1
    return w


def concat(a, b):
    return SimpleNamespace(n_rows=np.concatenate([a.n_rows, b.n_rows]), branch=np.concatenate([a.branch, b.branch]), lwr=np.concatenate([a.lwr, b.lwr]))
