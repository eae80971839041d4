"""The edge statistics of include/rappas_place.h (edge dispersion and edge correlation) restated in numpy: the
profiles from the integers, the lane rule spelled out (one rounded add after the other, the rows of all edges side by side), the ranks
by brute-force counting of `<` and `==`, and the finish.  Python integers and elementwise float64 operations only: np.sum is pairwise
and is not the order of the definition."""
import numpy as np

from tests import kr_ref as R

NAN_BITS = 0x7FF8000000000000
FIXED = 8


def out_words(B, F):
    return B * (6 + 4 * F) + 3 * F


def lane_sum(terms):
    """LS over the last axis of float64 [rows, S] terms that are already rounded: 64 lane partials, each sequential over s = l, l + 64,
    ... from +0.0, folded in lane order from +0.0"""
    rows, S = terms.shape
    r = np.zeros(rows)
    for l in range(64):
        p = np.zeros(rows)
        for s in range(l, S, 64):
            p = p + terms[:, s]
        r = r + p
    return r


def rank_devs(a, active):
    """int64 [rows, S]: d = rank2 - (n + 1) for the active entries of every row, 0 for the others; rank2 = 2 * #less + #equal + 1 by
    counting over the active entries"""
    rows, S = a.shape
    n = int(active.sum())
    d = np.zeros((rows, S), np.int64)
    if n == 0:
        return d
    v = a[:, active]                      # [rows, n]
    step = max(1, (1 << 24) // (n * n))   # rows a block, so that the comparison cube stays small
    for r0 in range(0, rows, step):
        w = v[r0:r0 + step]
        below = w[:, None, :] < w[:, :, None]  # [row, i, j]: a[j] < a[i]
        less = below.sum(axis=2)
        equal = n - less - below.sum(axis=1)   # (the entries above a[j] are the i it lies below; no NaN among them)
        d[r0:r0 + step][:, active] = 2 * less + equal + 1 - (n + 1)
    return d


def profiles(parent, m, S):
    """(P0, P1, active): float64 [B, S] mass share and imbalance, +0.0 for the root and for a sample without mass; bool [S]"""
    B = len(parent)
    root, _ = R.preorder(parent)
    mass, c = R.masses_of(m, B, S), R.clade_ref(parent, m, S)
    T = c[:, root]
    active = T != 0
    with np.errstate(all="ignore"):
        Tf = T.astype(np.float64)[:, None]
        P0 = mass.astype(np.float64) / Tf
        u, v = c.astype(np.float64) / Tf, (c - mass).astype(np.float64) / Tf
        P1 = (u + v) - 1.0
    for P in (P0, P1):
        P[~active] = 0.0
        P[:, root] = 0.0
    return np.ascontiguousarray(P0.T), np.ascontiguousarray(P1.T), active


def moments(a, active, n):
    """(mean, c, ss) of float64 [rows, S] whose inactive entries count as +0.0"""
    a0 = np.where(active[None, :], a, 0.0)
    with np.errstate(all="ignore"):
        mean = lane_sum(a0) / np.float64(n)
        c = np.where(active[None, :], a - mean[:, None], 0.0)
        ss = lane_sum(c * c)
    return mean, c, ss


def edgestat_ref(parent, m, S, meta=None):
    """(raw uint64 [B * (6 + 4F) + 3F], info uint32 [2]) as the header defines them"""
    B = len(parent)
    meta = np.zeros((0, S)) if meta is None else np.asarray(meta, np.float64).reshape(-1, S)
    F = meta.shape[0]
    RW = 6 + 4 * F
    raw = np.zeros(out_words(B, F), np.uint64)
    P0, P1, active = profiles(parent, m, S)
    n = int(active.sum())
    info = np.array([n, 0], np.uint32)
    if n == 0:
        return raw, info
    rows, feat = raw[:B * RW].reshape(B, RW), raw[B * RW:].reshape(F, 3)
    usable = [bool(np.isfinite(meta[f][active]).all()) for f in range(F)]
    info[1] = sum(1 << f for f in range(F) if not usable[f])
    gc, gd = np.zeros((F, S)), np.zeros((F, S), np.int64)
    for f in range(F):
        if not usable[f]:
            feat[f] = (NAN_BITS, NAN_BITS, 0)
            continue
        g = meta[f][None, :]
        mean, c, ss = moments(g, active, n)
        gc[f], gd[f] = c[0], rank_devs(np.where(active, g, 0.0), active)[0]
        feat[f] = (R.bits(mean)[0], R.bits(ss)[0], np.uint64(int((gd[f] * gd[f]).sum())))
    for q, P in enumerate((P0, P1)):
        mean, c, ss = moments(P, active, n)
        d = rank_devs(P, active)
        rows[:, 3 * q], rows[:, 3 * q + 1] = R.bits(mean), R.bits(ss)
        rows[:, 3 * q + 2] = (d * d).sum(axis=1).astype(np.uint64)
        for f in range(F):
            at = 6 + 4 * f + 2 * q
            if not usable[f]:
                rows[:, at], rows[:, at + 1] = NAN_BITS, 0
                continue
            with np.errstate(all="ignore"):
                rows[:, at] = R.bits(lane_sum(c * gc[f][None, :]))
            rows[:, at + 1] = (d * gd[f][None, :]).sum(axis=1).view(np.uint64)
    return raw, info


def finish_ref(B, raw, info):
    """(table float64 [B, 8 + 4F], feature_table float64 [F, 2]): the Finish, one rounding an operation"""
    raw = np.asarray(raw).view(np.uint64)
    F = (len(raw) - 6 * B) // (4 * B + 3)
    RW = 6 + 4 * F
    table, ftab = np.full((B, FIXED + 4 * F), np.nan), np.full((F, 2), np.nan)
    n = int(info[0])
    if n == 0:
        return table, ftab
    rows, feat = raw[:B * RW].reshape(B, RW), raw[B * RW:].reshape(F, 3)
    dbl, i64 = (lambda w: np.ascontiguousarray(w).view(np.float64)), (lambda w: np.ascontiguousarray(w).view(np.int64).astype(np.float64))
    nf = np.float64(n)
    with np.errstate(all="ignore"):
        for f in range(F):
            ftab[f] = (dbl(feat[f, 0:1])[0], dbl(feat[f, 1:2])[0] / nf)
        for q in range(2):
            mean, ss, rss = dbl(rows[:, 3 * q]), dbl(rows[:, 3 * q + 1]), i64(rows[:, 3 * q + 2])
            var = ss / nf
            sd = np.sqrt(var)
            table[:, 5 * q], table[:, 5 * q + 1], table[:, 5 * q + 2] = mean, var, sd
            if q == 0:
                table[:, 3], table[:, 4] = sd / mean, var / mean
            for f in range(F):
                gss, grss = dbl(feat[f, 1:2])[0], i64(feat[f, 2:3])[0]
                at = 6 + 4 * f + 2 * q
                table[:, FIXED + 4 * f + 2 * q] = dbl(rows[:, at]) / np.sqrt(ss * gss)
                table[:, FIXED + 4 * f + 2 * q + 1] = i64(rows[:, at + 1]) / np.sqrt(rss * grss)
    return table, ftab


def same_table(a, b):
    """two finished tables bit for bit, every NaN taken as one value"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((R.bits(a) == R.bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------------------------------------
# what the host and the device tests share
# ------------------------------------------------------------------------------------------------
def shapes(cross):
    """(B, S, F) of the word-for-word tests: S on both sides of a wave, of the crossover between the two ranking forms (`cross`), of the
    powers of two the sort pads to, and the limits; B odd and even, on both sides of the two edges a block of the counting form takes"""
    return [(1, 1, 0), (2, 3, 1), (3, 5, 1), (255, 2, 2), (257, 64, 8), (257, 65, 8), (2049, 130, 3), (300, cross, 1), (300, cross + 1, 1),
            (40, 1024, 2), (40, 1025, 2), (7, 4095, 8), (40, 4096, 2)]


def metadata(S, F, seed):
    """float64 [F, S]: a plain column, one of few repeated values, one negative throughout, one spread up to 1e100 in both signs, then
    plain ones again"""
    rng = np.random.default_rng(seed)
    cols = []
    for f in range(F):
        kind = f % 4
        if kind == 0:
            cols.append(rng.normal(size=S))
        elif kind == 1:
            cols.append(rng.integers(0, 4, S).astype(np.float64))
        elif kind == 2:
            cols.append(-rng.random(S) * 50 - 1)
        else:
            cols.append(np.where(rng.random(S) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-100, 100, S))
    return np.array(cols, np.float64).reshape(F, S)


def sparse_buffer(B, S, seed):
    """a sample mass buffer in which nine edges in ten are zero in nine samples in ten: long tie runs in every row"""
    rng = np.random.default_rng(seed)
    m = R.sample_buffer(B, S, seed, fill=1.0)
    W = 2 * B + 4
    quiet_edge, quiet_sample = rng.random(B) < 0.9, rng.random(S) < 0.9
    for s in range(S):
        if quiet_sample[s]:
            row = m[s * W:s * W + B]
            keep = int(np.argmax(row))
            row[quiet_edge] = 0
            if not row.any():
                row[keep] = 1 << 20
    return m
