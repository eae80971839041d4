"""The per-sample diversity measures of include/rappas_place.h restated in numpy: rk_log2 and rk_exp2 of rappas_amd/csrc/rk_divmath.h
operation by operation (every numpy operation below is one IEEE binary64 operation per element: no fused multiply-add, no pairwise
sum), the terms of a half-edge, and the order of the sum -- 256 lane partials per chunk of 2048 ids, folded by halving, the chunks in
order.  Also an exact evaluation in mpmath from the integers."""
import numpy as np

from tests.kr_ref import KR_CHUNK, clade_ref, masses_of, preorder

LANES = 256
FIXED = 5
NAN_BITS = 0x7FF8000000000000
SQRT2 = float.fromhex("0x1.6a09e667f3bcdp+0")
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
TWO_OVER_LN2 = float.fromhex("0x1.71547652b82fep+1")
FACTORIALS = [87178291200.0, 6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0]


def log2(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.uint64)
    e = ((b >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
    m = ((b & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    big = m > SQRT2
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    q = np.full(x.shape, 1.0 / 23.0)
    for d in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        q = q * z + 1.0 / d
    q = q * z
    r = s + s * q
    return e.astype(np.float64) + r * TWO_OVER_LN2


def exp2(y):
    y = np.ascontiguousarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        low = ~(y >= -1022.0)
        yy = np.where(low, 0.0, np.where(y > 1023.0, 1023.0, y))
        k = ((yy + 1024.0) + 0.5).astype(np.int64) - 1024
        t = (yy - k.astype(np.float64)) * LN2
        p = np.full(y.shape, 1.0 / FACTORIALS[0])
        for f in FACTORIALS[1:]:
            p = p * t + 1.0 / f
        p = p * t + 0.5
        p = p * t + 1.0
        p = p * t + 1.0
        scale = ((k + 1023).astype(np.uint64) << np.uint64(52)).view(np.float64)
        return np.where(low, 0.0, p * scale)


def pw(x, lg, theta):
    with np.errstate(all="ignore"):
        return np.where(x > 0.0, exp2(theta * lg), 1.0 if theta == 0.0 else 0.0)


def half_terms(a, T, h, theta):
    """[5 + 2 n_theta, n]: the terms of the half-edges with distal masses a (uint64 [n]) in a sample of total T != 0"""
    rooted, split = a > 0, (a > 0) & (a < np.uint64(T))
    with np.errstate(all="ignore"):
        D = a.astype(np.float64) / np.float64(np.uint64(T))
        E = 1.0 - D
        M = 2.0 * np.where(E < D, E, D)
        lgD, lgM = log2(D), log2(M)
        zero = np.zeros(a.shape, np.float64)
        rows = [np.where(rooted, h, zero), np.where(split, h, zero), np.where(split, h * M, zero), np.where(split, h * (D * E), zero),
                np.where(rooted, h * (-(D * lgD) * LN2), zero)]
        for th in theta:
            rows.append(np.where(rooted, h * pw(D, lgD, th), zero))
            rows.append(np.where(split, h * pw(M, lgM, th), zero))
    return np.stack(rows)


def diversity_ref(parent, bl, m, S, theta=()):
    """float64 [S, 5 + 2 n_theta] as the header defines it, term by term and in its order"""
    B = len(parent)
    theta = [float(t) for t in theta]
    C = FIXED + 2 * len(theta)
    root, _ = preorder(parent)
    mass, c = masses_of(m, B, S), clade_ref(parent, m, S)
    h = np.asarray(bl, np.float32).astype(np.float64) * 0.5
    h[root] = 0.0
    out = np.zeros((S, C), np.float64)
    for s in range(S):
        T = int(c[s, root])
        if T == 0:
            out[s].view(np.uint64)[:] = NAN_BITS
            continue
        prox, dist = half_terms(c[s], T, h, theta), half_terms(c[s] - mass[s], T, h, theta)
        for x0 in range(0, B, KR_CHUNK):
            n = min(KR_CHUNK, B - x0)
            # rows of 256 lanes; the ids a short chunk lacks are padded with +0.0, which leaves the bits of a sum that is never -0.0
            P, Q = np.zeros((C, KR_CHUNK)), np.zeros((C, KR_CHUNK))
            P[:, :n], Q[:, :n] = prox[:, x0:x0 + n], dist[:, x0:x0 + n]
            P, Q = P.reshape(C, KR_CHUNK // LANES, LANES), Q.reshape(C, KR_CHUNK // LANES, LANES)
            acc = np.zeros((C, LANES))
            for r in range((n + LANES - 1) // LANES):
                acc = (acc + P[:, r]) + Q[:, r]
            stride = LANES // 2
            while stride:
                acc = acc[:, :stride] + acc[:, stride:2 * stride]
                stride //= 2
            out[s] = acc[:, 0] if x0 == 0 else out[s] + acc[:, 0]
    return out


def diversity_exact(parent, bl, m, S, theta=()):
    """[S][5 + 2 n_theta] mpmath numbers at the working precision the caller set: the definition evaluated from the integers with
    exact logarithms and powers; None rows where a sample is empty"""
    import mpmath as mp
    B = len(parent)
    root, _ = preorder(parent)
    mass, c = masses_of(m, B, S), clade_ref(parent, m, S)
    h = [mp.mpf(float(np.float32(bl[x]))) / 2 if x != root else mp.mpf(0) for x in range(B)]
    rows = []
    for s in range(S):
        T = int(c[s, root])
        if T == 0:
            rows.append(None)
            continue
        row = [mp.mpf(0)] * (FIXED + 2 * len(theta))
        for x in range(B):
            for a in (int(c[s, x]), int(c[s, x]) - int(mass[s, x])):
                if a == 0 or h[x] == 0:
                    continue
                D = mp.mpf(a) / T
                row[0] += h[x]
                row[4] += h[x] * -(D * mp.log(D))
                for i, th in enumerate(theta):
                    row[FIXED + 2 * i] += h[x] * D ** mp.mpf(float(th))
                if a < T:
                    M = 2 * min(D, 1 - D)
                    row[1] += h[x]
                    row[2] += h[x] * M
                    row[3] += h[x] * D * (1 - D)
                    for i, th in enumerate(theta):
                        row[FIXED + 2 * i + 1] += h[x] * M ** mp.mpf(float(th))
        rows.append(row)
    return rows
