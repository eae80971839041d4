"""The edge-PCA definition of include/rappas_place.h (steps 1 - 8 and the finish) restated in numpy: node loops that add one outer
product after the other, explicit lane-rule loops, no np.sum and no np.dot anywhere.  Trees and buffers come from tests/kr_ref.py."""
import numpy as np

from tests import kr_ref as R

LANES = 64


def LS(F):
    """the lane rule along axis 0 of F [S, ...]: 64 sequential lane sums from +0.0 over s = l, l + 64, ..., then added in ascending lane
    order onto +0.0 (vectorised over the other axes: each of their entries is its own sum)"""
    F = np.asarray(F, np.float64)
    p = np.zeros((LANES,) + F.shape[1:], np.float64)
    for s in range(F.shape[0]):  # ascending s: every lane meets its own s in ascending order
        p[s % LANES] = p[s % LANES] + F[s]
    r = np.zeros(F.shape[1:], np.float64)
    for l in range(LANES):
        r = r + p[l]
    return r


def dot(a, b):
    return LS(a * b)


def out_doubles(B, S, k):
    return 1 + k * (3 + S + B)


def prepare(parent, bl, m, S):
    """steps 1 - 4, which depend on neither k nor iters: (B, S, n_active, Xc [B, S], G [S, S], trace)"""
    B = len(parent)
    root, _ = R.preorder(parent)
    mass, c = R.masses_of(m, B, S), R.clade_ref(parent, m, S)
    T = c[:, root]
    active = T != 0
    n = int(np.count_nonzero(active))
    if n < 2:
        return B, S, n, None, None, None
    with np.errstate(all="ignore"):
        u = c.astype(np.float64) / T.astype(np.float64)[:, None]
        v = (c - mass).astype(np.float64) / T.astype(np.float64)[:, None]
    live = active[None, :] & (np.arange(B) != root)[:, None]  # [B, S]
    X = np.where(live, ((u + v) - 1.0).T, 0.0)
    mean = LS(X.T) / float(n)
    Xc = np.where(live, X - mean[:, None], 0.0)
    G = None
    for x0 in range(0, B, R.KR_CHUNK):
        acc = np.zeros((S, S), np.float64)
        for x in range(x0, min(x0 + R.KR_CHUNK, B)):
            acc = acc + Xc[x][:, None] * Xc[x][None, :]
        G = acc if G is None else G + acc
    trace = LS(np.array([G[s, s] for s in range(S)]))
    return B, S, n, Xc, G, trace


def multiply(G, Q):
    """[k_eff, S]: out[j][s] = LS(t -> G[s][t] * Q[j][t])"""
    return LS(G.T[:, None, :] * Q.T[:, :, None])  # axis 0 is t; [t, j, s]


def largest(col):
    """(i, fabs(col[i])) for the smallest i with the largest fabs (plain >)"""
    i, best = 0, abs(col[0])
    for s in range(1, len(col)):
        if abs(col[s]) > best:
            i, best = s, abs(col[s])
    return i, best


def iterate(prep, k, iters, trace_to=None):
    """steps 5 - 8: (raw, info).  trace_to: a list that takes, for every column at its turn, (iteration, j, the projections the rule
    counts, its largest fabs, the scale it is measured against, whether it became a zero column)"""
    B, S, n, Xc, G, trace = prep
    raw = np.zeros(out_doubles(B, S, k), np.float64)
    k_eff = min(k, n - 1) if n >= 2 else 0
    info = np.array([n, k_eff], np.uint32)
    if k_eff == 0:
        return raw, info
    Q = np.empty((k_eff, S), np.float64)
    for j in range(k_eff):
        for s in range(S):
            Q[j, s] = float(((s * 8 + j + 1) * 2654435761) % (1 << 32)) / 4294967296.0 - 0.5
    noise = np.float64(S) * 2.0 ** -40  # the factor of step 6 for one projection (a power of two times S: exact)
    for it in range(iters):
        Y = multiply(G, Q)
        top0 = [largest(Y[j])[1] for j in range(k_eff)]  # as the product delivered the columns
        applied, scale = 0, np.float64(0.0)  # the live columns so far -- the projections a later column has been through -- and their largest top0
        for j in range(k_eff):
            i, best = largest(Y[j])
            against = top0[j] if top0[j] > scale else scale
            zero = best <= (noise * np.float64(applied if it else 0)) * against  # the zero rule, from the second iteration on; before it best == 0
            if trace_to is not None:
                trace_to.append((it, j, applied if it else 0, best, against, bool(zero)))
            if zero:
                Y[j] = 0.0
                continue
            applied += 1
            scale = against
            Y[j] = Y[j] / Y[j, i]
            nn = dot(Y[j], Y[j])
            for l in range(j + 1, k_eff):
                d = dot(Y[j], Y[l]) / nn
                Y[l] = Y[l] - d * Y[j]
        Q = Y
    Z = multiply(G, Q)
    lam, nn, rr = raw[1:1 + k], raw[1 + k:1 + 2 * k], raw[1 + 2 * k:1 + 3 * k]
    q_out = raw[1 + 3 * k:1 + 3 * k + k * S].reshape(k, S)
    w_out = raw[1 + 3 * k + k * S:].reshape(k, B)
    raw[0] = trace
    for j in range(k_eff):
        nn[j] = dot(Q[j], Q[j])
        if nn[j] == 0:
            nn[j] = 0.0
        else:
            lam[j] = dot(Q[j], Z[j]) / nn[j]
            r = Z[j] - lam[j] * Q[j]
            rr[j] = dot(r, r)
        q_out[j] = Q[j]
        w_out[j] = LS(Xc.T * Q[j][:, None])
    return raw, info


def epca_ref(parent, bl, m, S, k, iters):
    return iterate(prepare(parent, bl, m, S), k, iters)


def split(raw, B, S, k):
    """(trace, lambda [k], nn [k], rr [k], q [k, S], w [k, B]) of a raw output"""
    raw = np.asarray(raw)
    return (raw[0], raw[1:1 + k], raw[1 + k:1 + 2 * k], raw[1 + 2 * k:1 + 3 * k], raw[1 + 3 * k:1 + 3 * k + k * S].reshape(k, S),
            raw[1 + 3 * k + k * S:].reshape(k, B))


def finish_ref(B, S, k, raw):
    """the finish as a numpy restatement: (eigenvalue, share, residual, projection [S, k], loading [B, k])"""
    trace, lam, nn, rr, q, w = split(raw, B, S, k)
    on = (lam > 0) & (nn != 0)
    with np.errstate(all="ignore"):
        ev, share, res = np.where(on, lam, 0.0), np.where(on, lam / trace, 0.0), np.where(on, np.sqrt(rr / nn), 0.0)
        proj = np.where(on[None, :], q.T * np.sqrt(lam / nn)[None, :], 0.0)
        load = np.where(on[None, :], w.T / np.sqrt(lam * nn)[None, :], 0.0)
    return ev, share, res, proj, load


def planted_buffer(B=300, S=9, seed=5):
    """sample s belongs to group s mod 3; each group has a base mass of 2^28 .. 2^32 on B // 8 random branches; noise below 2^20 on
    30 % of the branches"""
    rng = np.random.default_rng(seed)
    W = 2 * B + 4
    m = np.zeros(S * W + 1, np.uint64)
    base = []
    for _ in range(3):
        g = np.zeros(B, np.uint64)
        g[rng.choice(B, B // 8, replace=False)] = rng.integers(1 << 28, 1 << 32, B // 8, dtype=np.uint64)
        base.append(g)
    for s in range(S):
        noise = rng.integers(0, 1 << 20, B, dtype=np.uint64) * (rng.random(B) < 0.3)
        m[s * W:s * W + B] = base[s % 3] + noise
    return m


def same(a, b):
    return a.shape == b.shape and bool((R.bits(a) == R.bits(b)).all())
