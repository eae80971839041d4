"""Planted sample buffers full of replicates, and their census: what ties they hold by construction.  Real pooled runs are full of
technical replicates and of samples of a read or two on the same edge; their mass vectors are multiples of one another, and a
multiple by a power of two gives the same bits in the profiles U, V (the conversion to binary64 and the division commute with it).
Every selection step of the sample calls then runs on ties.  The census counts them from the labels alone -- lower bounds, no
engine and no restatement --, so that a test which relies on a kind of tie can assert that the family still holds it.
Trees come from tests/kr_ref.py; star_singletons brings its own."""
import numpy as np

PICK_THREADS, PICK_BLOCKS = 256, 512   # squash_pick_kernel: thread (b - a - 1) mod 256 of block a mod min(S - 1, 512)
ORTH_THREADS = 256                     # epca_orth_kernel: entry s is looked at by thread s mod 256
FACTORS = (1, 2, 4)


def replicate_buffer(B, S, n_profiles, layout, seed, empties=(), triple=True):
    """(buffer, labels): n_profiles random mass vectors, drawn as kr_ref.sample_buffer draws them; sample s is a copy of profile
    label[s] times 1, 2 or 4 (by turns among the copies of a profile), so all copies of a profile have bit-identical U and V from
    different integers.  layout "interleaved": label[s] = s mod n_profiles -- tied pairs differ in a and in b, far apart --,
    "blocked": label[s] = s * n_profiles // S -- copies next to each other.  The samples in `empties` have no mass (label -1).
    triple: profile 0 is drawn with masses up to 2^52, so that its clade sums pass 2^53 and round on conversion, and its last copy
    is times 3: a near-tie -- equal or an ulp apart entry by entry -- with its exact copies (label stays 0; near[s] tells, see
    census).  Needs at least three copies of profile 0."""
    assert layout in ("interleaved", "blocked") and 1 <= n_profiles <= S
    rng = np.random.default_rng(seed)
    W = 2 * B + 4
    prof = []
    for p in range(n_profiles):
        top = 1 << 52 if triple and p == 0 else 1 << 34
        mass = rng.integers(1, top, B, dtype=np.uint64) * (rng.random(B) < 0.3)
        if not mass.any():
            mass[rng.integers(0, B)] = 1 << 30
        prof.append(mass)
    labels = np.array([s % n_profiles if layout == "interleaved" else s * n_profiles // S for s in range(S)], np.int64)
    labels[list(empties)] = -1
    m = np.zeros(S * W + 1, np.uint64)
    seen = [0] * n_profiles
    last0 = int(np.nonzero(labels == 0)[0][-1]) if triple else -1
    if triple:
        assert np.count_nonzero(labels == 0) >= 3
    for s in range(S):
        m[s * W + B:s * W + W] = rng.integers(0, 1000, B + 4, dtype=np.uint64)  # best and totals: no sample-level call reads them as masses
        if labels[s] < 0:
            continue
        f = 3 if s == last0 else FACTORS[seen[labels[s]] % 3]
        seen[labels[s]] += 1
        m[s * W:s * W + B] = prof[labels[s]] * np.uint64(f)
    m[-1] = 7
    return m, labels


def near_sample(labels, triple=True):
    """the times-3 copy of replicate_buffer: the last sample of profile 0 (None without one)"""
    return int(np.nonzero(np.asarray(labels) == 0)[0][-1]) if triple else None


def star_singletons(S, seed, only=None):
    """(parent, bl, buffer): a star of S + 1 nodes (node 0 the root) with one float32 length on every leaf edge; sample s has all its
    mass, a different integer each, on leaf 1 + s.  All samples are distinct and every pair is at the same distance exactly: two
    half lengths, twice (u differs by 1 on two leaves, v nowhere), which is the length, with no rounding in any order of the sum.
    only: the samples that keep their mass.  Two of them, a < b, make an edge-PCA matrix that is exact: Xc is +0.5 / -0.5 on their two
    leaves and 0 elsewhere, G = [[0.5, -0.5], [-0.5, 0.5]] on them, so the first product has Y[0][b] == -Y[0][a] bit for bit: a pivot
    tie of opposite signs, which only the smallest-index rule decides (q[a] = +1.0, q[b] = -1.0)."""
    rng = np.random.default_rng(seed)
    B = S + 1
    parent = np.zeros(B, np.int32)
    parent[0] = -1
    bl = np.full(B, np.float32(0.25 + rng.random()), np.float32)
    W = 2 * B + 4
    m = np.zeros(S * W + 1, np.uint64)
    mass = rng.permutation(S).astype(np.uint64) + np.uint64(1)
    for s in range(S) if only is None else only:
        m[s * W + 1 + s] = mass[s]
    return parent, bl, m


def star_labels(S):
    return np.arange(S, dtype=np.int64)


def rank_families():
    """the edge-PCA families: (name, B, S, n_profiles, layout, empties, planted rank) -- r distinct profiles give a centred matrix of
    rank r - 1.  rank 0 with 2 and 4 identical active samples (their mean is themselves: G == 0 exactly), 2 among empties, 3
    identical ones (the mean of three rounds: G is rounding noise, g * 1 1^T), rank 1 and rank 2"""
    return [("rank0-n2", 300, 2, 1, "blocked", (), 0), ("rank0-n4", 300, 4, 1, "blocked", (), 0), ("rank0-n2-of-5", 40, 5, 1, "blocked", (0, 2, 4), 0),
            ("noise-n3", 300, 3, 1, "blocked", (), 0), ("rank1-2x5", 300, 10, 2, "interleaved", (), 1), ("rank1-blocked-48", 40, 48, 2, "blocked", (5, 17), 1),
            ("rank2-3x4", 300, 12, 3, "interleaved", (), 2), ("rank2-blocked-47", 300, 47, 3, "blocked", (0, 46), 2)]


def dead_columns(G, S, k_eff):
    """the columns whose first product, G times the start vector, is all zero: by the definition they are zero columns for good (G
    times a zero column is zero), so the components sit in the columns that are left, in order.  The start vectors are affine in s
    between the wraps of the hash, and a G of few interleaved profiles can take such a vector to zero exactly."""
    from tests import epca_ref as E
    Q = np.array([[float(((s * 8 + j + 1) * 2654435761) % (1 << 32)) / 4294967296.0 - 0.5 for s in range(S)] for j in range(k_eff)])
    Y = E.multiply(G, Q)
    return tuple(j for j in range(k_eff) if not Y[j].any())


def check_epca_against_eigvalsh(f, raw, B, S, k, G, planted_rank, noise=False, dead=(), at_most=False, iters=None):
    """The finished output f (eigenvalue, share, residual, projection [S, k], loading [B, k]) of a raw output against
    numpy.linalg.eigvalsh of the restatement's G.  rank = the eigenvalues of G above 64 * S * 2^-53 of the largest -- the accuracy the
    eigenvalue test claims, so what is below it is no component --, which must be the planted rank (noise: G is the rounding of a
    zero matrix, g * 1 1^T with g <= 4 B 2^-106, of rank one by that count; its one eigenvalue is held to the same bars and to
    3 S B 2^-104; at_most: a random draw on a small tree may fall below the planted rank, which then only bounds it).  The
    components sit in the first `rank` columns that are not in `dead` (dead_columns), component after component:
      a component       min_i |eigenvalue_j - w_i| <= residual_j + 64 * S * 2^-53 * w_0 and residual_j <= 1e-12 * the first eigenvalue
      any other column  eigenvalue, share, residual, the projection column and the loading column are all +0.0
      the live loadings are unit and orthogonal to 1e-9; share_j is exactly eigenvalue_j / trace
    Returns the rank; prints each figure before it asserts."""
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    assert (bits(G) == bits(G.T)).all()
    w = np.linalg.eigvalsh(G)[::-1]
    bar = 64 * S * 2.0 ** -53 * w[0]
    rank = int(np.count_nonzero(w > bar)) if w[0] > 0 else 0
    print("eigvalsh", w[:4], "rank", rank, "planted", planted_rank, "dead", dead, "eigenvalue", f.eigenvalue, "share", f.share, "residual", f.residual)
    if noise:
        assert rank <= 1 and np.abs(G).max() <= 4 * B * 2.0 ** -106 and (f.eigenvalue <= 3 * S * B * 2.0 ** -104).all()
    elif at_most:
        assert rank <= planted_rank
    else:
        assert rank == planted_rank
    # iters: the residual bar only where that many iterations can have reached it (a power iteration gains w_i+1 / w_i a round)
    converged = iters is None or all((w[i + 1] / w[i]) ** iters <= 2.0 ** -53 for i in range(rank))
    live = [j for j in range(k) if j not in dead][:rank]
    trace = raw[0]
    for j in live:
        gap = np.abs(f.eigenvalue[j] - w).min()
        assert f.eigenvalue[j] > 0 and gap <= f.residual[j] + bar, (j, gap)
        assert not converged or f.residual[j] <= 1e-12 * f.eigenvalue[live[0]], j
        assert bits(f.share[j]) == bits(f.eigenvalue[j] / trace), j
    for j in range(k):
        if j not in live:
            for part in (f.eigenvalue[j], f.share[j], f.residual[j], f.projection[:, j], f.loading[:, j]):
                assert (bits(part) == 0).all(), (j, f.eigenvalue[j], f.share[j], f.residual[j])
    if live and converged:  # (the loadings of vectors that are not yet eigenvectors are not orthogonal)
        L =f.loading[:, live]
        assert np.abs(L.T @ L - np.eye(len(live))).max() <= 1e-9
    return rank


def census(labels, near=None, all_pairs_tie=False, k=None):
    """What ties the family holds by construction, as a dict of counts (lower bounds: the near copy is left out of every class).
    labels [S]: -1 = no mass; equal labels = bit-identical profiles; all_pairs_tie: the star, whose distinct samples are all at one
    distance.
      tied_pairs        the pairs a < b at the minimum distance of the first squash step (+0.0 between copies; every pair of the star)
      row_later_stride  those for which a tied pair (a, b') with b' <= b - 256 exists: the thread loop of the row comes to them in a later pass
      same_thread       those of them with b - b' a multiple of 256: the same thread meets both
      block_later_stride  those with a >= 512 whose block (a mod 512) has met a tied pair in an earlier row (S - 1 >= 512)
      blocks            the blocks that hold a tied pair
      seed_ties         the fewest samples that tie for a farthest-first seed while a class has no seed yet: the smallest class
                        (the star: every sample but the seeds so far, at least S - k + 1)
      equidistant       with k: the fewest samples at one distance from two centroids -- k above the number of distinct profiles
                        makes farthest-first take a second copy of a class, and every copy of that class is at +0.0 from both (the
                        star with k >= 2: every sample that is no seed, S - k)
      pivot_ties        the fewest entries of an edge-PCA column that tie for the pivot: bit-identical samples have bit-identical
                        rows of G, so the largest entry comes once per copy: the smallest class
      pivot_threads     the fewest threads (s mod 256) those copies sit in"""
    labels = np.asarray(labels)
    S = len(labels)
    cls = labels.copy()
    if near is not None:
        cls[near] = -2
    act = np.nonzero(cls >= 0)[0]
    a, b = np.triu_indices(S, 1)
    if all_pairs_tie:
        tie = (cls[a] >= 0) & (cls[b] >= 0)
    else:
        tie = (cls[a] >= 0) & (cls[a] == cls[b])
    a, b = a[tie], b[tie]
    n_blocks = min(S - 1, PICK_BLOCKS)
    row_later = same_thread = 0
    first_b, residues = {}, {}
    for x, y in zip(a.tolist(), b.tolist()):  # (ascending a, then b)
        if y - first_b.setdefault(x, y) >= PICK_THREADS:
            row_later += 1
            same_thread += y % PICK_THREADS in residues[x]  # (an earlier b of the row in the same thread is a multiple of 256 below)
        residues.setdefault(x, set()).add(y % PICK_THREADS)
    rows = set(a.tolist())
    block_later = sum(1 for x in a.tolist() if x >= n_blocks and x - n_blocks in rows)
    sizes = np.bincount(cls[act]) if len(act) else np.zeros(0, np.int64)
    sizes = sizes[sizes > 0]
    smallest = int(sizes.min()) if len(sizes) else 0
    out = dict(tied_pairs=len(a), row_later_stride=row_later, same_thread=int(same_thread), block_later_stride=block_later,
               blocks=len({x % n_blocks for x in rows}))
    n_distinct = len(sizes) + (near is not None)
    if all_pairs_tie:
        out.update(seed_ties=len(act) - (k or 1) + 1, equidistant=(len(act) - k if k and k >= 2 else 0), pivot_ties=0, pivot_threads=0)
    else:
        members = [np.nonzero(cls == c)[0] for c in np.unique(cls[act])]
        out.update(seed_ties=smallest if smallest >= 2 else 0, equidistant=(smallest if k and k > n_distinct and smallest >= 2 else 0),
                   pivot_ties=smallest if smallest >= 2 else 0,
                   pivot_threads=min((len({int(s) % ORTH_THREADS for s in mem}) for mem in members), default=0))
    return out
