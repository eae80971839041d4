"""Planted "line trees": databases and reads whose score rows sit on, next to and on either side of the -308 line of the weigh stage
(weigh_and_store in rappas_amd/csrc/rk_kernels.hip; select_and_weigh in oracle/rappas_oracle.c), and the census of what a set of reads
holds -- shared by tests/test_gpu_weigh_planted.py (GPU) and tests/test_weigh_planted_shapes.py (no GPU).

The database threshold is T = log10(thr) = -5.5 and every row score is a multiple of 2**-15 in [T, 0).  A branch a read of Q k-mers
hits at v1, v2 ... scores Q * T + (v1 - T) + (v2 - T) + ...; the float32 ulp between 256 and 512 is 2**-15, so below 512 in magnitude
every partial sum is exact whatever the order, and Q = 56 puts a branch hit once at T on -308.0 itself, one hit at T + 2**-15 on the
next float towards 0, and Q = 57 with a hit at T + 5.5 - 2**-15 on the next float away from 0.  (At and beyond 512 the oracle's score
vector is the definition, as everywhere in the suite.)  Reads have their own lengths: Q is one of Q_ALL, i.e. Q * T = -5.5, -44,
-302.5, -308, -313.5, -396 and -775.5, and the reads are shuffled, so that neighbours in a wave differ in regime.

Two kinds of read: "planted" ones carry none to four of the planted keys (rows of planted.planted_db, whose branches pick the select
shapes and keep the routes of tests/test_gpu_tie_order.py on their kernels; the scores are redrawn here from the line palette), and
"genome" ones are cut from a stretch every k-mer of which is a key whose row holds one branch b* at -0.125 (as synth.make_clade_db's
reads pile up on a clade): b* ends hundreds above the branches such a read hits once.  A read's last symbol belongs to no key, so an
ambiguity code can replace it (planted.with_ambiguity_code)."""
import functools

import numpy as np

from rappas_amd import synth
from oracle import oracle as O
from tests import planted as P

T = np.float32(-5.5)
THR = np.float32(10 ** -5.5)
STEP = 2.0 ** -15
LINE = np.float32(-308.0)
LINE_ABOVE = np.nextafter(LINE, np.float32(0))      # -307.99997
LINE_BELOW = np.nextafter(LINE, np.float32(-np.inf))  # -308.00003
Q_ALL = (1, 8, 55, 56, 57, 72, 141)
KEEP_FACTORS = (0.0, 0.01, 0.5, 1.0)
K_NS, KF_NS = 7, 0.01  # the ns_bound triple is run at this keep_at_most and keep_factor
VANISH, BAND_HI = -330.0, -312.0  # score - best at or below VANISH: term and numerator are +0.0; the open band between is kept empty

# the kinds of planted row: one score everywhere (on the line, one float above it, the one that lands one float below it with Q = 57),
# scores next to the threshold, eighths (differences of exactly -1 and -2: keep_factor 0.01 against 10**-2), any multiple of 2**-15
FLAT_T, FLAT_ABOVE, FLAT_BELOW, NEAR_T, EIGHTHS, ANY = range(6)
MODES = (FLAT_T, FLAT_ABOVE, FLAT_BELOW, NEAR_T, EIGHTHS, EIGHTHS, ANY)
NEAR_PALETTE = np.array([0.0, STEP, 2 * STEP, 0.125, 1.0, 2.0]) + float(T)
EIGHTH_PALETTE = np.array([-0.125, -0.25, -1.0, -2.0, -3.0, -4.125, float(T)])
GENOME_PALETTE = np.array([0.0, STEP, 0.125, 0.5, 1.0]) + float(T)  # the other branches of a genome row
N_STRETCH = 8

#          name: (alphabet, k, branches, reads, seed, keyword arguments of planted.planted_db) -- sizes and keywords of planted.TREES
TREES = {
    "line999": (4, 10, 999, 600, 999, dict(stride=256, clades=True)),
    "lineaa399": (20, 5, 399, 600, 399, dict(stride=256, clades=True)),
    "line2801": (4, 10, 2801, 600, 2801, dict(stride=64, clades=True, window=704, hash_quads=(10, 11))),
    "line9001": (4, 10, 9001, 600, 9001, dict(stride=64, clades=True, window=504)),
    "linewg13301": (4, 10, 13301, 300, 13301, dict(stride=256, clades=True, min_row=330, max_row=470, short_rows=0.12)),
}

# (tree, routes of tests/test_gpu_tie_order.py: ROUTES, ambiguity modes of the "ascii" route) of tests/test_gpu_weigh_planted.py
ROUTES = {
    "line999": ("lanes0", "lanes8", "lanes32", "lanes64"),
    "lineaa399": ("lanes0", "lanes64"),
    "line2801": ("windowed", "sorted_always", "hash", "hash_small"),
    "line9001": ("sorted",),
    "linewg13301": ("wg1", "wg2"),
}
ASCII = {"line999": ("skip", "max", "mean")}


def Ks_of(route):
    return tuple(K for K in P.K_EDGES if K <= 8) if route == "lanes8" else P.K_EDGES


def dense_index(alphabet, digits):
    k = digits.shape[-1]
    return (digits.astype(np.uint64) * (np.uint64(alphabet) ** np.arange(k, dtype=np.uint64))).sum(-1).astype(np.uint64)


def line_db(alphabet, k, nb, seed, **kw):
    """the rows of planted.planted_db with scores redrawn from the line palette, and the rows of N_STRETCH genome stretches.
    -> (database, digits of the planted keys, their row kinds, their row lengths, the stretches' digits)"""
    base, digits = P.planted_db(alphabet, k, nb, 300, seed, **kw)
    rng = np.random.default_rng(seed + 7)
    off = base.row_offsets.astype(np.int64)
    n_keys = len(off) - 1
    modes = np.array([MODES[i % len(MODES)] for i in range(n_keys)])
    scores = np.empty(len(base.scores), np.float64)
    for i in range(n_keys):
        m = off[i + 1] - off[i]
        scores[off[i]:off[i + 1]] = {
            FLAT_T: lambda: np.full(m, float(T)), FLAT_ABOVE: lambda: np.full(m, float(T) + STEP), FLAT_BELOW: lambda: np.full(m, -STEP),
            NEAR_T: lambda: rng.choice(NEAR_PALETTE, m), EIGHTHS: lambda: rng.choice(EIGHTH_PALETTE, m),
            ANY: lambda: -STEP * rng.integers(1, int(5.5 / STEP) + 1, m)}[modes[i]]()
    # genome stretches: every k-mer a key; its row holds the stretch's b* at -0.125 and other branches next to the threshold
    longest = max(Q_ALL) if alphabet == 4 else 96
    while True:  # (drawn again until no k-mer of a stretch is a planted key or occurs twice)
        stretch = rng.integers(0, alphabet, (N_STRETCH, longest + k + 40))
        codes = [int(dense_index(alphabet, stretch[s, j:j + k])) for s in range(N_STRETCH) for j in range(stretch.shape[1] - k + 1)]
        if len(set(codes) | set(dense_index(alphabet, digits).tolist())) == len(codes) + len(digits):
            break
    lo, hi = max(2, kw.get("min_row", 1)), kw.get("max_row", 24)
    g_codes, g_b, g_s = [], [], []
    for s in range(N_STRETCH):
        b_star = int(rng.integers(1, nb))
        for j in range(stretch.shape[1] - k + 1):
            g_codes.append(dense_index(alphabet, stretch[s, j:j + k]))
            m = int(rng.integers(lo, hi + 1))
            others = rng.choice(np.setdiff1d(np.arange(1, nb), [b_star]), size=min(m - 1, nb - 2), replace=False)
            b = np.concatenate([[b_star], others])
            v = np.concatenate([[-0.125], rng.choice(GENOME_PALETTE, len(others))])
            order = np.argsort(b)
            g_b.append(b[order])
            g_s.append(v[order])
    dense = np.concatenate([dense_index(alphabet, digits), np.array(g_codes, np.uint64)])
    assert len(np.unique(dense)) == len(dense)  # (no k-mer of a stretch is a planted key or occurs twice)
    lens = np.concatenate([np.diff(off), [len(b) for b in g_b]])
    row_off = np.zeros(len(dense) + 1, np.uint64)
    np.cumsum(lens, out=row_off[1:])
    all_s = np.concatenate([scores] + g_s)
    assert (all_s >= float(T)).all() and (all_s < 0).all() and (all_s / STEP == np.round(all_s / STEP)).all()
    sdb = synth.SynthDB(alphabet, k, nb, THR, T, synth.dense_to_code(alphabet, k, dense), row_off,
                        np.concatenate([base.branch_ids] + g_b).astype(np.uint16), all_s.astype(np.float32), seed)
    return sdb, digits, modes, np.diff(off), stretch


def line_reads(alphabet, k, digits, modes, row_len, stretch, n, seed):
    """n reads by recipe, shuffled: 24 each that carry one key of a FLAT_T / FLAT_ABOVE row with Q = 56 and of a FLAT_BELOW row with
    Q = 57 (the three floats at the line, for every keep_at_most); 12 without a key; 25 with one key of a row of fewer than 7 entries; a
    quarter cut from the genome stretches; the rest with one to four keys anywhere.  -> (characters, offsets)"""
    rng = np.random.default_rng(seed)
    letters = synth.AA_LETTERS if alphabet == 20 else synth.DNA_LETTERS
    Qs = np.array([q for q in Q_ALL if q + k - 1 <= stretch.shape[1] - 40])
    p_q = np.array([{1: 0.06, 8: 0.12, 55: 0.2, 56: 0.22, 57: 0.16, 72: 0.12, 141: 0.12}[int(q)] for q in Qs])
    p_q = p_q / p_q.sum()

    def keys_of(mode, longer_than=1):
        return np.nonzero((modes == mode) & (row_len > longer_than))[0]

    recipes = []  # (Q, key indices) or (Q, -1: a genome read)
    for mode, q in ((FLAT_T, 56), (FLAT_ABOVE, 56), (FLAT_BELOW, 57)):
        recipes += [(q, [int(rng.choice(keys_of(mode)))]) for _ in range(24)]
    recipes += [(int(rng.choice(Qs)), []) for _ in range(12)]
    recipes += [(int(rng.choice(Qs, p=p_q)), [int(rng.choice(np.nonzero(row_len < 7)[0]))]) for _ in range(25)]
    g_q = Qs[Qs >= 55]
    recipes += [(int(g_q[i % len(g_q)]), -1) for i in range(n // 4)]
    while len(recipes) < n:
        q = int(rng.choice(Qs, p=p_q))
        room = max(1, min(4, (q + k - 2) // (k + 1)))
        recipes.append((q, rng.integers(0, len(digits), int(rng.integers(1, room + 1))).tolist()))
    reads = []
    for i in rng.permutation(n):
        q, keys = recipes[i]
        L = q + k - 1
        st = rng.integers(0, alphabet, L)
        if keys == -1:  # L - 1 symbols of a stretch, the last symbol belongs to no key of it
            s, at = int(rng.integers(0, N_STRETCH)), int(rng.integers(0, 40))
            st[:L - 1] = stretch[s, at:at + L - 1]
            st[L - 1] = (stretch[s, at + L - 1] + 1 + int(rng.integers(0, alphabet - 1))) % alphabet
        elif L == k:
            if keys:
                st[:] = digits[keys[0]]
        else:
            seg = (L - 1) // max(1, len(keys))  # a stretch of the read for each key; the read's last symbol belongs to none
            assert not keys or seg >= k, (L, keys)
            for j, key in enumerate(keys):
                at = j * seg + int(rng.integers(0, seg - k + 1))
                st[at:at + k] = digits[key]
        reads.append(letters[st])
    off = np.zeros(n + 1, np.uint64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return np.ascontiguousarray(np.concatenate(reads)), off


@functools.lru_cache(maxsize=None)
def tree(name):
    """(database, oracle database, reads, offsets, sorted score vectors) of a line tree, made once a process and left unchanged"""
    alphabet, k, nb, n_reads, seed, kw = TREES[name]
    sdb, digits, modes, row_len, stretch = line_db(alphabet, k, nb, seed, **kw)
    odb = O.OracleDB.from_synth(sdb)
    seq, off = line_reads(alphabet, k, digits, modes, row_len, stretch, n_reads, seed + 1)
    return sdb, odb, seq, off, P.sorted_vectors(odb, seq, off)


@functools.lru_cache(maxsize=None)
def ambiguous(name, amb):
    """the reads of a line tree with an ambiguity code for their last symbol, and their sorted score vectors in ambiguity mode amb"""
    from tests import golden_util as GU
    sdb, odb, seq, off, _ = tree(name)
    seq = P.with_ambiguity_code(sdb.alphabet, seq, off)
    return seq, P.sorted_vectors(odb, seq, off, GU.AMB[amb])


def vectors_of(name, amb=None):
    return tree(name)[4] if amb is None else ambiguous(name, amb)[1]


@functools.lru_cache(maxsize=None)
def oracle_place(name, K, keep_factor, amb=None, ns_bound=float("-inf")):
    from tests import golden_util as GU
    sdb, odb, seq, off, _ = tree(name)
    if amb is not None:
        seq, _ = ambiguous(name, amb)
    return odb.place(seq, off, keep_at_most=K, keep_factor=keep_factor, amb_mode=GU.AMB[amb or "mean"], ns_bound=ns_bound)


def calls(name, amb=None):
    """(keep_at_most, keep_factor, ns_bound) of every call tests/test_gpu_weigh_planted.py makes on a tree"""
    return [(K, kf, float("-inf")) for K in P.K_EDGES for kf in KEEP_FACTORS] + [(K_NS, KF_NS, b) for b in ns_bounds(vectors_of(name, amb))]


@functools.lru_cache(maxsize=None)
def reference(name, amb, K, keep_factor, ns_bound):
    """tests/weigh_ref.py on every read of a tree: (n_rows [n], LWR [n, K] with 0.0 beyond n_rows, BELOW_NSBOUND [n], the smallest
    relative margin of a cut decision)"""
    from tests import weigh_ref as WR
    vectors = vectors_of(name, amb)
    n_rows, lwr, below, closest = np.zeros(len(vectors), np.int64), np.zeros((len(vectors), K)), np.zeros(len(vectors), bool), 1.0
    for r, (order, bits) in enumerate(vectors):
        n_rows[r], rows, below[r], margin = WR.weigh(bits[:K].view(np.float32), keep_factor, ns_bound)
        lwr[r, :n_rows[r]] = rows
        closest = closest if margin is None else min(closest, margin)
    return n_rows, lwr, below, closest


# ---- the census ----
COUNTS = ["plain", "deep", "straddle", "edge_at", "edge_above", "edge_below", "edge_above_subnormal", "fewer", "none", "vanish", "band",
          "tied_best", "mixed_wave"]


def census(vectors, K):
    """what the reads hold for keep_at_most K; lowest and best are those of the first numBest = min(K, touched) entries of the sorted
    score vector.  edge_above_subnormal: lowest is the float above the line and 10**best < 2.3e-308 too, so that every term of the
    unshifted sum lies below the smallest normal binary64.  band: reads with a difference score - best inside (VANISH, BAND_HI) among
    their first 16 scores (must stay 0).  mixed_wave: aligned groups of four consecutive reads -- one wave of 16-lane groups -- that
    hold a shifted and an unshifted read."""
    seen = dict.fromkeys(COUNTS, 0)
    regime = []  # per read: 1 shifted, 0 unshifted, -1 nothing touched
    for order, bits in vectors:
        if len(order) == 0:
            seen["none"] += 1
            regime.append(-1)
            continue
        s = bits.view(np.float32)
        d16 = s[:16].astype(np.float64) - float(s[0])
        seen["band"] += bool(((d16 > VANISH) & (d16 < BAND_HI)).any())
        seen["fewer"] += len(order) < K
        s = s[:K]
        best, lowest = s[0], s[-1]
        shifted = bool(lowest <= LINE)
        regime.append(int(shifted))
        seen["plain"] += bool(lowest > -307)
        seen["deep"] += bool(best <= LINE)
        seen["straddle"] += bool(best > LINE >= lowest)
        seen["edge_at"] += bool(lowest == LINE)
        seen["edge_above"] += bool(lowest == LINE_ABOVE)
        seen["edge_below"] += bool(lowest == LINE_BELOW)
        seen["edge_above_subnormal"] += bool(lowest == LINE_ABOVE and 10.0 ** float(best) < 2.3e-308)
        seen["vanish"] += bool(shifted and (s.astype(np.float64) - float(best) <= VANISH).any())
        seen["tied_best"] += bool(len(s) > 1 and bits[0] == bits[1])
    for g in range(len(regime) // 4):
        four = regime[4 * g:4 * g + 4]
        seen["mixed_wave"] += 1 in four and 0 in four
    return seen


def census_floor(K):
    """the least every count must reach for keep_at_most K (band: the most)"""
    need = dict(plain=30, deep=30, edge_at=10, edge_above=10, edge_below=10, edge_above_subnormal=5, none=5, mixed_wave=50)
    if K >= 2:
        need.update(straddle=30, tied_best=30)
    if K >= 3:
        need.update(vanish=20)
    if K >= 7:
        need.update(fewer=20)
    return need


def assert_census(vectors, K, what):
    seen = census(vectors, K)
    assert seen["band"] == 0, f"{what} K={K}: {seen['band']} reads with a difference inside ({VANISH}, {BAND_HI})"
    short = {c: (seen[c], n) for c, n in census_floor(K).items() if seen[c] < n}
    assert not short, f"{what} K={K}: too few reads with {short} ({seen})"
    return seen


def ns_bounds(vectors):
    """the float32 triple around the most frequent best score b0 among placed reads: below it, b0 itself, above it; at least 20 reads
    have their best score on b0, 20 above and 20 below"""
    best = np.array([bits[:1].view(np.float32)[0] for order, bits in vectors if len(order)], np.float32)
    values, counts = np.unique(best, return_counts=True)
    b0 = values[np.argmax(counts)]
    assert (best == b0).sum() >= 20 and (best > b0).sum() >= 20 and (best < b0).sum() >= 20, (b0, (best == b0).sum(), (best > b0).sum(), (best < b0).sum())
    return float(np.nextafter(b0, np.float32(-np.inf))), float(b0), float(np.nextafter(b0, np.float32(np.inf)))
