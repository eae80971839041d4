"""Planted databases and reads whose score vectors have a known shape, the plain-sort reference of the engine's order among equal
scores (score descending, branch ascending: DESIGN.md section 2, "Tie policy"), and the census of the shapes a set of reads holds --
shared by tests/test_gpu_select_locate.py, tests/test_gpu_tie_order.py (GPU) and tests/test_planted_shapes.py (no GPU).

A "family" describes where a placement kernel keeps a branch while it selects: the stream (the registers one lane feeds from every
4 * G-th slot), the quad (four neighbouring slots, always one lane's) and, for trees cut into windows, the window.  The census counts
the adversarial shapes relative to that layout, so that every kernel is given the reads that are hard for IT."""
import functools

import numpy as np

from rappas_amd import synth
from oracle import oracle as O

STREAMS = 64  # 4 streams in each of a 16-lane group's lanes

# the kinds of planted rows (the first four are the generator tests/test_gpu_select_locate.py began with)
ONE_STREAM, NEIGHBOURS, ANYWHERE, THREE_IN_A_STREAM, CLADE, ONE_WINDOW, NEIGHBOUR_WINDOWS, FAR_WINDOWS, HASH_QUAD = range(9)


def planted_db(alphabet, k, nb, n_keys, seed, stride=STREAMS, min_row=1, max_row=24, clades=False, window=0, hash_quads=(), short_rows=0.0):
    """rows of min_row ... max_row entries: branches `stride` apart (one stream), runs of neighbours, random sets and mixtures; scores
    drawn from 1, 2, 3 or 8 dyadic fractions of the threshold, so that equal sums are everywhere.  clades: also rows that hold a run
    of 4 ... 12 neighbours with ONE score (four of the best in one quad).  window: the tree is cut into windows of that many branches
    -- also rows whose branches sit in one window, in two neighbouring ones, and in two that are more than three apart.  hash_quads:
    the LOGS of place_hash64_kernel's tables -- also rows that hold, with one score, four branches whose home slots are one quad of the table.
    short_rows: that share of the rows has 1 ... 12 entries whatever min_row says (reads that touch fewer than K branches on a database
    of long rows).  Returns the database and the keys' digits.  (With the defaults: the databases tests/test_gpu_select_locate.py always had.)"""
    rng = np.random.default_rng(seed)
    digits = rng.integers(0, alphabet, (n_keys, k))
    dense = (digits.astype(np.uint64) * (np.uint64(alphabet) ** np.arange(k, dtype=np.uint64))).sum(1).astype(np.uint64)
    _, first = np.unique(dense, return_index=True)
    first.sort()
    digits, dense = digits[first], dense[first]
    thr, thr_log10 = synth.thresholds(1.5, alphabet, k)
    n_win = (nb - 1) // window + 1 if window else 0
    kinds = [ONE_STREAM, NEIGHBOURS, ANYWHERE, THREE_IN_A_STREAM] + ([CLADE, CLADE] if clades else []) + \
        ([ONE_WINDOW, NEIGHBOUR_WINDOWS, FAR_WINDOWS] if window else []) + [HASH_QUAD] * len(hash_quads)
    together = []  # sets of four branches in one quad of a hash table
    for logs in hash_quads:
        ids = np.arange(1, nb)
        q = Hash(logs, 1).quad(ids)
        order = np.argsort(q, kind="stable")
        cut = np.nonzero(np.diff(q[order]))[0] + 1
        together += [g[:4] for g in np.split(ids[order], cut) if len(g) >= 4]
    rows_b, rows_s = [], []
    for _ in range(len(dense)):
        m = int(rng.integers(min(min_row, nb - 1), min(max_row, nb - 1) + 1))
        kind = int(rng.integers(0, 4)) if len(kinds) == 4 else int(rng.choice(kinds))
        if short_rows and rng.random() < short_rows:
            m, kind = int(rng.integers(1, 13)), kind if kind < CLADE else ANYWHERE
        b = set()
        run = None
        if kind in (ONE_STREAM, THREE_IN_A_STREAM) and nb > stride + 2:  # one stream: b, b + stride, b + 2 * stride ...
            b0 = int(rng.integers(1, min(stride, nb - stride - 1) + 1))
            same = np.arange(b0, nb, stride)
            b.update(rng.choice(same, size=min(len(same), m if kind == ONE_STREAM else 3), replace=False).tolist())
        if kind == NEIGHBOURS:
            b0 = int(rng.integers(1, nb - m + 1))
            b.update(range(b0, b0 + m))
        if kind == CLADE:  # a run of neighbours with one score, starting on either slot numbering's quad boundary or anywhere
            n_run = int(rng.integers(4, 13))
            n_run = min(n_run, nb - 1)
            b0 = int(rng.integers(1, nb - n_run + 1))
            how = int(rng.integers(0, 3))
            if how < 2 and b0 >= 4:
                b0 = (b0 & ~3) - how  # how = 0: branch b0 is a multiple of 4; how = 1: slot b0 + 1 is
            run = range(b0, b0 + n_run)
            b.update(run)
            m = max(m, n_run)
        if kind == HASH_QUAD:  # four branches whose home slots are one quad of the hash table, with one score
            run = together[int(rng.integers(0, len(together)))].tolist()
            b.update(run)
        if kind in (ONE_WINDOW, NEIGHBOUR_WINDOWS, FAR_WINDOWS):
            far = 1 if kind == NEIGHBOUR_WINDOWS else 4
            if kind != ONE_WINDOW and n_win <= far:  # (the tree has too few windows)
                kind = ONE_WINDOW
            w0 = int(rng.integers(0, n_win if kind == ONE_WINDOW else n_win - far))
            wins = [w0] if kind == ONE_WINDOW else [w0, w0 + far]
            pool = np.concatenate([np.arange(max(1, w * window), min(nb, (w + 1) * window)) for w in wins])
            if kind != ONE_WINDOW:  # one branch in either window at least
                b.update(int(rng.integers(max(1, w * window), min(nb, (w + 1) * window))) for w in wins)
            m = max(m, len(b))
            b.update(rng.choice(np.setdiff1d(pool, list(b)), size=min(m - len(b), len(pool) - len(b)), replace=False).tolist())
            m = len(b)
        if len(b) < m:  # the rest (ANYWHERE: all of the row) anywhere in the tree
            b.update(rng.choice(np.arange(1, nb), size=m - len(b), replace=False).tolist())
        b = np.array(sorted(b), dtype=np.uint16)
        palette = int(rng.choice([1, 2, 3, 8]))
        s = (rng.integers(1, palette + 1, len(b)).astype(np.float32) / np.float32(8.0)) * np.float32(thr_log10)
        if run is not None:  # the clade's one score: the row's best or second best (scores are negative: the smallest fraction is best)
            s[np.isin(b, np.array(run))] = np.float32(int(rng.integers(1, 3)) / 8.0) * np.float32(thr_log10)
        rows_b.append(b)
        rows_s.append(s.astype(np.float32))
    off = np.zeros(len(dense) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in rows_b], out=off[1:])
    sdb = synth.SynthDB(alphabet, k, nb, thr, thr_log10, synth.dense_to_code(alphabet, k, dense), off,
                        np.concatenate(rows_b).astype(np.uint16), np.concatenate(rows_s).astype(np.float32), seed)
    return sdb, digits


def planted_reads(alphabet, k, digits, n, L, seed, p_keys=(0.06, 0.5, 0.3, 0.14)):
    """random reads of L symbols carrying none, one, two ... of the keys (p_keys[j] = the share of reads with j of them), each in its
    own stretch of the read; the read's last symbol belongs to no key"""
    rng = np.random.default_rng(seed)
    letters = synth.AA_LETTERS if alphabet == 20 else synth.DNA_LETTERS
    st = rng.integers(0, alphabet, (n, L))
    n_slots = len(p_keys) - 1
    how_many = rng.choice(np.arange(n_slots + 1), size=n, p=list(p_keys))
    slots = [j * L // n_slots for j in range(n_slots)]
    assert L // n_slots > k, (L, n_slots, k)
    for r in range(n):
        for j in range(how_many[r]):
            at = slots[j] + int(rng.integers(0, L // n_slots - k))
            st[r, at:at + k] = digits[int(rng.integers(0, len(digits)))]
    seq = np.ascontiguousarray(letters[st.reshape(-1)])
    return seq, (np.arange(n + 1, dtype=np.uint64) * np.uint64(L))


def with_ambiguity_code(alphabet, seq, off):
    """the same reads with their last symbol (outside every planted k-mer) replaced by N / X: each takes the ambiguity kernel"""
    seq = seq.copy()
    seq[off[1:].astype(np.int64) - 1] = ord("X") if alphabet == 20 else ord("N")
    return seq


def place_prefilled(pp, packed, n, L, K, keep_factor=0.01, amb=None, flags=None, seq=None, off=None, lens=None):
    """rk_place_packed_device into result tensors pre-filled with 0xFF bytes; every read must have been written.  amb ("skip" / "max" /
    "mean") with the packer's flags and the reads' characters: reads with an ambiguity code go through place_ascii_kernel (without the
    characters nobody places them).  lens: a length per read instead of the one length L."""
    import torch
    import rappas_amd as ra
    dev = torch.device("cuda", 0)
    out = dict(n_rows=torch.full((n,), 0xFF, dtype=torch.uint8, device=dev),
               branch=torch.full((n, K), -1, dtype=torch.int16, device=dev),
               score=torch.full((n, K), -1, dtype=torch.int32, device=dev).view(torch.float32),
               lwr=torch.full((n, K), -1, dtype=torch.int64, device=dev).view(torch.float64),
               flags=torch.full((n,), -1, dtype=torch.int32, device=dev))
    kw = {}
    if amb is not None:
        kw = dict(flags_in=torch.from_numpy(flags.view(np.int32)).to(dev), treatAmbiguities=amb != "skip", treatAmbiguitiesWithMax=amb == "max")
        if seq is not None:
            kw.update(seq_ascii=torch.from_numpy(seq).to(dev), seq_off=torch.from_numpy(off.astype(np.int64)).to(dev))
    if lens is not None:
        kw.update(lens=torch.from_numpy(lens.view(np.int32)).to(dev))
        L = 0
    pp.place_packed(torch.from_numpy(packed.view(np.int32)).to(dev), fixed_len=L, out=out, keepAtMost=K, keepFactor=keep_factor, **kw)
    torch.cuda.synchronize()
    o = {f: t.cpu().numpy() for f, t in out.items()}
    unwritten = np.nonzero((o["n_rows"] == 0xFF) | (o["flags"] == -1))[0]
    assert len(unwritten) == 0, f"{len(unwritten)} of {n} reads never written (first: {unwritten[:8]})"
    return ra.Placements(o["n_rows"], o["branch"].view(np.uint16), o["score"], o["lwr"], o["flags"].view(np.uint32), {})


def sorted_vectors(odb, seq, off, amb_mode=O.AMB_MEAN):
    """per read: the touched branches by (score descending, branch ascending) and their scores' bits"""
    res = []
    for r in range(len(off) - 1):
        S, touched, _ = odb.score_vector(bytes(seq[int(off[r]):int(off[r + 1])]), amb_mode)
        touched = np.sort(touched.astype(np.int64))
        order = touched[np.argsort(-S[touched].astype(np.float64), kind="stable")]
        res.append((order, S[order].view(np.uint32)))
    return res


def check_against_sorted_vectors(got, vectors, K, what):
    """every read's rows are the first n_rows entries of the plain sort of its score vector, branch for branch and bit for bit"""
    for r, (order, bits) in enumerate(vectors):
        n = int(got.n_rows[r])
        assert n <= min(K, len(order)), (what, r, K, n, len(order))
        assert np.array_equal(got.branch[r, :n].astype(np.int64), order[:n]) and np.array_equal(got.score[r, :n].view(np.uint32), bits[:n]), \
            f"{what} K={K} read {r}: got {got.branch[r, :n]} {got.score[r, :n]}, sorted vector {order[:K]} {bits[:K].view(np.float32)}"


# ---- families: where a kernel keeps branch b during its select ----
class Family:
    """stream(b), quad(b) and window(b) (None: the tree is not cut) of an array of branch ids, as integers that are equal exactly when
    two branches share the stream / quad / window; streams compare in the order the kernel's rounds break ties between streams in"""
    name = ""
    windows = False

    def window(self, b):
        return None


class Dense(Family):
    """place_packed_kernel / place_packed16_kernel / place_ascii_kernel with G lanes a read: slot = branch + 1, a lane reads quads
    G apart, so slots 4 * G apart share a stream (select_topk, Heads4 / Heads3)"""
    def __init__(self, G):
        self.G, self.name, self.stride = G, f"dense{G}", 4 * G

    def stream(self, b):
        return (b + 1) % self.stride

    def quad(self, b):
        return (b + 1) // 4


class Windowed(Family):
    """place_packed16w_kernel: the tree in windows of W branches, inside a window slot = branch - first + 1 and the 64 streams of a
    16-lane group; the heads live on from window to window, so equal window-relative slots mod 64 share a stream across windows too.
    place_packed16s_kernel (name "sorted") is counted in this layout as well, with its own, narrower windows: it feeds its heads from
    the lists of the slots a read touched, in list order, which this census does not model -- for that kernel the stream shapes
    (stream_equal / stream_differ, tie_ids_along / tie_ids_against) are those of the kernel its tiles are handed over to; the window
    shapes, quad_run, straddle, fewer and none are its own.  (The row-for-row comparison with the plain sort does not depend on it.)"""
    windows = True

    def __init__(self, W, name="windowed"):
        self.W, self.name, self.stride = W, name, STREAMS

    def stream(self, b):
        return (b % self.W + 1) % STREAMS

    def quad(self, b):
        return (b // self.W) * (self.W // 4 + 2) + (b % self.W + 1) // 4

    def window(self, b):
        return b // self.W


class Hash(Family):
    """place_hash64_kernel: key = branch + 1 at table slot (key * 0x9E3779B1) >> (32 - LOGS) (its home; a clash moves it on), lane l reads
    the table's quads 64 apart: slots 256 apart share a stream.  The windows are those of the tiles it hands to place_packed16w_kernel."""
    windows = True

    def __init__(self, logs, W):
        self.logs, self.W, self.name, self.stride = logs, W, f"hash{1 << logs}", 256

    def slot(self, b):
        return (((b + 1).astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)).astype(np.int64) >> (32 - self.logs)

    def stream(self, b):
        return self.slot(b) % 256

    def quad(self, b):
        return self.slot(b) // 4

    def window(self, b):
        return b // self.W


class Workgroup(Family):
    """place_wg_kernel with NW waves and P branch-range passes: a pass holds 32 / P of the tree's 32 index-line ranges, a wave owns
    32 / P / NW of them; in a pass slot = branch - the pass's first branch, a wave's lanes read its segment's quads 64 apart: slots
    256 apart inside a wave's range share a stream, the four slots of a quad one lane"""
    def __init__(self, nb, NW, P):
        self.nb, self.NW, self.P, self.name, self.stride = nb, NW, P, f"wg{P}", 256
        span = 32 // P
        edge = [i * nb // 32 for i in range(33)]
        self.seg_lo, self.seg_base = [], []
        for p in range(P):
            for w in range(NW):
                q_lo, q_hi = p * span + w * span // NW, p * span + (w + 1) * span // NW
                if q_hi > q_lo and edge[q_hi] > edge[q_lo]:
                    self.seg_lo.append(edge[q_lo])
                    self.seg_base.append(edge[p * span])
        self.seg_lo, self.seg_base = np.array(self.seg_lo), np.array(self.seg_base)

    def _seg(self, b):
        return np.searchsorted(self.seg_lo, b, side="right") - 1

    def stream(self, b):
        s = self._seg(b)
        slot, sq0 = b - self.seg_base[s], (self.seg_lo[s] - self.seg_base[s]) // 4
        return s * 256 + ((slot // 4 - sq0) % 64) * 4 + slot % 4

    def quad(self, b):
        s = self._seg(b)
        return s * (1 << 16) + (b - self.seg_base[s]) // 4


def window_plan(nb, bits, stream):
    """(windows, branches a window) of a windowed image (rk_geometry.h: window_plan); stream: the image was built for
    place_packed16s_kernel first (DNA beyond 4 500 branches with short rows, every windowed amino-acid tree, RK_WSTREAM_ALWAYS)"""
    n_win = min(64, (nb + 511) // 512 if stream else (nb + 895) // 896)
    return n_win, ((nb + n_win - 1) // n_win + 3) & ~3


def family(route, nb, bits):
    """the family of the kernel a route of tests/test_gpu_tie_order.py reaches, on a tree of nb branches with `bits` bits a symbol"""
    stream = bits == 5 or nb > 4500  # the image of these trees' short rows was built for place_packed16s_kernel first
    W = window_plan(nb, bits, stream)[1]
    if route.startswith("lanes"):
        return Dense(int(route[5:]) or 16)
    return {"ascii": lambda: Dense(64), "windowed": lambda: Windowed(W), "sorted": lambda: Windowed(W, "sorted"),
            "sorted_always": lambda: Windowed(window_plan(nb, bits, True)[1], "sorted"), "hash": lambda: Hash(11, W),
            "hash_small": lambda: Hash(10, W), "hash_slack": lambda: Hash(11, W), "wg1": lambda: Workgroup(nb, 8, 1),
            "wg2": lambda: Workgroup(nb, 16, 2), "wg4": lambda: Workgroup(nb, 16, 4)}[route]()


SHAPES = ["none", "fewer", "straddle", "tie_ids_along", "tie_ids_against", "stream_equal", "stream_differ", "quad_run",
          "one_window", "neighbour_windows", "far_windows"]


def shapes_met(vectors, K, seen, fam=None):
    """which of the adversarial shapes the reads' score vectors hold for keep_at_most K, in the layout of `fam` (default: 16 lanes):
    none / fewer than K touched, a tie across rank K, equal scores in different streams with the stream order along / against the
    branch order, two of the K best in one stream with equal / different scores, four of them in one quad, and -- trees in windows --
    the K best in one window, in two neighbouring ones, more than three windows apart"""
    fam = fam or Dense(16)
    for order, bits in vectors:
        if len(order) == 0:
            seen["none"] += 1
            continue
        if len(order) < K:
            seen["fewer"] += 1
        if len(order) > K and bits[K - 1] == bits[K]:
            seen["straddle"] += 1
        top, tb = order[:K], bits[:K]
        stream = fam.stream(top)
        for i in range(len(top)):
            for j in range(i + 1, len(top)):
                if stream[i] == stream[j]:
                    seen["stream_equal" if tb[i] == tb[j] else "stream_differ"] += 1
                elif tb[i] == tb[j]:  # top is sorted: top[i] < top[j] here
                    seen["tie_ids_along" if stream[i] < stream[j] else "tie_ids_against"] += 1
        if "quad_run" in seen and len(top) >= 4 and np.unique(fam.quad(top), return_counts=True)[1].max() >= 4:
            seen["quad_run"] += 1
        w = fam.window(top)
        if w is not None and "one_window" in seen and len(top) >= 2:
            lo, hi = int(w.min()), int(w.max())
            if lo == hi:
                seen["one_window"] += 1
            elif hi - lo == 1:
                seen["neighbour_windows"] += 1
            elif hi - lo > 3:
                seen["far_windows"] += 1


def shapes_possible(fam, nb):
    """the shapes that can occur on a tree of nb branches in the layout of `fam`"""
    need = ["none", "fewer", "straddle", "tie_ids_along", "quad_run"]
    if isinstance(fam, Hash) or nb + 1 > fam.stride:  # (below, a slot is its own stream id: no pair against the order, none in one stream)
        need += ["tie_ids_against", "stream_equal", "stream_differ"]
    if fam.windows:
        n_win = (nb - 1) // fam.W + 1
        need += ["one_window"] + (["neighbour_windows"] if n_win > 1 else []) + (["far_windows"] if n_win > 4 else [])
    return need


def census(vectors, Ks, fam):
    seen = dict.fromkeys(SHAPES, 0)
    for K in Ks:
        shapes_met(vectors, K, seen, fam)
    return seen


def assert_census(vectors, Ks, fam, nb, what):
    seen = census(vectors, Ks, fam)
    missing = [c for c in shapes_possible(fam, nb) if seen[c] == 0]
    assert not missing, f"{what} ({fam.name}): no read with {missing} ({seen})"
    return seen


# ---- the planted trees of tests/test_gpu_tie_order.py and tests/test_planted_shapes.py: database, reads, sorted score vectors ----
K_ALL = tuple(range(1, 17))
K_EDGES = (1, 2, 3, 7, 8, 9, 15, 16)

#        name: (alphabet, k, branches, symbols a read, reads, seed, keyword arguments of planted_db, p_keys of planted_reads)
MANY = (0.04, 0.06, 0.02, 0.04, 0.1, 0.2, 0.18, 0.18, 0.18)  # up to eight keys a read: ~100 row entries, more than a hash table of 64 keys takes
TREES = {
    **{f"dna{nb}": (4, 10, nb, 150, 400, 300 + nb, dict(stride=32 if nb < 128 else 256, clades=True), None) for nb in (30, 63, 64, 65, 399, 998, 999)},
    "aa399": (20, 5, 399, 100, 400, 17, dict(stride=256, clades=True), None),
    "dna1117": (4, 10, 1117, 150, 300, 1117, dict(stride=256, clades=True), None),  # (the largest tree the dense 16-lane kernel keeps: windows start beyond 1 276 branches)
    "dna1277": (4, 10, 1277, 150, 300, 1277, dict(stride=64, clades=True, window=640), None),
    "dna2801": (4, 10, 2801, 150, 300, 2801, dict(stride=64, clades=True, window=704, hash_quads=(10, 11)), None),
    "dna4500": (4, 10, 4500, 150, 300, 4500, dict(stride=64, clades=True, window=752), None),
    "dna4501": (4, 10, 4501, 150, 300, 4501, dict(stride=64, clades=True, window=504), None),
    "dna9001": (4, 10, 9001, 150, 250, 9001, dict(stride=64, clades=True, window=504, hash_quads=(10, 11)), None),
    "dna2801many": (4, 10, 2801, 150, 200, 2801, dict(stride=64, clades=True, window=704, hash_quads=(10, 11) * 3), MANY),
    "dna9001many": (4, 10, 9001, 150, 200, 9001, dict(stride=64, clades=True, window=504, hash_quads=(10, 11) * 3), MANY),
    "aa1999": (20, 5, 1999, 100, 300, 1999, dict(stride=64, clades=True, window=500), None),
    "wg13301": (4, 10, 13301, 150, 200, 13301, dict(stride=256, clades=True, min_row=330, max_row=470, short_rows=0.12), None),
}


# (tree, route, keep_at_most values, ambiguity mode) of every case of tests/test_gpu_tie_order.py
CASES = ([(f"dna{nb}", "lanes8", tuple(range(1, 9)), None) for nb in (30, 63, 64, 65, 399, 998)] +
         [(f"dna{nb}", f"lanes{g}", K_ALL, None) for nb in (30, 63, 64, 65, 399, 998, 999) for g in (32, 64)] +
         [("aa399", "lanes64", K_ALL, None)] +
         [(name, "ascii", K_ALL, amb) for name in ("dna64", "dna399", "dna999", "aa399") for amb in ("skip", "max", "mean")] +
         [(name, "windowed", K_ALL, None) for name in ("dna1277", "dna2801", "dna4500", "dna9001")] +
         [("dna1117", f"lanes{g}", K_ALL, None) for g in (32, 64)] +
         [(name, "sorted", K_ALL, None) for name in ("dna4501", "dna9001", "aa1999")] +
         [(name, route, K_EDGES, None) for name in ("dna2801", "dna9001") for route in ("hash", "hash_small")] +
         [(name, "hash_slack", K_EDGES, None) for name in ("dna2801many", "dna9001many")] +
         [("wg13301", "wg1", K_EDGES, None), ("wg13301", "wg2", (8, 16), None), ("wg13301", "wg4", (8, 16), None)])


@functools.lru_cache(maxsize=None)
def tree(name):
    """(database, oracle database, reads, offsets, sorted score vectors) of a planted tree, made once a process and left unchanged"""
    alphabet, k, nb, L, n_reads, seed, kw, p_keys = TREES[name]
    sdb, digits = planted_db(alphabet, k, nb, 300, seed, **kw)
    odb = O.OracleDB.from_synth(sdb)
    seq, off = planted_reads(alphabet, k, digits, n_reads, L, seed + 1, **({} if p_keys is None else dict(p_keys=p_keys)))
    return sdb, odb, seq, off, sorted_vectors(odb, seq, off)


@functools.lru_cache(maxsize=None)
def ambiguous(name, amb):
    """the reads of a planted tree with an ambiguity code each, and their sorted score vectors in ambiguity mode amb"""
    from tests import golden_util as GU
    sdb, odb, seq, off, _ = tree(name)
    seq = with_ambiguity_code(sdb.alphabet, seq, off)
    return seq, sorted_vectors(odb, seq, off, GU.AMB[amb])


@functools.lru_cache(maxsize=None)
def oracle_place(name, K, keep_factor, amb=None):
    """the oracle's placements of a planted tree's reads, once per (keep_at_most, keep_factor, ambiguity mode)"""
    from tests import golden_util as GU
    sdb, odb, seq, off, _ = tree(name)
    if amb is not None:
        seq, _ = ambiguous(name, amb)
    return odb.place(seq, off, keep_at_most=K, keep_factor=keep_factor, amb_mode=GU.AMB[amb or "mean"])
