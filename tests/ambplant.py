"""Planted reads and databases for place_ascii_kernel's accumulate paths (amb_position and its caller in rk_kernels.hip), and the census
of the shapes they hold -- shared by tests/test_amb_planted_shapes.py (no GPU) and tests/test_gpu_amb_planted.py (GPU).

A SITE is one ambiguous k-mer of a read (1 ... max_amb ambiguity codes inside it) together with the rows of its alternative words.
The reads are generated first: random symbols with ambiguity codes at chosen indices.  Then the alternative words of every site are
given rows by recipe (row lengths around the kernel's 16- and 64-entry limits, 0 ... W alternatives without a row, a branch shared
by exactly h alternatives, branches at the borders of the Samb / Camb chunks and of the tree windows); nearly every other k-mer of a
read has no row, so the reported rows are made of the sites' branches.  Where two sites ask for the same word the first assignment
wins, and a word that is also a plain k-mer of some read gets no row as an alternative.  The census is computed from the FINAL
database and reads: it restates the kernel's predicates in plain Python, with amb_chunk and s_win taken from the host tool the
geometry tests compile (tests/geometry_grid.cpp: case amb nb=... lds=... indexed=...)."""
import atexit
import collections
import functools
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

from rappas_amd import synth
from oracle import oracle as O
from tests import golden_util as GU
from tests import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
LIST_CAP = 160                                # ASCII_LIST_CAP: the pending list is flushed before it would hold more than LIST_CAP - 1 rows
LENGTHS = (1, 15, 16, 17, 63, 64, 65, 98)     # row lengths around the 16-lane and the 64-lane form's limits
X_LENGTHS = (1, 16, 65)                       # ... of the third and further alternatives of a code with twenty
DNA_CODES = {2: "RYSWKM", 3: "BDHV", 4: "N"}
AA_CODES = {2: "BZJ", 20: "X"}


# ---- the geometry of the ambiguity kernel, from the host tool ----
@functools.lru_cache(maxsize=None)
def _tool():
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "no C++ compiler (g++) for tests/geometry_grid.cpp"
    d = tempfile.mkdtemp(prefix="ambplant_geometry_")
    atexit.register(shutil.rmtree, d, True)
    exe = os.path.join(d, "geometry_grid")
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "rappas_amd", "csrc"), os.path.join(ROOT, "tests", "geometry_grid.cpp"),
                    "-o", exe], check=True)
    return exe


@functools.lru_cache(maxsize=None)
def amb_geometry(nb, indexed=False):
    """(amb_chunk, s_win) of a tree of nb branches on a CU with 160 KB of LDS"""
    out = subprocess.run([_tool(), "case", "amb", f"nb={nb}", f"lds={LDS_PER_CU}", f"indexed={int(indexed)}"], check=True, capture_output=True, text=True).stdout
    f = dict(kv.split("=", 1) for kv in out.rstrip("\n").split("\t")[2].split())
    assert f["status"] == "0", out
    return int(f["amb_chunk"]), int(f["s_win"])


@functools.lru_cache(maxsize=None)
def smallest_chunked_tree(beyond=64):
    """the smallest tree whose Samb / Camb windows do not cover it, with at least `beyond` branches left to the second chunk pass.  (Chunk
    passes begin at amb_chunk < n_branches, 5 301 branches with 160 KB of LDS -- but there the second pass holds the tree's last branch
    alone, and the branches lo + 1 and "another one above the border" the census asks for do not exist; amb_chunk falls by one for every
    two branches more, so n_branches - amb_chunk only grows.)"""
    lo, hi = 100, 8192  # (8 192: the largest tree that never gets an indexed image)
    assert amb_geometry(lo)[0] >= lo and hi - amb_geometry(hi)[0] >= beyond
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if mid - amb_geometry(mid)[0] >= beyond:
            hi = mid
        else:
            lo = mid
    return hi


KS = (1, 7, 16)
MODES = ("mean", "max", "skip")


def keep_factor(K):
    """keep_at_most 16 runs with keep factor 0 (every one of the 16 best is reported), the others with the default"""
    return 0.0 if K == 16 else 0.01


# ---- the families ----
#        name: alphabet, k, branches (None: smallest_chunked_tree()), table mode, indexed image, star reads, seed
FAMILIES = {
    "dna99": dict(alphabet=4, k=8, nb=99, table="auto", indexed=False, n_star=320, seed=9901),
    "aa399": dict(alphabet=20, k=4, nb=399, table="auto", indexed=False, n_star=400, seed=39901),
    "dna_chunks": dict(alphabet=4, k=8, nb=None, table="auto", indexed=False, n_star=320, seed=6001),
    "dna_indexed": dict(alphabet=4, k=8, nb=19999, table="hash", indexed=True, n_star=360, seed=19999),
    "dna_windows": dict(alphabet=4, k=8, nb=45001, table="auto", indexed=False, n_star=360, seed=45001),
    "dna16": dict(alphabet=4, k=16, nb=99, table="hash", indexed=False, n_star=280, seed=1699),
    # (k = 16 has no code at p >= 16: the alternatives placed at bit 32 of the code and beyond take a longer k-mer)
    "dna20": dict(alphabet=4, k=20, nb=99, table="hash", indexed=False, n_star=280, seed=2099),
}
TABLES_OF_DNA99 = ("auto", "direct8", "hash")  # the table modes dna99 runs in on the device; every other family runs in its own

_POSITIONS = ["code@0", "code@k-1", "code@63", "code@64", "code@64+k-2", "code@R-k", "code@R-1"]
_COMMON = ["base=QT", "touched_before_plain", "touched_before_amb", "touched_later_plain", "codes<k_apart", "codes>=k_apart", "code_run>k",
           "only_codes", "R==k", "R<k", "pending_row>64"] + _POSITIONS
_DNA_W = ["W=2", "W=3", "W=4"] + [f"missing={m}" for m in range(5)] + [f"shared={h}" for h in range(1, 5)]
_BORDERS = ["general:chunks", "at_lo-1", "at_lo", "at_lo+1", "first_branch", "last_branch", "straddles_border"]
# the classes that must hold >= 4 sites (or reads) in a family
CLASSES = {
    "dna99": ["lane16", "lane64", "general:row>64"] + _DNA_W + _COMMON + [f"p={p}" for p in range(8)] +
             ["hits_before_code=159", "hits_before_code=160", "hits_before_code=161", "hits_before_code>=192", "flush_at_cap", "skipped:2_codes"],
    "aa399": ["lane16", "lane64", "general:row>64", "general:W>4", "W=2", "W=20", "missing=0", "missing=1", "missing=2", "missing>=10", "missing=20",
              "shared=1", "shared=2", "shared=19", "shared=20"] + _COMMON + [f"p={p}" for p in range(4)],
    "dna_chunks": _BORDERS + _DNA_W + _COMMON + [f"p={p}" for p in range(8)],
    "dna_indexed": _BORDERS + _DNA_W + _COMMON + [f"p={p}" for p in range(8)],
    "dna_windows": ["lane16", "lane64", "general:row>64", "at_lo-1", "at_lo", "at_lo+1", "first_branch", "last_branch", "straddles_border",
                    "top7_in_3_windows", "top16_in_3_windows", "top1_in_last_window", "top7_in_last_window", "top16_in_last_window"] +
                   _DNA_W + _COMMON + [f"p={p}" for p in range(8)],
    "dna16": ["lane16", "lane64", "general:row>64", "general:two_codes", "W=4x4", "W=2x2", "W=2x3", "W=3x2", "W=4x2", "repeated_words", "skipped:3_codes"] +
             _DNA_W + _COMMON + [f"p={p}" for p in range(16)],
}
CLASSES["dna20"] = CLASSES["dna16"] + [f"p={p}" for p in range(16, 20)] + ["2p>=32", "second_code:2p>=32"]


class Family:
    """one family after generation: sdb (synth.SynthDB), pydb (the dict tests/pyref.py reads), seq / off (the reads), reads (their
    strings), sites (a list per read), census (a Counter of class names) and what the geometry tool gave"""


def _letters(alphabet):
    return "ATCG" if alphabet == 4 else pyref.AA_ORDER


def _alts(alphabet, ch):
    kind, val = pyref.classify(alphabet, ch)
    return val if kind == "amb" else None


def _plans(name, alphabet, k, n_star, rng):
    """(symbols, {index: code}, tags) of every read of a family"""
    by_w = DNA_CODES if alphabet == 4 else AA_CODES
    widest = max(by_w)  # every other code is the one with most alternatives (N / X): its last alternatives occur under no other code
    cycle = [c for i in range(12) for w in sorted(by_w) if w != widest for c in (by_w[widest][0], by_w[w][i % len(by_w[w])])]
    n = [0]

    def code():
        n[0] += 1
        return cycle[n[0] % len(cycle)]

    max_amb = int(math.floor(math.pow(k, 1.0 / alphabet)))
    plans = []
    for i in range(n_star):  # short reads with one code; read i's site number i % (sites of the read) is its star
        R = int(rng.integers(k + 4, 64))
        tags = {"star"} | ({"plain_rows"} if i % 3 == 0 else set()) | ({"last_window"} if i % 4 == 1 else set())
        plans.append((R, {int(rng.integers(0, R)): code()}, tags))
    for i in range(5):  # the code at every index that is special relative to the 64-position blocks
        R = 64 + 3 * k + 7 * i
        for pos in (0, k - 1, 63, 64, 64 + k - 2, R - k, R - 1):
            plans.append((R, {pos: code()}, {"spread", "plain_rows"}))
    for i in range(8):  # two codes less than k apart: the k-mers that hold both are skipped where max_amb = 1
        plans.append((60, {20: code(), 20 + 1 + i % (k - 1): code()}, {"spread"}))
    for d in (k, k + 1, 3 * k, k, k + 2, 2 * k):
        plans.append((70 if 12 + 3 * k < 70 else 3 * k + 24, {12: code(), 12 + d: code()}, {"spread"}))
    for i in range(4):
        plans.append((50 + i, {15 + j: code() for j in range(k + 2 + i)}, {"spread"}))  # a run of codes longer than k
        plans.append((k + 4 + i, {j: code() for j in range(k + 4 + i)}, set()))          # only codes
    for i in range(2 * k):
        plans.append((k, {i % k: code()}, {"spread"}))                                    # exactly k symbols, one code
    for i in range(4):
        plans.append((max(1, k - 1 - 2 * i), {0: code()}, set()))                         # shorter than k
    for i in range(6):  # a pending plain row of more than 64 entries when the code forces the flush
        plans.append((50, {40: code()}, {"long_pending", "spread"}))
    if name == "dna99":
        for h in (159, 160, 161, 192, 200):  # h plain k-mers with a row each, then a code
            for t in range(4):
                plans.append((h + k + t, {h + k - 1: code()}, {f"hits={h}", "spread"}))
    if max_amb >= 2:  # two codes in one k-mer (DNA k >= 16): class pairs with equal and with coprime counts; three codes are skipped
        pairs = ["NN", "RR", "RB", "BR", "NR", "YY", "NN", "KH", "VM", "NS", "WW", "NN"]
        for i in range(36):
            a, b = pairs[i % len(pairs)]
            plans.append((3 * k + 4, {k + 2: a, k + 2 + 1 + (5 * i) % (k - 1): b}, {"star2", "spread"}))
        for i in range(6):
            plans.append((3 * k, {k: "N", k + 2 + i: "R", k + 5 + i: "B"}, {"spread"}))
    return plans


def _kmers(alphabet, k, read):
    """per k-mer of a read: (its symbols with -1 at the codes, the indices of its codes inside it); None for reads that are not placed"""
    seq, alts = [], {}
    for i, ch in enumerate(read):
        kind, val = pyref.classify(alphabet, ch)
        assert kind != "bad"
        seq.append(val if kind == "state" else -1)
        if kind == "amb":
            alts[i] = val
    return [(seq[j:j + k], [p for p in range(k) if seq[j + p] == -1]) for j in range(len(read) - k + 1)], alts


def _words(alphabet, kmer, ps, alts_at):
    """the alternative words of an ambiguous k-mer in the reference's order (word w takes alternative w % count at EVERY code)"""
    W = 1
    for p in ps:
        W *= len(alts_at[p])
    out = []
    for w in range(W):
        sym = list(kmer)
        for p in ps:
            sym[p] = alts_at[p][w % len(alts_at[p])]
        out.append(pyref.kmer_code(alphabet, sym))
    return out


def _site_rows(pool, lens, h, rot):
    """rows (sorted branch lists; None: no row) of lengths lens: exactly h of them list pool[rot]; while the pool is large enough every other
    entry is listed once (the largest number of alternatives that list one branch is then exactly h), beyond that the rows are runs of the pool"""
    P = len(pool)
    star = pool[rot % P]
    rest = [b for b in pool[rot % P + 1:] + pool[:rot % P]]
    present = [a for a, n in enumerate(lens) if n]
    rows = [None] * len(lens)
    disjoint = sum(lens) <= P - 1
    at = 0
    for i, a in enumerate(present):
        n = lens[a] - (1 if i < h else 0)
        if disjoint:
            row, at = rest[at:at + n], at + n
        else:
            s0 = (a * 29) % (P - 1)
            row = (rest[s0:] + rest[:s0])[:n]
        row = row + ([star] if i < h or len(row) < n else [])  # (a row of every branch of the tree lists the shared one too)
        rows[a] = sorted(row)
    return rows


@functools.lru_cache(maxsize=None)
def family(name):
    f = Family()
    spec = FAMILIES[name]
    f.name, f.alphabet, f.k, f.table, f.indexed = name, spec["alphabet"], spec["k"], spec["table"], spec["indexed"]
    nb = f.nb = spec["nb"] or smallest_chunked_tree()
    k, alphabet = f.k, f.alphabet
    f.max_amb = int(math.floor(math.pow(k, 1.0 / alphabet)))
    f.chunk, f.s_win = amb_geometry(nb, f.indexed)
    n_win = (nb + min(f.s_win, nb) - 1) // min(f.s_win, nb)
    f.borders = [w * f.s_win for w in range(1, n_win)] if n_win > 1 else list(range(f.chunk, nb, f.chunk)) if f.chunk < nb else []
    rng = np.random.default_rng(spec["seed"])
    P_thr, T = synth.thresholds(1.5, alphabet, k)
    letters = _letters(alphabet)

    # the reads
    plans = _plans(name, alphabet, k, spec["n_star"], rng)
    reads = []
    for R, codes, tags in plans:
        s = [letters[int(x)] for x in rng.integers(0, alphabet, R)]
        for i, c in codes.items():
            s[i] = c
        reads.append("".join(s))
    parsed = [_kmers(alphabet, k, r) for r in reads]
    plain = {pyref.kmer_code(alphabet, km) for kms, _ in parsed for km, ps in kms if not ps}

    # the scores: distinct float32 values in [T, 0)
    used = set()

    def score(lo, hi):  # a new value T * u, u in [lo, hi): u near 1 is a score near the threshold
        while True:
            v = np.float32(float(T) * float(rng.uniform(lo, hi)))
            if v.tobytes() not in used and T <= v < 0:
                used.add(v.tobytes())
                return v

    rows, bands = {}, {}  # word -> [(branch, score)], and the (lo, hi) every score was drawn with

    def give(word, branches, band_of=lambda e, b: (0.95, 1.0)):
        if word not in rows:
            bands[word] = [band_of(e, b) for e, b in enumerate(branches)]
            rows[word] = [(b, score(*bands[word][e])) for e, b in enumerate(branches)]

    def low_row(branches):
        return sorted(branches)

    Wmax = 4 if alphabet == 4 else 20
    need = {}  # (length class, alternative) -> the entry indices no star site has taken yet

    def refill(c, a):
        need[c, a] = list(range(c))

    def pool_of(tags):
        """the branches a read's rows are drawn from: on a small tree all of them; on a large one those next to a chunk or window border,
        the tree's first and last branch and 120 others -- for a "last_window" read all from the last window"""
        if nb <= 400:
            return [int(b) for b in rng.permutation(np.arange(1, nb))]
        lo_all = 1
        special = []
        if "last_window" in tags and f.borders:
            lo_all = f.borders[-1]
            special = list(dict.fromkeys(b for b in (f.borders[-1], f.borders[-1] + 1, nb - 1) if b < nb))
        else:
            B = f.borders[int(rng.integers(0, len(f.borders)))]
            special = list(dict.fromkeys(b for b in (B - 1, B, B + 1, 1, nb - 1) if b < nb))
            if len(f.borders) > 1:
                B2 = f.borders[int(rng.integers(0, len(f.borders)))]
                special += [b for b in (B2 - 1, B2, B2 + 1) if b not in special and b < nb]
        others = [int(b) for b in rng.choice(np.arange(lo_all, nb), size=min(140, nb - lo_all), replace=False) if int(b) not in special][:120]
        if len(others) < 120:  # (a last window of a few branches only: the rest from the whole tree)
            others += [int(b) for b in rng.choice(np.arange(1, lo_all), size=140, replace=False) if int(b) not in special][:120 - len(others)]
        return special + others

    # deliberate rows on plain k-mers, before any site: what is pending when a code forces the flush, and what touches a site's branches before and after it
    pools = []
    for r, ((R, codes, tags), (kms, alts)) in enumerate(zip(plans, parsed)):
        pool = pool_of(tags)
        pools.append(pool)
        plain_js = [j for j, (km, ps) in enumerate(kms) if not ps]
        word = lambda j: pyref.kmer_code(alphabet, kms[j][0])
        hits = [int(t[5:]) for t in tags if t.startswith("hits=")]
        if hits:
            for j in plain_js[:hits[0]]:
                give(word(j), low_row(pool[(3 * j) % 90:(3 * j) % 90 + 1 + j % 3]))
        if "long_pending" in tags and plain_js:
            give(word(plain_js[len(plain_js) // 3]), low_row(pool[:min(len(pool), 70 + r % 20)]))
        if "plain_rows" in tags and plain_js:
            for j in (plain_js[0], plain_js[-1]):
                give(word(j), low_row(pool[:6]))

    # the sites
    s_no = 0
    for r, ((R, codes, tags), (kms, alts)) in enumerate(zip(plans, parsed)):
        pool = pools[r]
        site_js = [j for j, (km, ps) in enumerate(kms) if 1 <= len(ps) <= f.max_amb]
        if "star2" in tags:
            two = [j for j in site_js if len(kms[j][1]) == 2]
            star_j = two[r % len(two)] if two else None
        else:
            star_j = site_js[r % len(site_js)] if site_js and "star" in tags else None
        for j in site_js:
            km, ps = kms[j]
            words = _words(alphabet, km, ps, {p: alts[j + p] for p in ps})
            distinct = list(dict.fromkeys(words))
            W = len(distinct)
            s_no += 1
            if j == star_j:  # every alternative has a row, of the length class that still needs most entries seen
                lens = []
                for a in range(W):
                    if not any(need.get((c, a)) for c in LENGTHS):  # (every length of this alternative has been through: once more)
                        for c in LENGTHS:
                            refill(c, a)
                    wide = a >= 2 and W > 4  # (twenty alternatives: the third and further ones have rows of 1, 16 and 65 entries)
                    among = LENGTHS if not wide else X_LENGTHS
                    lens.append(max(among, key=lambda c: (len(need[c, a]) / c, c)) if a < Wmax else 16)
                h = (1, 2, 19, 20)[(s_no // 5) % 4] if W > 4 else 1 + (s_no // 5) % W
            else:
                tier = s_no % 3
                choice = (LENGTHS[:3], LENGTHS[:6], LENGTHS)[tier]
                m = (s_no // 3) % (W + 1) if W <= 4 else (0, 1, 0, 2, 0, 1, 10, 0, 19, 20)[(s_no // 3) % 10]
                gone = {(s_no + i) % W for i in range(m)}
                lens = [0 if a in gone else choice[(s_no + 3 * a) % len(choice)] for a in range(W)]
                here = [a for a in range(W) if lens[a]]
                if here and tier:
                    lens[here[0]] = ((17, 63, 64), (65, 98))[tier - 1][(s_no // 3) % (4 - tier)]
                if W > 4:
                    lens = [n if a < 2 or not n else 65 if (a + s_no) % 7 == 0 else X_LENGTHS[(a + s_no) % 2] for a, n in enumerate(lens)]
                n_here = sum(1 for n in lens if n)
                h = min(max(n_here, 1), (1, 2, 19, 20)[(s_no // 5) % 4] if W > 4 else 1 + (s_no // 5) % W)
            # (a code with twenty alternatives keeps the words that are plain k-mers elsewhere: one in ten, of a key space they hardly fill)
            new = [a for a in range(W) if distinct[a] not in rows and (W > 4 or distinct[a] not in plain)]
            made = _site_rows(pool, lens, h, s_no if nb <= 400 else s_no % 16)
            stars = {}
            if j == star_j:  # 16 entries of the site's rows, with different branches, get the read's best scores
                taken, quota = set(), 16
                order = sorted(new, key=lambda a: -len(need.get((lens[a], a), ())) if a < Wmax else 0)
                while quota and order:
                    progress = False
                    for a in list(order):
                        if not quota:
                            break
                        if a >= Wmax or made[a] is None:
                            order.remove(a)
                            continue
                        left = [e for e in need[lens[a], a] if made[a][e] not in taken]
                        if not left:
                            left = [e for e in range(lens[a]) if made[a][e] not in taken]
                            if not left:
                                order.remove(a)
                                continue
                            refill(lens[a], a)
                        e = left[0]
                        need[lens[a], a].remove(e)
                        taken.add(made[a][e])
                        stars[a, e] = score(0.003, 0.5)
                        quota -= 1
                        progress = True
                    if not progress:
                        break
            shared = pool[(s_no if nb <= 400 else s_no % 16) % len(pool)]
            for a in new:
                if made[a] is None:
                    continue

                def band_of(e, b, a=a):
                    if (a, e) in stars:
                        return (0.003, 0.5)  # the read's best scores
                    # the branch several alternatives list: scores of every magnitude -- in the reads that need no star, at the star, and wherever
                    # three alternatives or more share it in the 16-lane form (two terms commute: the order of a sum shows from the third on)
                    if b == shared and ("spread" in tags or j == star_j or (h >= 3 and max(lens) <= 16)):
                        return (0.003, 1.0)
                    return (0.95, 1.0)
                give(distinct[a], made[a], band_of)

    def finish():
        codes_sorted = sorted(rows)
        off = np.zeros(len(codes_sorted) + 1, np.uint64)
        np.cumsum([len(rows[c]) for c in codes_sorted], out=off[1:])
        return synth.SynthDB(alphabet, k, nb, P_thr, T, np.array(codes_sorted, np.uint64), off,
                             np.array([b for c in codes_sorted for b, _ in rows[c]], np.uint16),
                             np.array([v for c in codes_sorted for _, v in rows[c]], np.float32), spec["seed"])

    # No read may hold an exact tie among its best 17 scores (the reference's order among equal scores is its hash map's).  The sums of a
    # read are float32 values near Q * T, far coarser than the scores: where the oracle finds a tie in any mode, the scores of the rows
    # that read meets are drawn again, each from the range it came from.
    f.seq, f.off = reads_array(reads)
    for attempt in range(12):
        f.sdb = finish()
        odb = O.OracleDB.from_synth(f.sdb)
        tied = set()
        for mode in MODES:
            for K in KS:
                tied.update(np.nonzero(odb.place(f.seq, f.off, keep_at_most=K, keep_factor=keep_factor(K), amb_mode=GU.AMB[mode])["flags"] & O.RO_FLAG_TIE)[0].tolist())
        odb.close()
        if not tied:
            break
        for r in sorted(tied):
            kms, alts = parsed[r]
            met = set()
            for j, (km, ps) in enumerate(kms):
                met.update([pyref.kmer_code(alphabet, km)] if not ps else _words(alphabet, km, ps, {p: alts[j + p] for p in ps}) if len(ps) <= f.max_amb else [])
            for w in sorted(met & set(rows)):
                rows[w] = [(b, score(*bands[w][e])) for e, (b, _) in enumerate(rows[w])]
    assert not tied, (name, sorted(tied))

    f.reads = reads
    f.pydb = dict(alphabet=alphabet, k=k, n_branches=nb, T=T, P=P_thr, rows=rows)
    f.n_with_code = sum(1 for r in reads if any(_alts(alphabet, ch) is not None for ch in r))
    f.sites, f.census = census(f)
    return f


# ---- the census: the kernel's predicates restated, on the final database and reads ----
def census(f):
    """(sites, counts): per read the list of its sites -- dict(j, p, W, rows=[(word, branches) or None per alternative word], path, ...) --
    and a Counter of the class names of CLASSES; a site counts once in every class it belongs to, a read once in every per-read class"""
    k, alphabet, nb, rows = f.k, f.alphabet, f.nb, f.pydb["rows"]
    s_win = min(f.s_win, nb)
    n_win = (nb + s_win - 1) // s_win
    seen = collections.Counter()
    all_sites = []
    for read in f.reads:
        R = len(read)
        kms, alts = _kmers(alphabet, k, read)
        code_at = sorted(alts)
        per_read = set()
        sites = []
        if R < k:
            per_read.add("R<k")
        if R == k and code_at:
            per_read.add("R==k")
        if code_at and len(code_at) == R and R >= k:
            per_read.add("only_codes")
        gaps = [b - a for a, b in zip(code_at, code_at[1:])]
        if any(g < k for g in gaps) and len(code_at) == 2:
            per_read.add("codes<k_apart")
        if gaps and all(g >= k for g in gaps):
            per_read.add("codes>=k_apart")
        run = best = 0
        for i in range(R):
            run = run + 1 if i in alts else 0
            best = max(best, run)
        if best > k and best < R:
            per_read.add("code_run>k")
        # the walk of place_ascii_kernel over the read (the same in every tree window): plain hits are listed, a code or the list's cap flushes them
        touched = {}       # branch -> {"plain", "amb"}
        plain_at = collections.defaultdict(list)  # branch -> the plain k-mers that list it
        cnt, before_first_code, first_code_met = 0, 0, False
        for j0 in range(0, len(kms), 64):
            block = range(j0, min(j0 + 64, len(kms)))
            p0 = j0
            amb_js = [j for j in block if kms[j][1]]
            for na in amb_js + [None]:
                stretch = range(p0, na if na is not None else block[-1] + 1)
                hits = [j for j in stretch if pyref.kmer_code(alphabet, kms[j][0]) in rows]
                if cnt + len(hits) > LIST_CAP - 1:
                    if cnt:
                        per_read.add("flush_at_cap")
                    cnt = 0
                cnt += len(hits)
                if not first_code_met:
                    before_first_code += len(hits)
                for j in hits:
                    row = rows[pyref.kmer_code(alphabet, kms[j][0])]
                    if len(row) > 64:
                        per_read.add("pending_row>64")
                    for b, _ in row:
                        touched.setdefault(b, set()).add("plain")
                        plain_at[b].append(j)
                if na is None:
                    break
                if not first_code_met and before_first_code:
                    h = before_first_code
                    per_read.add(f"hits_before_code={h}" if h < 192 else "hits_before_code>=192")
                first_code_met = True
                cnt = 0  # flush(): everything before the ambiguous k-mer is applied first
                km, ps = kms[na]
                if len(ps) > f.max_amb:
                    seen[f"skipped:{len(ps)}_codes"] += 1
                else:
                    words = _words(alphabet, km, ps, {p: alts[na + p] for p in ps})
                    got = [(w, tuple(b for b, _ in rows[w])) if w in rows else None for w in words]
                    s = dict(j=na, ps=ps, W=len(words), rows=got, codes=[na + p for p in ps])
                    counts = collections.Counter(b for g in got if g for b in g[1])
                    s["branches"] = set(counts)
                    longest = max([len(g[1]) for g in got[:4] if g] or [0])
                    if len(ps) == 2:
                        s["path"] = "general:two_codes"
                    elif len(words) > 4:
                        s["path"] = "general:W>4"
                    elif f.chunk < min(s_win, nb):
                        s["path"] = "general:chunks"
                    else:
                        s["path"] = "lane16" if longest <= 16 else "lane64" if longest <= 64 else "general:row>64"
                    lab = {s["path"], f"p={ps[0]}"}
                    if alphabet == 4 and 2 * ps[0] >= 32:  # the alternative's bits go into the high word of the k-mer code
                        lab.add("2p>=32")
                    if alphabet == 4 and len(ps) == 2 and 2 * ps[1] >= 32:
                        lab.add("second_code:2p>=32")
                    lab.add("W=" + "x".join(str(len(alts[na + p])) for p in ps))
                    if len(set(words)) < len(words):
                        lab.add("repeated_words")
                    missing = sum(1 for g in got if g is None)
                    lab.add(f"missing={missing}")
                    if missing >= 10:
                        lab.add("missing>=10")
                    if counts:
                        lab.add(f"shared={max(counts.values())}")
                        if any(b not in touched for b in counts):
                            lab.add("base=QT")
                        if any("plain" in touched.get(b, ()) for b in counts):
                            lab.add("touched_before_plain")
                        if any("amb" in touched.get(b, ()) for b in counts):
                            lab.add("touched_before_amb")
                    for c in s["codes"]:
                        for what, at in zip(_POSITIONS, (0, k - 1, 63, 64, 64 + k - 2, R - k, R - 1)):
                            if c == at:
                                lab.add(what)
                    for B in f.borders:
                        for what, at in (("at_lo-1", B - 1), ("at_lo", B), ("at_lo+1", B + 1)):
                            if at in counts:
                                lab.add(what)
                        sides = [{b >= B for b in g[1]} for g in got if g]  # one alternative lists a branch below the border, ANOTHER one above it
                        if any(i != j2 for i, x in enumerate(sides) if False in x for j2, y in enumerate(sides) if True in y):
                            lab.add("straddles_border")
                    if 1 in counts:
                        lab.add("first_branch")
                    if nb - 1 in counts:
                        lab.add("last_branch")
                    s["labels"] = lab
                    for b in counts:
                        touched.setdefault(b, set()).add("amb")
                    sites.append(s)
                p0 = na + 1
        for s in sites:
            if any(j > s["j"] for b in s["branches"] for j in plain_at.get(b, ())):
                s["labels"].add("touched_later_plain")
            for c in s["labels"]:
                seen[c] += 1
        for c in per_read:
            seen[c] += 1
        all_sites.append(sites)
    return all_sites, seen


def window_census(f, reported):
    """for trees in windows: per keep_at_most K, the reads whose K reported branches lie in three or more windows / all in the last one;
    reported: {K: the oracle's placements}"""
    s_win = min(f.s_win, f.nb)
    last = (f.nb - 1) // s_win
    seen = collections.Counter()
    for K, ref in reported.items():
        for r in range(len(f.reads)):
            n = int(ref["n_rows"][r])
            if n < K:
                continue
            wins = {int(b) // s_win for b in ref["branch"][r, :n]}
            if len(wins) >= 3:
                seen[f"top{K}_in_3_windows"] += 1
            if wins == {last}:
                seen[f"top{K}_in_last_window"] += 1
    return seen


def reads_array(reads):
    seq = np.frombuffer("".join(reads).encode(), np.uint8).copy()
    off = np.zeros(len(reads) + 1, np.uint64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return seq, off


def code_free(f, n, seed=5):
    """n reads of the family's alphabet without an ambiguity code: copies of planted reads with every code replaced by a plain symbol"""
    rng = np.random.default_rng(seed)
    letters = _letters(f.alphabet)
    out = []
    for i in range(n):
        r = f.reads[i % len(f.reads)]
        out.append("".join(ch if _alts(f.alphabet, ch) is None else letters[int(rng.integers(0, f.alphabet))] for ch in r))
    return out


# ---- the oracle's view of a family, made once a process ----
@functools.lru_cache(maxsize=None)
def oracle_db(name):
    return O.OracleDB.from_synth(family(name).sdb)


@functools.lru_cache(maxsize=None)
def oracle_place(name, K, mode):
    f = family(name)
    return oracle_db(name).place(f.seq, f.off, keep_at_most=K, keep_factor=keep_factor(K), amb_mode=GU.AMB[mode])


def entries_seen(f, ref):
    """(needed, seen): the (row length, alternative, entry index) triples of the alternative rows of f's sites -- every entry index of
    every (length, alternative) that occurs -- and those whose branch is among the rows `ref` (the oracle's placements) reports for a
    read that holds the site.  Alternatives beyond the fourth count for codes with twenty only."""
    Wmax = 4 if f.alphabet == 4 else 20
    needed = {(c, a, e) for a in range(Wmax) for c in planted_lengths(f, a) for e in range(c)}
    seen = set()
    for r, sites in enumerate(f.sites):
        reported = set(int(b) for b in ref["branch"][r, :int(ref["n_rows"][r])])
        for s in sites:
            for a, g in enumerate(s["rows"][:Wmax]):
                if g is not None:
                    seen.update((len(g[1]), a, e) for e, b in enumerate(g[1]) if b in reported)
    return needed, seen & needed


def planted_lengths(f, a):
    """the row lengths the recipe gives alternative number a of a code (rows of other lengths are inherited from words met before)"""
    return LENGTHS if a < 4 and (f.alphabet == 4 or a < 2) else X_LENGTHS
