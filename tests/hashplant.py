"""Planted probe chains for the hashed k-mer table (RK_TABLE_HASH: open addressing, linear probing, 16-byte slots {key + 1, descriptor},
load <= 0.5, built on the host by build_table in rk_engine.hip) -- shared by tests/test_hash_table_shapes.py (no GPU) and
tests/test_gpu_hash_probe.py (GPU).

Random keys at load 0.5 end almost every probe in its home slot.  The keys made here all have their home in the last eighth of the
table: they form ONE cluster that runs past the last slot and on from slot 0, so that a lookup walks up to half the table, most walks
step from the last slot to slot 0, and -- with 64-bit keys -- keys whose `key + 1` agree in the low word, or have a zero low word, sit
on each other's probe paths.  Everything here restates the table's definition in numpy; nothing is imported from the engine but the
image file it writes (table_of_image)."""
import functools

import numpy as np

import rappas_amd as ra
from rappas_amd import synth

M64 = (1 << 64) - 1
LOW = np.uint64(0xFFFFFFFF)
ALIAS_BIT = 1 << 32  # c and c ^ ALIAS_BIT: key + 1 equal in the low word, different in the high one (the low word of c is not all ones)


def mix64(x):
    """numpy twin of mix64 in rk_device.h (the finaliser of MurmurHash3), on uint64 arrays"""
    x = np.array(x, dtype=np.uint64, ndmin=1)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    return x


def home(codes, slots):
    return (mix64(codes) & np.uint64(slots - 1)).astype(np.int64)


def bits_of(alphabet):
    return 2 if alphabet == 4 else 5


def random_codes(alphabet, k, n, rng):
    """n random key codes: symbol i at bits [i * b, (i + 1) * b), amino-acid digits below 20"""
    b = bits_of(alphabet)
    digits = rng.integers(0, alphabet, (n, k)).astype(np.uint64)
    return (digits << (np.uint64(b) * np.arange(k, dtype=np.uint64))).sum(1, dtype=np.uint64)


def valid_code(alphabet, k, codes):
    codes = np.asarray(codes, dtype=np.uint64)
    b = bits_of(alphabet)
    ok = (codes >> np.uint64(b * k)) == 0 if b * k < 64 else np.ones(len(codes), bool)
    for i in range(k):
        ok &= ((codes >> np.uint64(b * i)) & np.uint64((1 << b) - 1)) < np.uint64(alphabet)
    return ok


def digits_of(alphabet, k, code):
    b = bits_of(alphabet)
    return [(int(code) >> (b * i)) & ((1 << b) - 1) for i in range(k)]


def dense_index(alphabet, k, codes):
    """the index of a code among all sigma^k k-mers (DNA: the code itself; amino acids: its digits in base 20)"""
    codes = np.asarray(codes, dtype=np.uint64)
    if alphabet == 4:
        return codes
    b = np.uint64(bits_of(alphabet))
    return sum(((codes >> (b * np.uint64(i))) & np.uint64(31)) * np.uint64(20 ** i) for i in range(k))


def band(slots):
    """the last eighth of the table"""
    return slots - max(1, slots // 8)


def _band_codes(alphabet, k, slots, n, rng, also=None):
    """n distinct codes whose home lies in the last eighth (`also`: a further condition on an array of codes)"""
    lo = band(slots)
    if alphabet == 4 and k <= 8:
        pool = np.arange(4 ** k, dtype=np.uint64)
        pool = pool[home(pool, slots) >= lo]
        if also is not None:
            pool = pool[also(pool)]
        assert len(pool) >= n, (len(pool), n)
        return rng.choice(pool, size=n, replace=False)
    got = np.zeros(0, dtype=np.uint64)
    while len(got) < n:
        c = random_codes(alphabet, k, 64 * n + 4096, rng)
        c = c[home(c, slots) >= lo]
        if also is not None:
            c = c[also(c)]
        got = np.concatenate([got, c])
        _, first = np.unique(got, return_index=True)
        got = got[np.sort(first)]
    return got[:n]


def plant_keys(alphabet, k, slots, seed):
    """slots / 2 key codes (build_table sizes the table at exactly `slots` for that count: load 0.5) whose home slot
    mix64(code) & (slots - 1) lies in the last eighth of the table: one cluster that runs past the end and on from slot 0"""
    assert slots >= 16 and slots & (slots - 1) == 0
    return _band_codes(alphabet, k, slots, slots // 2, np.random.default_rng(seed))


def plant_alias_keys(alphabet, k, slots, seed):
    """64-bit keys (bits * k > 32) in pairs c, c ^ (1 << 32) with BOTH homes in the last eighth.  A quarter of the pairs is stored whole;
    of the others one member is stored and the other -- absent -- is returned for the reads to ask for.  -> (keys [slots / 2], absent
    partners)"""
    assert bits_of(alphabet) * k > 33
    rng = np.random.default_rng(seed)
    n = slots // 2
    lo = band(slots)

    def pair_ok(c):
        p = c ^ np.uint64(ALIAS_BIT)
        return (home(p, slots) >= lo) & valid_code(alphabet, k, p) & ((c & LOW) != LOW) & ((c & np.uint64(ALIAS_BIT)) == 0)

    n_whole = n // 4  # pairs stored whole: 2 keys each
    firsts = _band_codes(alphabet, k, slots, n_whole + (n - 2 * n_whole), rng, also=pair_ok)
    whole, single = firsts[:n_whole], firsts[n_whole:]
    flip = rng.random(len(single)) < 0.5  # which member of a half-stored pair is the stored one
    stored = np.where(flip, single ^ np.uint64(ALIAS_BIT), single)
    keys = np.concatenate([whole, whole ^ np.uint64(ALIAS_BIT), stored])
    assert len(keys) == n and len(np.unique(keys)) == n
    return rng.permutation(keys), stored ^ np.uint64(ALIAS_BIT)


def zero_low_codes(k=17):
    """DNA k = 17: sixteen G's and base d -- code 0xFFFFFFFF | d << 32, whose key + 1 has a zero low word"""
    assert k == 17
    return np.array([0xFFFFFFFF | (d << 32) for d in range(4)], dtype=np.uint64)


def plant_zero_low_keys(slots, seed, k=17):
    """DNA k = 17, slots / 2 keys: the four codes whose key + 1 has a zero low word, for each of them three keys whose home is its home
    or the slot before -- they queue up through its slot -- and keys with their home in the last eighth for the rest (where a special
    code's home lies inside their cluster, the cluster's keys queue up through its slot too)"""
    rng = np.random.default_rng(seed)
    n = slots // 2
    special = zero_low_codes(k)
    per = 3
    keys = [special]
    for h in home(special, slots):
        near = np.zeros(0, dtype=np.uint64)
        while len(near) < per:
            c = random_codes(4, k, 64 * slots, rng)
            d = (int(h) - home(c, slots)) & (slots - 1)
            near = np.unique(np.concatenate([near, c[(d <= 1) & ((c & LOW) != LOW)]]))
        keys.append(rng.permutation(near)[:per])
    keys = np.concatenate(keys)
    rest = _band_codes(4, k, slots, n - len(keys), rng, also=lambda c: ~np.isin(c, keys) & ((c & LOW) != LOW))
    keys = np.concatenate([keys, rest])
    assert len(keys) == n and len(np.unique(keys)) == n
    return rng.permutation(keys)


def rows_db(alphabet, k, n_branches, keys, seed, min_row=1, max_row=24, lens=None):
    """a row per key: random distinct branches 1 .. n_branches - 1, scores thr_log10 * U[0, 1) in float32 -- sums of them tie by rounding
    only (a read or two in a batch of 300-symbol reads), so the order among equal scores plays next to no part.  lens: the rows' lengths instead of min_row .. max_row"""
    rng = np.random.default_rng(seed)
    keys = np.asarray(keys, dtype=np.uint64)
    if lens is None:
        lens = rng.integers(min_row, min(max_row, n_branches - 1) + 1, size=len(keys))
    lens = np.asarray(lens, dtype=np.int64)
    off = np.zeros(len(keys) + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    br = np.concatenate([rng.choice(n_branches - 1, size=int(n), replace=False) + 1 for n in lens]).astype(np.uint16)
    thr, t = synth.thresholds(1.5, alphabet, k)
    sc = (t * rng.random(len(br), dtype=np.float32)).astype(np.float32)
    return synth.SynthDB(alphabet, k, n_branches, thr, t, keys, off, br, sc, seed)


def save_image(sdb, path, table_mode=ra.RK_TABLE_HASH):
    ra.save_db_image(str(path), sdb.alphabet, sdb.k, sdb.n_branches, sdb.thr_log10, sdb.thr, sdb.key_codes, sdb.row_offsets, sdb.branch_ids,
                     sdb.scores, table_mode=table_mode)


TABLE_AT = 4096  # the table section of an image file (rk_image_impl.h: sections start on 4 096-byte boundaries, the table first)


def table_bytes_of_image(path):
    """(rk_db_info, the table section's bytes) of a file written by ra.save_db_image"""
    info, _ = ra.db_image_info(str(path))
    with open(path, "rb") as f:
        f.seek(TABLE_AT)
        raw = f.read(int(info.table_bytes))
    assert len(raw) == info.table_bytes
    return info, raw


def table_of_image(path):
    """(rk_db_info, table u64 [table_slots, 2] = {key + 1, descriptor}) of a hashed image"""
    info, raw = table_bytes_of_image(path)
    assert info.table_mode == ra.RK_TABLE_HASH and info.table_bytes == 16 * info.table_slots
    return info, np.frombuffer(raw, dtype="<u8").reshape(int(info.table_slots), 2).copy()


def probe(table, codes):
    """the plain linear probe of every code at once: from its home slot on until its key + 1 or an empty slot is met.
    -> dict of arrays per code: home, slot (where the walk ended), steps (slots walked beyond the home), found, wrapped (stepped from
    the last slot to slot 0), alias (met a slot with the low word of its key + 1 and another high word), zero_low (walked on from an
    occupied slot whose key + 1 has a zero low word)"""
    codes = np.asarray(codes, dtype=np.uint64)
    slots = len(table)
    stored = table[:, 0]
    want = codes + np.uint64(1)
    h0 = home(codes, slots)
    n = len(codes)
    res = dict(home=h0, slot=h0.copy(), steps=np.zeros(n, np.int64), found=np.zeros(n, bool), wrapped=np.zeros(n, bool),
               alias=np.zeros(n, bool), zero_low=np.zeros(n, bool))
    live = np.arange(n)
    h = h0.copy()
    for _ in range(slots + 1):
        if not len(live):
            break
        key = stored[h[live]]
        hit, empty = key == want[live], key == 0
        res["found"][live[hit]] = True
        res["slot"][live] = h[live]
        on = ~hit & ~empty
        res["alias"][live[on & ((key & LOW) == (want[live] & LOW))]] = True
        res["zero_low"][live[on & ((key & LOW) == 0)]] = True
        live = live[on]
        res["wrapped"][live[h[live] == slots - 1]] = True
        h[live] = (h[live] + 1) & (slots - 1)
        res["steps"][live] += 1
    assert not len(live), "a probe went round the whole table"
    return res


def census(table, keys, queries):
    """what the table and a set of query codes hold of the planted shapes.  Per key (keys: displacement from home, stored at a lower
    slot than its home) and per query code (queries: the arrays of probe()), and the counts the tests assert on"""
    keys = np.asarray(keys, dtype=np.uint64)
    queries = np.unique(np.asarray(queries, dtype=np.uint64))
    slots = len(table)
    pk = probe(table, keys)
    assert pk["found"].all(), "a key cannot be reached from its home before an empty slot"
    pq = probe(table, queries)
    is_key = np.isin(queries, keys)
    assert np.array_equal(pq["found"], is_key)
    absent = ~pq["found"]
    # (an absent code that starts inside a cluster walks to the cluster's end: at 16 slots a walk of 8 is one through all of it)
    return dict(slots=slots, n_keys=len(keys), occupied=int((table[:, 0] != 0).sum()),
                displacement=pk["steps"], below_home=pk["slot"] < pk["home"],
                max_displacement=int(pk["steps"].max()), keys_below_home=int((pk["slot"] < pk["home"]).sum()),
                queries=queries, probe=pq, n_queries=len(queries),
                absent_long=int((absent & (pq["steps"] >= min(8, slots // 2))).sum()),
                longest_absent=int(pq["steps"][absent].max()) if absent.any() else 0,
                wrapped=int(pq["wrapped"].sum()), alias=int(pq["alias"].sum()),
                keys_behind_zero_low=int(pk["zero_low"].sum()), queries_behind_zero_low=int((pq["zero_low"] & pq["found"]).sum()))


def letters_of(alphabet):
    """state -> character: DNA ATCG for 0..3 (the first character in the lowest bits), amino acids in the state order of rappas_place.h"""
    return np.frombuffer(b"ATCG" if alphabet == 4 else b"RHKDESTNQCGPAILMFWYV", dtype=np.uint8)


def planted_reads(alphabet, k, codes, n, L, seed, amb=False, always=()):
    """n random reads of L symbols with two to four of `codes` (as many as fit: one when L < 2 k) written in, each at a random offset of
    its own stretch of the read.  always: codes dealt out in turn, one to each read's first stretch, so that each of them is asked for.
    amb: one symbol of one written k-mer is replaced by the character that stands for every state (N / X) -- the code is then one of
    the alternatives, the others are codes that are (nearly all) absent and walk.  -> (seq u8, off u64)"""
    rng = np.random.default_rng(seed)
    letters = letters_of(alphabet)
    st = rng.integers(0, alphabet, (n, L))
    seq = letters[st]
    codes = [int(c) for c in codes]
    always = [int(c) for c in always]
    for r in range(n):
        m = max(1, min(int(rng.integers(2, 5)), L // k))
        width = L // m
        hit = int(rng.integers(0, m))
        for j in range(m):
            code = always[r % len(always)] if always and j == 0 else codes[int(rng.integers(0, len(codes)))]
            at = j * width + int(rng.integers(0, width - k + 1))
            seq[r, at:at + k] = letters[digits_of(alphabet, k, code)]
            if amb and j == hit:
                seq[r, at + int(rng.integers(0, k))] = ord("N") if alphabet == 4 else ord("X")
    return np.ascontiguousarray(seq.reshape(-1)), np.arange(n + 1, dtype=np.uint64) * np.uint64(L)


def codes_of_reads(alphabet, k, seq, off):
    """per read the key codes its k-mers make the device look up (u64 arrays): the code of every k-mer of unambiguous characters, and
    for a k-mer with ONE N / X every alternative's code (the engine's ambiguity kernel looks each of them up; k-mers with more, and
    reads with any other character, give nothing)"""
    b = bits_of(alphabet)
    table = np.full(256, 255, dtype=np.uint8)
    table[letters_of(alphabet)] = np.arange(alphabet)
    table[ord("N") if alphabet == 4 else ord("X")] = 254
    out = []
    for r in range(len(off) - 1):
        st = table[seq[int(off[r]):int(off[r + 1])]].astype(np.uint64)
        if len(st) < k or (st == 255).any():
            out.append(np.zeros(0, dtype=np.uint64))
            continue
        wild = st == 254
        st[wild] = 0
        Q = len(st) - k + 1
        c = np.zeros(Q, dtype=np.uint64)
        n_wild = np.zeros(Q, dtype=np.int64)
        at = np.zeros(Q, dtype=np.uint64)  # the wild symbol's place in the k-mer
        for i in range(k):
            c |= st[i:i + Q] << np.uint64(b * i)
            n_wild += wild[i:i + Q]
            at[wild[i:i + Q]] = i
        one = n_wild == 1
        alts = (c[one][:, None] | (np.arange(alphabet, dtype=np.uint64)[None, :] << (np.uint64(b) * at[one])[:, None])).reshape(-1)
        out.append(np.concatenate([c[n_wild == 0], alts]))
    return out


# ---- the planted tables: name -> (alphabet, k, slots, how the keys are made) ----
TABLES = {
    "dna6_16": (4, 6, 16, "band"), "dna6_256": (4, 6, 256, "band"), "dna8_1024": (4, 8, 1024, "band"),
    "dna17_16": (4, 17, 16, "band"), "dna17_1024": (4, 17, 1024, "band"),
    "aa7_16": (20, 7, 16, "band"), "aa7_256": (20, 7, 256, "band"),
    # 64-bit keys: pairs that differ in bit 32 only, and the codes whose key + 1 has a zero low word
    "dna17_alias": (4, 17, 256, "alias"), "aa7_alias": (20, 7, 256, "alias"),
    "dna17_zero_low": (4, 17, 256, "zero_low"),
}
SEED = 20
N_READS = 200


@functools.lru_cache(maxsize=None)
def keys_of(name):
    """(keys, absent codes the reads must ask for) of a planted table"""
    alphabet, k, slots, how = TABLES[name]
    if how == "alias":
        return plant_alias_keys(alphabet, k, slots, SEED)
    if how == "zero_low":
        return plant_zero_low_keys(slots, SEED, k), np.zeros(0, dtype=np.uint64)
    return plant_keys(alphabet, k, slots, SEED), np.zeros(0, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def database(name, n_branches=399, min_row=1, max_row=24):
    alphabet, k, slots, how = TABLES[name]
    return rows_db(alphabet, k, n_branches, keys_of(name)[0], SEED + 1, min_row, max_row)


@functools.lru_cache(maxsize=None)
def reads(name, L, amb=False, n=N_READS):
    """the reads of a planted table: random symbols around two to four key k-mers; the 64-bit shapes' special codes -- the absent
    partners, the zero-low-word keys and the keys queued behind them -- go to the reads in turn"""
    alphabet, k, slots, how = TABLES[name]
    keys, partners = keys_of(name)
    always = ()
    if how == "alias":  # (a read too short for two k-mers keeps a key)
        always = np.concatenate([partners, keys]) if L >= 2 * k else keys
    elif how == "zero_low":
        always = keys
    return planted_reads(alphabet, k, keys, n, L, SEED + 2 + L, amb=amb, always=tuple(int(c) for c in always))


def assert_table(info, table, sdb, unit=16):
    """what build_table promises of any hashed table: slots as the header says and the load <= 0.5 rule gives, n_keys of them occupied,
    every key reachable from its home before an empty slot, its descriptor's length field the row length rounded up to 16 (32 in a
    large-tree image), no descriptor shared"""
    n = sdb.n_keys
    slots = 16
    while slots < 2 * n:
        slots *= 2
    assert info.table_slots == slots == len(table) and info.n_keys == n
    assert int((table[:, 0] != 0).sum()) == n
    p = probe(table, sdb.key_codes)
    assert p["found"].all()
    desc = table[p["slot"], 1]
    want_len = (np.diff(sdb.row_offsets.astype(np.int64)) + unit - 1) // unit * unit
    assert np.array_equal((desc & np.uint64((1 << 24) - 1)).astype(np.int64), want_len)
    assert len(np.unique(desc)) == n and (table[table[:, 0] == 0, 1] == 0).all()
    return p


def assert_planted(name, table, sdb, seq, off, what=""):
    """the conditions that keep a planted case from being a random-key test: asserted by the CPU tests and again by every GPU case
    before it places anything.  -> the census of the table and of the codes the reads make the device look up"""
    alphabet, k, slots, how = TABLES[name]
    keys = sdb.key_codes
    per_read = codes_of_reads(alphabet, k, seq, off)
    c = census(table, keys, np.concatenate(per_read))
    n = c["n_keys"]
    where = f"{name} {what}: " + str({f: v for f, v in c.items() if isinstance(v, int)})
    assert c["occupied"] == n == slots // 2, where
    if how == "band":
        assert c["max_displacement"] >= n // 2, where
        assert c["keys_below_home"] >= n // 2, where
    long_reads = [q for r, q in enumerate(per_read) if int(off[r + 1] - off[r]) >= 30]
    if long_reads:
        assert np.mean([np.isin(q, keys).any() for q in long_reads]) >= 0.9, where
        # absent codes that walk 8 slots or more (16 slots: 8 is a walk through the whole cluster): >= 5 % of the batch's distinct codes
        assert c["absent_long"] >= 0.05 * c["n_queries"], where
        if how == "band":
            assert c["wrapped"] >= 100, where
    if how == "alias":
        assert c["alias"] >= 20, where
    if how == "zero_low":
        assert c["keys_behind_zero_low"] >= 1 and c["queries_behind_zero_low"] >= 1, where
    return c


# ---- the compact direct table (RK_TABLE_DIRECT), restated: both block forms and the layout rule ----
def decode_compact(raw, space):
    """(first unit, units) u64 [space] of every dense k-mer index, decoded from the table section of an image: 16-byte blocks
    {u32 first unit, 12 x u8 units} or -- at half the size -- {u32 first unit, 24 x u4 units, the low nibble first}; an absent code
    (0 units) decodes to (0, 0).  Also returns which form it is ("bytes" / "nibbles")"""
    blocks = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 16)
    if len(blocks) == (space + 11) // 12:
        form = "bytes"
        units = blocks[:, 4:].astype(np.uint64)
    else:
        assert len(blocks) == (space + 23) // 24, (len(blocks), space)
        form = "nibbles"
        units = np.stack([blocks[:, 4:] & 15, blocks[:, 4:] >> 4], axis=2).reshape(len(blocks), 24).astype(np.uint64)
    base = np.frombuffer(blocks[:, :4].tobytes(), dtype="<u4").astype(np.uint64)
    first = base[:, None] + np.cumsum(units, axis=1) - units
    first[units == 0] = 0
    return first.reshape(-1)[:space], units.reshape(-1)[:space], form


def compact_layout(sdb):
    """the layout rule: rows in ascending dense order from unit 1 on (unit 0 is reserved), ceil(len / 16) units each, absent codes 0"""
    assert sdb.alphabet == 4  # (dense index = code)
    space = 4 ** sdb.k
    units = np.zeros(space, dtype=np.uint64)
    units[sdb.key_codes.astype(np.int64)] = (np.diff(sdb.row_offsets.astype(np.int64)) + 15) // 16
    first = np.uint64(1) + np.cumsum(units) - units
    first[units == 0] = 0
    return first, units


EDGE_CODES = np.arange(12, 24, dtype=np.uint64)  # one whole block of the byte form


@functools.lru_cache(maxsize=None)
def compact_edge_db(longest=4080):
    """the compact table's upper edge: DNA k = 6 on 9 001 branches, codes 12 .. 23 -- block 1 of the byte form -- with 4 080 entries each
    (255 units: twelve counts of 255 in one block), their neighbours 11 and 24 absent, 700 further rows of 200 .. 399 entries.  longest = 4 081: the first of the twelve
    rows has one entry more (256 units), and the table must become RK_TABLE_DIRECT8"""
    rng = np.random.default_rng(4080)
    others = rng.choice(np.setdiff1d(np.arange(4 ** 6, dtype=np.uint64), np.arange(11, 25, dtype=np.uint64)), size=700, replace=False)
    keys = np.concatenate([EDGE_CODES, others])
    lens = np.concatenate([[longest] + [4080] * 11, rng.integers(200, 400, size=700)])
    order = rng.permutation(len(keys))
    return rows_db(4, 6, 9001, keys[order], 4081, lens=lens[order])
