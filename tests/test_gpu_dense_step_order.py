"""GPU (-m gpu): the order of the LDS operations of the dense 24-entry accumulate steps (units_run<..., D24> in rk_kernels.hip, run
by place_packed16_kernel<..., ROW24>; DESIGN.md 4.1a "Round 10").  Step n + 1 reads the score words that step n has just written
whenever two consecutive rows hold a branch in common, from whatever lane and slot the branch has in either row; a step loop whose
reads overtook the writes in front of them would lose an update exactly there.  The inputs plant that by construction: every k-mer
is present, every row holds the first n of the same 48 branches (branch 0 and branch 1 022 among them), rotated by an amount of its
own, so two consecutive rows of one unit always share the whole shorter row, at other entry positions -- other lanes, and the first
against the second slot of a lane -- and a unit of a 25- or 48-entry row shares with its neighbour in most cases (checked: at least
85 % of all steps behind a step of another row meet a word that step wrote).  Row lengths are 1, 8, 9, 16, 17, 24, 25 and 48;
the reads' unit counts are every value from 1 to 2U + 7 (the main block alone, each of the one-, two- and three-pair tails, lists
shorter than the ring) as the largest of a tile and beside longer reads, and tiles mix four reads of very different length.  Each
case first checks those preconditions on the CPU with a numpy twin of the unit layout.  Bar: the oracle's placements for every
read -- flags, n_rows, branches, score bits, LWR -- written into 0xFF-filled result buffers, so a read that was never placed fails;
and the canonical 16-entry units' results, bit for bit.  Once with every score at or above the threshold (`mono`), once with a
share below it."""
import numpy as np
import pytest

import rappas_amd as ra
from oracle import oracle as O
from rappas_amd import synth
from tests.util import compare_with_oracle

pytestmark = pytest.mark.gpu

ROW_LENS = [1, 8, 9, 16, 17, 24, 25, 48]
N_BRANCHES = 1023
POOL = 48   # branches every row draws on (the longest row holds them all)
U = 8       # the ring (RK_RING)
UNIT = 24   # entries of a dense unit
K_BEST = 7


def rows_db(alphabet, k, seed, below_threshold):
    """-> (SynthDB, units[space], rows): the row of k-mer i has ROW_LENS[i % 8] entries, pool[(j + rot_i) % n] in entry j"""
    rng = np.random.default_rng(seed)
    space = alphabet ** k
    assert space % len(ROW_LENS) == 0
    rl = np.resize(np.asarray(ROW_LENS, dtype=np.int64), space)
    pool = np.concatenate([[0, N_BRANCHES - 1], 1 + rng.choice(N_BRANCHES - 2, size=POOL - 2, replace=False)])
    rng.shuffle(pool)
    rot = rng.integers(0, POOL, size=space)
    rows = [pool[(np.arange(n) + r) % n] for n, r in zip(rl.tolist(), rot.tolist())]
    off = np.zeros(space + 1, dtype=np.uint64)
    np.cumsum(rl, out=off[1:])
    br = np.concatenate(rows).astype(np.uint16)
    thr, t = synth.thresholds(1.5, alphabet, k)
    sc = (t * rng.random(len(br), dtype=np.float32)).astype(np.float32)
    low = rng.random(len(br)) < below_threshold
    sc[low] = (t * (1.0 + rng.random(int(low.sum()), dtype=np.float32))).astype(np.float32)
    assert bool((sc < t).any()) == (below_threshold > 0)
    key_codes = synth.dense_to_code(alphabet, k, np.arange(space, dtype=np.uint64))
    return synth.SynthDB(alphabet, k, N_BRANCHES, thr, t, key_codes, off, br, sc, seed), (rl + UNIT - 1) // UNIT, rows


def kmers_of(alphabet, k, s):
    """dense k-mer indices of a read's positions, in order (first symbol = lowest digit, as synth.codes_of_reads)"""
    s = np.asarray(s, dtype=np.int64)
    q = len(s) - k + 1
    idx = np.zeros(max(q, 0), dtype=np.int64)
    for i in range(k):
        idx += s[i:i + q] * alphabet ** i
    return idx


def read_of_units(rng, alphabet, k, units, m, max_len):
    """a random read whose rows hold exactly m units (m = 0: one symbol short of a k-mer)"""
    if m == 0:
        return rng.integers(0, alphabet, size=k - 1)
    while True:
        q = int(rng.integers((m + 1) // 2, m + 1))
        s = rng.integers(0, alphabet, size=q + k - 1)
        if len(s) <= max_len and units[kmers_of(alphabet, k, s)].sum() == m:
            return s


def planted_tiles(rng, long_units):
    """unit counts of the four reads of each tile; `long_units` stands for a read of full length"""
    tiles = []
    for m in range(1, 2 * U + 8):  # the largest count of a tile is every value 1 .. 2U + 7, in every group of the wave
        tiles.append([m] * 4)
        others = [int(x) for x in rng.integers(0, m + 1, size=3)]
        for g in range(4):
            tiles.append(others[:g] + [m] + others[g:])
    for m in range(1, 2 * U + 8):  # ... and each of them beside reads of very different length
        tiles.append([m, long_units, 1, (m * 5) % 23 + 1])
        tiles.append([long_units, 2, m, 0])
    tiles += [[1, 2 * U + 7, long_units, U], [long_units, 1, 2 * U, 3], [U - 2, long_units, 2 * U + 1, 1], [long_units] * 4]
    pool = np.concatenate([np.arange(0, 2 * U + 8), np.full(8, long_units)])
    for _ in range(120):
        tiles.append([int(x) for x in rng.choice(pool, size=4)])
    return tiles


def assert_hazard_planted(alphabet, k, rows, states):
    """Twin of the unit layout: entry e of a unit is lane e (first slot) for e < 16 and lane e - 16 (second slot) above.  Every step
    that follows a step of another row must meet a word that step wrote; over the reads a shared branch must come from another lane,
    from the second slot after the first and from the first after the second."""
    def where(row, unit):
        ent = row[unit * UNIT:(unit + 1) * UNIT]
        return {int(b): (e % 16, e // 16) for e, b in enumerate(ent.tolist())}
    other_lane = first_to_second = second_to_first = pairs = met = 0
    for s in states:
        idx = kmers_of(alphabet, k, s)
        for a, b in zip(idx[:-1].tolist(), idx[1:].tolist()):
            wa, wb = where(rows[a], (len(rows[a]) - 1) // UNIT), where(rows[b], 0)  # the last unit of a row, the first of the next
            shared = set(wa) & set(wb)
            # a row of one unit holds the first n branches: two such rows share the shorter one.  A unit of a 25- or 48-entry row holds
            # 1 or 24 of its branches, which the rotation may leave outside a short row next to it.
            assert shared or len(rows[a]) > UNIT or len(rows[b]) > UNIT, (a, b)
            pairs += 1
            met += bool(shared)
            other_lane += any(wa[x][0] != wb[x][0] for x in shared)
            first_to_second += any(wa[x][1] == 0 and wb[x][1] == 1 for x in shared)
            second_to_first += any(wa[x][1] == 1 and wb[x][1] == 0 for x in shared)
    assert pairs > 1000 and met >= 0.85 * pairs and other_lane > pairs // 2 and first_to_second > pairs // 50 and second_to_first > pairs // 50, \
        (pairs, met, other_lane, first_to_second, second_to_first)
    return pairs, met, other_lane, first_to_second, second_to_first


def place_into_filled_buffers(db, seq, off, K=K_BEST):
    """through the entry point that takes per-read lengths (and the packer's flags)"""
    import torch
    pp = ra.PlacementProcess(db)
    packed, lens, flags = pp.pack_reads_host(seq, off)
    n = len(off) - 1
    dev = torch.device("cuda", 0)
    out = dict(n_rows=torch.full((n,), 0xFF, dtype=torch.uint8, device=dev),
               branch=torch.full((n, K), -1, dtype=torch.int16, device=dev),
               score=torch.full((n, K), -1, dtype=torch.int32, device=dev).view(torch.float32),
               lwr=torch.full((n, K), -1, dtype=torch.int64, device=dev).view(torch.float64),
               flags=torch.full((n,), -1, dtype=torch.int32, device=dev))
    pp.place_packed(torch.from_numpy(packed.view(np.int32)).to(dev), lens=torch.from_numpy(lens.view(np.int32)).to(dev),
                    flags_in=torch.from_numpy(flags.view(np.int32)).to(dev), out=out, keepAtMost=K)
    torch.cuda.synchronize()
    o = {f: t.cpu().numpy() for f, t in out.items()}
    unwritten = np.nonzero((o["n_rows"] == 0xFF) | (o["flags"] == -1))[0]
    assert len(unwritten) == 0, f"{len(unwritten)} of {n} reads never written (first: {unwritten[:8]})"
    return ra.Placements(o["n_rows"], o["branch"].view(np.uint16), o["score"], o["lwr"], o["flags"].view(np.uint32), {}), pp.ns_bound


@pytest.mark.parametrize("alphabet,k,L", [(4, 5, 150), (20, 3, 100)], ids=["dna", "aa"])
@pytest.mark.parametrize("below_threshold", [0.0, 0.3], ids=["mono", "below_threshold"])
def test_consecutive_rows_over_the_same_words(dev_lib, monkeypatch, alphabet, k, L, below_threshold):
    sdb, units, rows = rows_db(alphabet, k, seed=1001 + alphabet, below_threshold=below_threshold)
    rng = np.random.default_rng(1002 + alphabet)
    long_units = -1  # marks a read of L symbols in the tile lists
    tiles = planted_tiles(rng, long_units)
    states = [rng.integers(0, alphabet, size=L) if m == long_units else read_of_units(rng, alphabet, k, units, m, L) for t in tiles for m in t]
    n = len(states)
    assert n < 32768  # (a batch this small keeps its order: tile t is reads 4t .. 4t + 3)
    total = np.asarray([units[kmers_of(alphabet, k, s)].sum() for s in states]).reshape(-1, 4)
    lens = np.asarray([len(s) for s in states]).reshape(-1, 4)
    assert set(range(1, 2 * U + 8)) <= set(total.max(axis=1).tolist())      # every list length as a tile's longest ...
    assert set(range(1, 2 * U + 8)) <= set(total[total.max(axis=1) > 4 * U].reshape(-1).tolist())  # ... and beside a long read
    assert (lens.max(axis=1) >= 10 * np.maximum(lens.min(axis=1), 1)).sum() >= 2 * U + 7  # very different lengths in one tile
    assert_hazard_planted(alphabet, k, rows, states[::7])
    letters = synth.DNA_LETTERS if alphabet == 4 else synth.AA_LETTERS
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in states], out=off[1:])
    seq = np.ascontiguousarray(letters[np.concatenate(states)])
    odb = O.OracleDB.from_synth(sdb)
    monkeypatch.delenv("RK_NO_DENSE_UNITS", raising=False)
    dense = ra.PhyloKmerDB.from_synth(sdb, device=0)
    monkeypatch.setenv("RK_NO_DENSE_UNITS", "1")
    canon = ra.PhyloKmerDB.from_synth(sdb, device=0)
    monkeypatch.delenv("RK_NO_DENSE_UNITS", raising=False)
    try:
        assert dense.kernel_name().startswith("place_packed16_kernel<") and "ROW24," in dense.kernel_name(), dense.kernel_name()
        assert "ROW24," not in canon.kernel_name(), canon.kernel_name()
        got, ns_bound = place_into_filled_buffers(dense, seq, off)
        ref = odb.place(seq, off, keep_at_most=K_BEST, keep_factor=0.01, ns_bound=ns_bound)
        st = compare_with_oracle(got, ref, odb, seq, off)  # every read: nothing sampled
        assert st["n"] == n and st["placed"] >= int((total.reshape(-1) > 0).sum()), st
        want, _ = place_into_filled_buffers(canon, seq, off)
        for f in ("n_rows", "branch", "flags"):
            assert np.array_equal(getattr(got, f), getattr(want, f)), f
        assert np.array_equal(got.score.view(np.uint32), want.score.view(np.uint32))
        assert np.array_equal(got.lwr.view(np.uint64), want.lwr.view(np.uint64))
    finally:
        dense.close()
        canon.close()
