"""GPU (-m gpu): the start and the end of the row ring of the dense 24-entry kernel (place_packed16_kernel<..., ROW24>; DESIGN.md 4.1a
"Round 9"): a tile's first U = 8 row gathers leave from inside the emit phase when, after the emit's first prefix scan (positions
0..63 of the four reads), every read of the tile holds at least 2U units and no more than its list takes, and from the flush otherwise;
the step loop leaves after an even number of steps once the tile's longest list is done.  Small DNA k = 5 databases on 1 023 branches whose reads put lists of every
length around U and 2U, multi-unit rows across the ring's two boundaries, reads shorter than k and missing reads into the tiles.
Each test first computes with a numpy twin of the first-scan rule (below 32 768 reads a batch keeps its order: tile t is reads
4t .. 4t + 3) how many of its tiles start the ring early and how many do not, and asserts that both kinds occur and that a tile with
exactly 2U units in one read and more in the others is among them -- a precondition on the inputs, checked on the CPU.  Bar: the
oracle's placements for every read, written into 0xFF-filled result buffers so that a read never written fails; and the canonical
16-entry units' results, bit for bit."""
import numpy as np
import pytest

import rappas_amd as ra
from oracle import oracle as O
from rappas_amd import synth

from tests.util import compare_with_oracle

pytestmark = pytest.mark.gpu

K_MER = 5
SPACE = 4 ** K_MER
N_BRANCHES = 1023
U = 8            # the ring (RK_RING)
UNIT = 24        # entries of a dense unit
FIRST_SCAN = 64  # positions the emit's first prefix scan covers
# what a read's list holds before it is flushed (rk_geometry.h, 1 023 branches in the 160 KiB of LDS of a CU: list_cap = 128 pairs of
# items, less 3U + 2 of slack); a first scan that counts more leaves the batch to the path that passes it through the list in parts
CAP_ITEMS = 2 * 128 - 3 * U - 2
K_BEST = 7


def make_db(units, seed, below_threshold=0.0):
    """units[i] = dense units of the row of k-mer i (0: the k-mer is absent); a row of n units holds 24 n - 4 entries on distinct
    random branches (branch 0 and branch 1 022 among them)"""
    rng = np.random.default_rng(seed)
    present = np.nonzero(units)[0]
    rl = (units[present].astype(np.int64) * UNIT - 4)
    off = np.zeros(len(present) + 1, dtype=np.uint64)
    np.cumsum(rl, out=off[1:])
    br = np.concatenate([rng.choice(N_BRANCHES, size=int(n), replace=False) for n in rl]).astype(np.uint16)
    br[0] = 0
    if N_BRANCHES - 1 not in br[:int(off[1])]:
        br[1] = N_BRANCHES - 1
    thr, t = synth.thresholds(1.5, 4, K_MER)
    sc = (t * rng.random(len(br), dtype=np.float32)).astype(np.float32)
    low = rng.random(len(br)) < below_threshold
    sc[low] = (t * (1.0 + rng.random(int(low.sum()), dtype=np.float32))).astype(np.float32)
    return synth.SynthDB(4, K_MER, N_BRANCHES, thr, t, synth.dense_to_code(4, K_MER, present.astype(np.uint64)), off, br, sc, seed)


def reads_from_states(states):
    """list of arrays of symbols 0..3 -> (seq, off)"""
    off = np.zeros(len(states) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in states], out=off[1:])
    flat = np.concatenate([np.asarray(s, dtype=np.int64) for s in states]) if len(states) else np.zeros(0, np.int64)
    return np.ascontiguousarray(synth.DNA_LETTERS[flat]), off


def unit_prefix(units, s):
    """units of the rows of a read's k-mer positions, in order (first symbol = lowest digit, as synth.codes_of_reads)"""
    s = np.asarray(s, dtype=np.int64)
    q = len(s) - K_MER + 1
    if q <= 0:
        return np.zeros(0, dtype=np.int64)
    idx = np.zeros(q, dtype=np.int64)
    for i in range(K_MER):
        idx += s[i:i + q] * 4 ** i
    return units[idx].astype(np.int64)


def tiles_of(units, states):
    """the numpy twin of the first-scan rule -> (early[t], first[t, 4], total[t, 4]); a missing read counts -1 units"""
    n = len(states)
    nt = (n + 3) // 4
    first = np.full(4 * nt, -1, dtype=np.int64)
    total = np.full(4 * nt, -1, dtype=np.int64)
    for r, s in enumerate(states):
        u = unit_prefix(units, s)
        first[r] = u[:FIRST_SCAN].sum()
        total[r] = u.sum()
    first, total = first.reshape(nt, 4), total.reshape(nt, 4)
    return (first >= 2 * U).all(axis=1) & (first <= CAP_ITEMS).all(axis=1), first, total


def assert_both_kinds(early, first):
    assert early.any() and (~early).any(), (int(early.sum()), len(early))
    edge = early & (first == 2 * U).any(axis=1) & ((first > 2 * U).sum(axis=1) == 3)
    assert edge.any(), "no tile with exactly 2U units in one read and more in the others"


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


class Engines:
    """the dense and the canonical handle of one database, and its oracle"""

    def __init__(self, sdb, monkeypatch):
        self.odb = O.OracleDB.from_synth(sdb)
        monkeypatch.delenv("RK_NO_DENSE_UNITS", raising=False)
        self.dense = ra.PhyloKmerDB.from_synth(sdb, device=0)
        monkeypatch.setenv("RK_NO_DENSE_UNITS", "1")
        self.canon = ra.PhyloKmerDB.from_synth(sdb, device=0)
        monkeypatch.delenv("RK_NO_DENSE_UNITS", raising=False)

    def close(self):
        self.dense.close()
        self.canon.close()

    def check(self, seq, off, min_placed):
        dense, canon = self.dense, self.canon
        assert dense.kernel_name().startswith("place_packed16_kernel<") and "ROW24," in dense.kernel_name(), dense.kernel_name()
        assert "ROW24," not in canon.kernel_name(), canon.kernel_name()
        n = len(off) - 1
        got, ns_bound = place_into_filled_buffers(dense, seq, off)
        ref = self.odb.place(seq, off, keep_at_most=K_BEST, keep_factor=0.01, ns_bound=ns_bound)
        st = compare_with_oracle(got, ref, self.odb, seq, off)  # every read: nothing sampled
        assert st["n"] == n and st["placed"] >= min_placed, st
        want, _ = place_into_filled_buffers(canon, seq, off)
        for f in ("n_rows", "branch", "flags"):
            assert np.array_equal(getattr(got, f), getattr(want, f)), f
        assert np.array_equal(got.score.view(np.uint32), want.score.view(np.uint32))
        assert np.array_equal(got.lwr.view(np.uint64), want.lwr.view(np.uint64))


def random_read(rng, q):
    """a read of q k-mer positions (q = 0: one symbol short of a k-mer)"""
    return rng.integers(0, 4, size=q + K_MER - 1 if q > 0 else K_MER - 1)


def composed_reads(rng):
    """case A's reads, as lists of Q per tile: every row is one unit, so a read's units are its Q"""
    tiles = []
    tiles += [[141] * 4, [200] * 4, [141, 200, 141, 144]]            # four long reads (Q = 200: a second batch of positions)
    tiles += [[0, 141, 141, 141], [141, 0, 30, 141], [141, 141, 141, 0], [0, 0, 0, 141], [0, 0, 0, 0]]  # shorter than k among long ones
    tiles += [[q] * 4 for q in range(0, 41)]                        # wcnt = every count 0 .. 40 (every wcnt mod 8); early from 16 on
    for m in range(1, 18):                                          # the largest count of a tile is each of 1 .. 17
        tiles.append([m] + [int(x) for x in rng.integers(0, m + 1, size=3)])
        tiles.append([int(x) for x in rng.integers(0, m + 1, size=3)] + [m])
    tiles += [[16, 20, 30, 141], [141, 17, 16, 18], [15, 20, 30, 141], [17, 17, 17, 17], [16, 16, 16, 15]]  # around 2U, one read deciding
    pool = np.concatenate([np.arange(0, 41), np.full(12, 141)])
    for _ in range(600):
        tiles.append([int(x) for x in rng.choice(pool, size=4)])
    for _ in range(150):                                            # tiles of reads at and above 2U: mostly early
        tiles.append([int(x) for x in rng.choice(np.concatenate([np.arange(14, 41), np.full(6, 141)]), size=4)])
    return tiles


@pytest.mark.parametrize("below_threshold", [0.0, 0.3], ids=["mono", "below_threshold"])
def test_case_a_ragged_reads_every_list_length(dev_lib, monkeypatch, below_threshold):
    units = np.ones(SPACE, dtype=np.int64)
    rng = np.random.default_rng(901)
    tiles = composed_reads(rng)
    states = [random_read(rng, q) for t in tiles for q in t]
    early, first, total = tiles_of(units, states)
    assert_both_kinds(early, first)
    qs = np.asarray(tiles)
    assert np.array_equal(total, qs) and np.array_equal(first, np.minimum(qs, FIRST_SCAN))  # units = Q
    assert set(range(1, 18)) <= set(total.max(axis=1).tolist())
    assert set((total.max(axis=1) % U).tolist()) == set(range(U))  # the exit test at every wcnt mod U
    for q in (15, 16, 17):  # the early path on and off around 2U
        t = np.nonzero((total == q).all(axis=1))[0]
        assert len(t) and bool(early[t[0]]) == (q >= 2 * U)
    seq, off = reads_from_states(states)
    assert len(states) < 32768
    e = Engines(make_db(units, seed=902, below_threshold=below_threshold), monkeypatch)
    try:
        e.check(seq, off, min_placed=len(states) // 2)
    finally:
        e.close()


def test_case_b_first_scan_decides_not_the_total(dev_lib, monkeypatch):
    """half of the k-mers present -- those that begin with A or C, so a position holds a unit when its symbol is one of the two --
    and reads whose positions 0..63 carry 8 .. 24 units while every read's total is far above 2U"""
    first_sym = np.arange(SPACE) % 4
    units = (first_sym < 2).astype(np.int64)
    rng = np.random.default_rng(903)
    n = 3000
    want = rng.integers(8, 25, size=n)
    want[:8] = [16, 17, 20, 24, 24, 24, 24, 15]  # tile 0: exactly 2U in one read and more in the others; tile 1: one read below
    states = []
    for r in range(n):
        s = rng.integers(0, 4, size=141 + K_MER - 1)
        head = np.where(rng.permutation(FIRST_SCAN) < want[r], rng.integers(0, 2, size=FIRST_SCAN), rng.integers(2, 4, size=FIRST_SCAN))
        s[:FIRST_SCAN] = head
        states.append(s)
    early, first, total = tiles_of(units, states)
    assert np.array_equal(first.reshape(-1), want) and first.min() == 8 and first.max() == 24
    assert total.min() >= 3 * U, total.min()  # the total would start the ring everywhere
    assert_both_kinds(early, first)
    assert early[0] and not early[1]
    seq, off = reads_from_states(states)
    e = Engines(make_db(units, seed=904), monkeypatch)
    try:
        e.check(seq, off, min_placed=n // 2)
    finally:
        e.close()


def test_case_c_multi_unit_rows_across_the_ring_boundaries(dev_lib, monkeypatch):
    """rows of 1, 2, 3 and 15 units; reads in which a row of each of the longer kinds lies across list slots U - 1 | U and across
    2U - 1 | 2U (found among random reads by the twin, in tiles that start the ring early and in tiles that do not)"""
    rng = np.random.default_rng(905)
    units = rng.choice(np.asarray([1, 2, 3, 15]), size=SPACE, p=[0.76, 0.1, 0.1, 0.04]).astype(np.int64)
    n = 3000
    qs = rng.choice(np.asarray([6, 9, 12, 20, 141]), size=n)
    states = [random_read(rng, int(q)) for q in qs]
    # tile 0: exactly 2U units in one read (a random read cut where its units reach 2U) and more in the three others
    while True:
        s = random_read(rng, 40)
        cut = np.nonzero(np.cumsum(unit_prefix(units, s)) == 2 * U)[0]
        if len(cut):
            states[1] = s[:int(cut[0]) + K_MER]
            break
    for r in (0, 2, 3):
        states[r] = random_read(rng, 141)
    early, first, total = tiles_of(units, states)
    assert_both_kinds(early, first)
    assert early[0] and first[0, 1] == 2 * U
    seen = set()
    for r, s in enumerate(states):
        u = unit_prefix(units, s)
        start = np.cumsum(u) - u
        for b in (U, 2 * U):
            for nu in (2, 3, 15):
                if ((u == nu) & (start < b) & (start + u > b)).any():
                    seen.add((b, nu, bool(early[r // 4])))
    missing = {(b, nu, e) for b in (U, 2 * U) for nu in (2, 3, 15) for e in (False, True)} - seen
    assert not missing, f"no row planted across (boundary, units, early tile): {sorted(missing)}"
    # ... and batches that go through the list in parts, behind a ring started early and behind one that was not
    parts = (total > CAP_ITEMS).any(axis=1)
    assert (parts & early).any() and (parts & ~early).any(), (int((parts & early).sum()), int((parts & ~early).sum()))
    seq, off = reads_from_states(states)
    e = Engines(make_db(units, seed=906), monkeypatch)
    try:
        e.check(seq, off, min_placed=n // 2)
    finally:
        e.close()


def test_case_d_missing_reads_in_the_last_tile(dev_lib, monkeypatch):
    units = np.ones(SPACE, dtype=np.int64)
    rng = np.random.default_rng(907)
    e = Engines(make_db(units, seed=902), monkeypatch)
    try:
        kinds, edge = set(), False
        for n in (1, 2, 3, 5, 4 * 37 + 1, 4 * 500 + 1):
            qs = rng.choice(np.asarray([16, 17, 24, 40, 141]), size=n)  # every read alone would start the ring: the missing ones decide
            if n > 8:
                qs[:8] = [16, 20, 30, 141, 8, 141, 141, 141]
            states = [random_read(rng, int(q)) for q in qs]
            early, first, total = tiles_of(units, states)
            assert not early[-1] and (first[-1] == -1).sum() == 4 - n % 4  # the last tile misses reads and starts its ring in the flush
            kinds |= set(early.tolist())
            edge = edge or bool((early & (first == 2 * U).any(axis=1) & ((first > 2 * U).sum(axis=1) == 3)).any())
            seq, off = reads_from_states(states)
            e.check(seq, off, min_placed=n)
        assert kinds == {False, True} and edge
    finally:
        e.close()
