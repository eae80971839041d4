"""GPU (-m gpu): the row ring of the dense 24-entry kernel (place_packed16_kernel<..., ROW24>) at its own depth U' (RK_RING_DENSE;
DESIGN.md 4.1a "Round 11"), with the list items of a block of U' steps held in ONE register -- lane u of a read's 16 lanes holds the
item of ring place u, read by one ds_read_b32 with per-lane addresses and handed to the step by DPP row_newbcast:u.  What moves with
U': the early start (every read of the tile holds >= 2U' units after the emit's first prefix scan), the tail of up to (U' - 2) / 2
pairs of steps, the fillers behind the longest list (as far as the 16-item read of the last block reaches) and the room of the list.
Databases, reads and the bar are those of test_gpu_dense_ring_start.py (DNA k = 5 on 1 023 branches, planted units); the numpy twin of
the start rule below is at U', asserted on the CPU as a precondition on the inputs: early and late starts both occur, and a tile
with exactly 2U' first-scan units in one read and more in the others is among them.  Bar: the oracle's placements for every read,
written into 0xFF-filled result buffers; and the canonical 16-entry units' results (RK_NO_DENSE_UNITS on a second handle), bit for bit."""
import numpy as np
import pytest

from tests import test_gpu_dense_ring_start as rs

pytestmark = pytest.mark.gpu

K_MER = rs.K_MER
SPACE = rs.SPACE
FIRST_SCAN = rs.FIRST_SCAN
U = 12                                       # the dense ring (RK_RING_DENSE in rk_geometry.h)
ITEM_BLOCK = 16                              # items one register holds: a row of 16 lanes
REACH = max(2 * U, U + ITEM_BLOCK)           # fillers behind the longest list: the item read of the last whole block ends there
CAP_ITEMS = 2 * 128 - REACH - 2              # what a read's list holds (1 023 branches: list_cap = 128 pairs of items)
TOP = 2 * U + 17                             # the longest list of a tile takes every length 0 .. TOP


def tiles_of(units, states):
    """the numpy twin of the first-scan rule at U' -> (early[t], first[t, 4], total[t, 4]); a missing read counts -1 units"""
    n = len(states)
    nt = (n + 3) // 4
    first = np.full(4 * nt, -1, dtype=np.int64)
    total = np.full(4 * nt, -1, dtype=np.int64)
    for r, s in enumerate(states):
        u = rs.unit_prefix(units, s)
        first[r] = u[:FIRST_SCAN].sum()
        total[r] = u.sum()
    first, total = first.reshape(nt, 4), total.reshape(nt, 4)
    return (first >= 2 * U).all(axis=1) & (first <= CAP_ITEMS).all(axis=1), first, total


def exact_edge(early, first):
    return early & (first == 2 * U).any(axis=1) & ((first > 2 * U).sum(axis=1) == 3)


def assert_both_kinds(early, first):
    assert early.any() and (~early).any(), (int(early.sum()), len(early))
    assert exact_edge(early, first).any(), "no tile with exactly 2U' units in one read and more in the others"


Engines = rs.Engines


def composed_reads(rng):
    """case A's reads, as lists of Q per tile: every row is one unit, so a read's units are its Q"""
    tiles = []
    tiles += [[141] * 4, [200] * 4, [141, 200, 141, 144]]            # four long reads (Q = 200: a second batch of positions)
    tiles += [[0, 141, 141, 141], [141, 0, 30, 141], [141, 141, 141, 0], [0, 0, 0, 141], [0, 0, 0, 0]]  # shorter than k among long ones
    tiles += [[q] * 4 for q in range(0, TOP + 1)]                   # wcnt = every count 0 .. 2U' + 17; early from 2U' on
    for m in range(1, TOP + 1):                                     # the largest count of a tile is each of 1 .. 2U' + 17
        tiles.append([m] + [int(x) for x in rng.integers(0, m + 1, size=3)])
        tiles.append([int(x) for x in rng.integers(0, m + 1, size=3)] + [m])
    tiles += [[2 * U, 2 * U + 4, 2 * U + 14, 141], [141, 2 * U + 1, 2 * U, 2 * U + 2], [2 * U - 1, 2 * U + 4, 2 * U + 14, 141],
              [2 * U + 1] * 4, [2 * U, 2 * U, 2 * U, 2 * U - 1]]     # around 2U', one read deciding
    pool = np.concatenate([np.arange(0, TOP + 1), np.full(12, 141)])
    for _ in range(500):
        tiles.append([int(x) for x in rng.choice(pool, size=4)])
    for _ in range(150):                                            # tiles of reads at and above 2U': mostly early
        tiles.append([int(x) for x in rng.choice(np.concatenate([np.arange(2 * U - 2, TOP + 1), np.full(6, 141)]), size=4)])
    return tiles


@pytest.mark.parametrize("below_threshold", [0.0, 0.3], ids=["mono", "below_threshold"])
def test_case_a_every_list_length_to_two_rings_and_an_item_block(dev_lib, monkeypatch, below_threshold):
    units = np.ones(SPACE, dtype=np.int64)
    rng = np.random.default_rng(1101)
    tiles = composed_reads(rng)
    states = [rs.random_read(rng, q) for t in tiles for q in t]
    early, first, total = tiles_of(units, states)
    assert_both_kinds(early, first)
    qs = np.asarray(tiles)
    assert np.array_equal(total, qs) and np.array_equal(first, np.minimum(qs, FIRST_SCAN))  # units = Q
    longest = total.max(axis=1)
    # every length 0 .. 2U' + 17 of the longest list: every count of tail pairs (0 .. (U' - 2) / 2) behind zero, one and two whole
    # blocks, and every place of the item register's reload -- in tiles that start late (below 2U') and, from 2U' on, early as well
    assert set(range(0, TOP + 1)) <= set(longest.tolist())
    assert set(range(2 * U, TOP + 1)) <= set(longest[early].tolist())
    assert set(range(1, TOP + 1)) <= set(longest[~early].tolist())
    for q in (2 * U - 1, 2 * U, 2 * U + 1):  # the early path on and off around 2U'
        t = np.nonzero((total == q).all(axis=1))[0]
        assert len(t) and bool(early[t[0]]) == (q >= 2 * U)
    seq, off = rs.reads_from_states(states)
    assert len(states) < 32768
    e = Engines(rs.make_db(units, seed=1102, below_threshold=below_threshold), monkeypatch)
    try:
        e.check(seq, off, min_placed=len(states) // 2)
    finally:
        e.close()


def test_case_b_first_scan_decides_not_the_total(dev_lib, monkeypatch):
    """three quarters of the k-mers present -- those that do not begin with T -- and reads whose positions 0..63 carry U' .. 3U' units
    while every read's total is far above 2U'"""
    first_sym = np.arange(SPACE) % 4
    units = (first_sym < 3).astype(np.int64)
    rng = np.random.default_rng(1103)
    n = 2400
    want = rng.integers(U, 3 * U + 1, size=n)
    want[:8] = [2 * U, 2 * U + 1, 2 * U + 4, 3 * U, 3 * U, 3 * U, 3 * U, 2 * U - 1]  # tile 0: exactly 2U' in one read; tile 1: one read below
    assert 3 * U <= FIRST_SCAN
    states = []
    for r in range(n):
        s = rng.integers(0, 4, size=141 + K_MER - 1)
        s[:FIRST_SCAN] = np.where(rng.permutation(FIRST_SCAN) < want[r], rng.integers(0, 3, size=FIRST_SCAN), 3)
        states.append(s)
    early, first, total = tiles_of(units, states)
    assert np.array_equal(first.reshape(-1), want) and first.min() == U and first.max() == 3 * U
    assert total.min() >= 3 * U, total.min()  # the total would start the ring everywhere
    assert_both_kinds(early, first)
    assert early[0] and not early[1]
    seq, off = rs.reads_from_states(states)
    e = Engines(rs.make_db(units, seed=1104), monkeypatch)
    try:
        e.check(seq, off, min_placed=n // 2)
    finally:
        e.close()


def test_case_c_multi_unit_rows_across_the_ring_and_every_item_block(dev_lib, monkeypatch):
    """rows of 1, 2, 3 and 15 units; reads in which a row of each of the longer kinds lies across list slot b - 1 | b for b = U', 2U'
    and every further multiple of the item block (U' items: the register is reloaded once a block) up to 6U', in tiles that start
    the ring early and in tiles that do not; and batches that overflow the list behind both kinds of start"""
    rng = np.random.default_rng(1105)
    units = rng.choice(np.asarray([1, 2, 3, 15]), size=SPACE, p=[0.76, 0.1, 0.1, 0.04]).astype(np.int64)
    n = 3000
    qs = rng.choice(np.asarray([U - 2, U + 1, 2 * U - 4, 2 * U + 4, 3 * U, 60, 90, 141]), size=n, p=[0.08, 0.08, 0.08, 0.08, 0.08, 0.15, 0.15, 0.3])
    states = [rs.random_read(rng, int(q)) for q in qs]
    # tile 0: exactly 2U' units in one read (a random read cut where its units reach 2U') and more in the three others
    while True:
        s = rs.random_read(rng, 60)
        cut = np.nonzero(np.cumsum(rs.unit_prefix(units, s)) == 2 * U)[0]
        if len(cut):
            states[1] = s[:int(cut[0]) + K_MER]
            break
    for r in (0, 2, 3):
        states[r] = rs.random_read(rng, 141)
    early, first, total = tiles_of(units, states)
    assert_both_kinds(early, first)
    assert early[0] and first[0, 1] == 2 * U
    bounds = [U * m for m in range(1, 7)]
    seen = set()
    for r, s in enumerate(states):
        u = rs.unit_prefix(units, s)
        start = np.cumsum(u) - u
        if total[r // 4].max() > CAP_ITEMS:  # (a batch that goes through the list in parts lays its rows elsewhere)
            continue
        for b in bounds:
            for nu in (2, 3, 15):
                if ((u == nu) & (start < b) & (start + u > b)).any():
                    seen.add((b, nu, bool(early[r // 4])))
    missing = {(b, nu, e) for b in bounds for nu in (2, 3, 15) for e in (False, True)} - seen
    assert not missing, f"no row planted across (boundary, units, early tile): {sorted(missing)}"
    parts = (total > CAP_ITEMS).any(axis=1)
    assert (parts & early).any() and (parts & ~early).any(), (int((parts & early).sum()), int((parts & ~early).sum()))
    seq, off = rs.reads_from_states(states)
    e = Engines(rs.make_db(units, seed=1106), monkeypatch)
    try:
        e.check(seq, off, min_placed=n // 2)
    finally:
        e.close()


def test_case_d_missing_reads_in_the_last_tile(dev_lib, monkeypatch):
    units = np.ones(SPACE, dtype=np.int64)
    rng = np.random.default_rng(1107)
    e = Engines(rs.make_db(units, seed=1102), monkeypatch)
    try:
        kinds, edge = set(), False
        for n in (1, 2, 3, 5, 4 * 37 + 1, 4 * 500 + 1):
            qs = rng.choice(np.asarray([2 * U, 2 * U + 1, 3 * U, 5 * U, 141]), size=n)  # every read alone would start the ring: the missing ones decide
            if n > 8:
                qs[:8] = [2 * U, 2 * U + 4, 3 * U, 141, U, 141, 141, 141]
            states = [rs.random_read(rng, int(q)) for q in qs]
            early, first, total = tiles_of(units, states)
            assert not early[-1] and (first[-1] == -1).sum() == 4 - n % 4  # the last tile misses reads and starts its ring in the flush
            kinds |= set(early.tolist())
            edge = edge or bool(exact_edge(early, first).any())
            seq, off = rs.reads_from_states(states)
            e.check(seq, off, min_placed=n)
        assert kinds == {False, True} and edge
    finally:
        e.close()
