"""GPU (-m gpu): the probe path of place_packed16_kernel on compact tables (rk_compact32.h: index -> block and position -> first unit
and units of the row -> list items) on planted DNA k=6 (4 096 k-mers, 171 blocks of 24) and amino-acid k=3 (8 000) databases of 399
and 999 branches, through both instances of the kernel: the dense 24-entry view and the canonical 16-entry units (RK_NO_DENSE_UNITS).

The databases (row length a function of the dense index, so the engine's table is known by construction):
  ramp    every k-mer present, 1..15 units, (7 idx + idx / 24) mod 15: every position of a block meets every count -- nibble form;
  sparse  a quarter of the k-mers absent in runs of five that start at 20 m - 3 (against blocks of 24 and words of 8 and 4 they come to
          straddle every word and block boundary), the others 1 or 2 units: a batch's units fit the list, the usual emit -- nibble form;
  byte    every k-mer present, 1 or 2 units, three rows of 16, 17 and 24 units: the byte form, and emit's wide-row scans;
  heavy   every row 6 units: a read's first batch (144 positions of a 150-base read, 98 of a 100-residue one) holds 864 / 588 units,
          more than any list (2 cap - 26 <= 486 items), so every batch takes the path that rebuilds a descriptor: the dense view's
          parts, the canonical kernel's row cursor;
  longest (canonical, 999 branches) one row of 999 entries = 63 units -- rk_db_create refuses a row of more entries than the tree has
          branches, and this kernel serves at most 1 275 branches, so 80 units is the most it can ever meet and a row of 255, the most a
          compact table holds, cannot be built for it -- among rows of 3 units: a read's first batch holds >= 294 units, more than the
          list (2 cap - 26 = 250 items at 999 branches), so the long row goes through accumulate_list by a rebuilt descriptor.
ramp (mean 8 units a position) takes the same two fallback paths for whole reads and the usual emit for the short ones.

Reads: 2 000 uniform reads (150 bases; 100 residues -- a record of 16 words, the kernel's limit, holds 102) = 2.8e5 probes, plus eight
reads each of length k - 1 (Q = 0), k, 150, 160 and 256 (DNA: the second probe batch, positions >= 144) or k - 1, k, 30 and 102 (amino
acids).  Bar: tests/util.compare_with_oracle on every read (scores as bit patterns), after db.kernel_name() has named the kernel."""
import functools
import re

import numpy as np
import pytest

import rappas_amd as ra
from oracle import oracle as O
from rappas_amd import synth
from tests.util import compare_with_oracle

pytestmark = pytest.mark.gpu

SHAPES = {"dna": (4, 6, 150, (5, 6, 150, 160, 256)), "aa": (20, 3, 100, (2, 3, 30, 102))}
KINDS = {"ramp": "DIRECT4", "sparse": "DIRECT4", "byte": "DIRECT", "heavy": "DIRECT4", "longest": "DIRECT"}


def units_of(kind, space):
    idx = np.arange(space, dtype=np.int64)
    few = 1 + (idx % 5 == 0)
    if kind == "ramp":
        return 1 + (7 * idx + idx // 24) % 15
    if kind == "sparse":
        return np.where((idx + 3) % 20 < 5, 0, few)
    if kind == "heavy":
        return np.full(space, 6, dtype=np.int64)
    if kind == "byte":
        u = few.copy()
        u[[5, space // 2 + 12, space - 2]] = [16, 17, 24]  # (24 units = 384 entries: still distinct branches on 399)
        return u
    u = np.full(space, 3, dtype=np.int64)  # "longest"
    u[77] = 63  # (planted() trims it to the tree's 999 entries)
    return u


@functools.lru_cache(maxsize=None)
def planted(shape, n_branches, kind):
    """(SynthDB, OracleDB, reads, offsets, the oracle's placements): built once, shared by both instances, never written to"""
    alphabet, k, L, others = SHAPES[shape]
    space = alphabet ** k
    rng = np.random.default_rng(811 + alphabet + n_branches)
    idx = np.arange(space, dtype=np.int64)
    units = units_of(kind, space)
    rl = np.minimum(np.where(units > 0, units * 16 - (5 * idx) % 16, 0), n_branches)  # ends anywhere in its last unit
    present = np.nonzero(rl)[0]
    rl = rl[present]
    off = np.zeros(len(present) + 1, dtype=np.uint64)
    np.cumsum(rl, out=off[1:])
    row = np.repeat(np.arange(len(present)), rl)
    within = np.arange(int(off[-1]), dtype=np.int64) - off[:-1].astype(np.int64)[row]
    br = ((37 * present[row] + within) % n_branches).astype(np.uint16)  # runs of neighbouring branches; any 24 in a row distinct
    thr, t = synth.thresholds(1.5, alphabet, k)
    sc = (t * rng.random(len(br), dtype=np.float32)).astype(np.float32)
    low = rng.random(len(br)) < 0.2
    sc[low] = (t * (1.0 + rng.random(int(low.sum()), dtype=np.float32))).astype(np.float32)
    sdb = synth.SynthDB(alphabet, k, n_branches, thr, t, synth.dense_to_code(alphabet, k, present.astype(np.uint64)), off, br, sc, 811)
    parts = [synth.make_reads(alphabet, 2000, L, seed=812 + alphabet)] + [synth.make_reads(alphabet, 8, n, seed=813 + n) for n in others]
    seq = np.concatenate([p[0] for p in parts])
    lens = np.concatenate([np.diff(p[1].astype(np.int64)) for p in parts])
    roff = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(lens, out=roff[1:])
    odb = O.OracleDB.from_synth(sdb)
    return sdb, odb, seq, roff, odb.place(seq, roff)


CASES = [(s, nb, kind) for s in SHAPES for nb in (399, 999) for kind in ("ramp", "sparse", "byte", "heavy")]


def run_case(monkeypatch, shape, n_branches, kind, dense):
    sdb, odb, seq, roff, ref = planted(shape, n_branches, kind)
    if dense:
        monkeypatch.delenv("RK_NO_DENSE_UNITS", raising=False)
    else:
        monkeypatch.setenv("RK_NO_DENSE_UNITS", "1")
    db = ra.PhyloKmerDB.from_synth(sdb, device=0)
    try:
        name = db.kernel_name()
        assert name.startswith("place_packed16_kernel<G=16,") and f",{KINDS[kind]}," in name and ("ROW24," in name) == dense, name
        if kind in ("heavy", "longest"):  # the units of a uniform read's first batch exceed the list
            first_batch = min(SHAPES[shape][2] - SHAPES[shape][1] + 1, 144 if shape == "dna" else 112)
            assert (6 if kind == "heavy" else 3) * first_batch > 2 * int(re.search(r"cap=(\d+)", name).group(1)) - 26, name
        got = ra.PlacementProcess(db).processQueries(seq, roff)
        st = compare_with_oracle(got, ref, odb, seq, roff)  # every read: nothing sampled
        assert st["n"] == len(roff) - 1 and st["placed"] >= 2000, st
    finally:
        db.close()


@pytest.mark.parametrize("instance", ["dense24", "canonical"])
@pytest.mark.parametrize("shape,n_branches,kind", CASES, ids=[f"{s}-{nb}-{kind}" for s, nb, kind in CASES])
def test_probe_path_against_the_oracle(dev_lib, monkeypatch, shape, n_branches, kind, instance):
    run_case(monkeypatch, shape, n_branches, kind, instance == "dense24")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_longest_row_through_the_row_cursor(dev_lib, monkeypatch, shape):
    """the longest row a tree of 999 branches can hold (63 units) in the canonical instance, in batches that never fit the list"""
    run_case(monkeypatch, shape, 999, "longest", False)
