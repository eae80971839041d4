"""The dense 24-entry row units of small trees (rk_device.h ROW_UNIT24): place_packed16_kernel on the dense view must give what it gives
on the canonical 16-entry units, field for field and bit for bit.  RK_NO_DENSE_UNITS (developer library only, read when a handle is
made) keeps a handle on the canonical layout."""
import re

import numpy as np
import pytest

import rappas_amd as ra
from oracle import oracle as O
from rappas_amd import synth
from tests.util import compare_with_oracle

pytestmark = pytest.mark.gpu


def _make(sdb, monkeypatch, dense, **kw):
    if dense:
        monkeypatch.delenv("RK_NO_DENSE_UNITS", raising=False)
    else:
        monkeypatch.setenv("RK_NO_DENSE_UNITS", "1")
    db = ra.PhyloKmerDB.from_synth(sdb, **kw)
    monkeypatch.delenv("RK_NO_DENSE_UNITS", raising=False)
    assert ("ROW24," in db.kernel_name()) == dense, db.kernel_name()
    return db


def _place(db, seq, off, K=7):
    return ra.PlacementProcess(db).processQueries(seq, off, keepAtMost=K)


def _assert_same(a, b):
    assert np.array_equal(a.n_rows, b.n_rows)
    assert np.array_equal(a.branch, b.branch)
    assert np.array_equal(a.flags, b.flags)
    assert np.array_equal(a.score.view(np.uint32), b.score.view(np.uint32))
    assert np.array_equal(a.lwr.view(np.uint64), b.lwr.view(np.uint64))


def _both(sdb, monkeypatch, cases):
    """cases: [(seq, off, K)]; every case placed through a dense and a canonical handle of the same database"""
    out = []
    dd = _make(sdb, monkeypatch, True)
    dc = _make(sdb, monkeypatch, False)
    try:
        assert dd.kernel_name().startswith("place_packed16_kernel<"), dd.kernel_name()
        for seq, off, K in cases:
            a, b = _place(dd, seq, off, K), _place(dc, seq, off, K)
            _assert_same(a, b)
            out.append(a)
    finally:
        dd.close()
        dc.close()
    return out


def _rows_db(alphabet, k, n_branches, lens, seed, below_threshold=0.0):
    """every k-mer present (a read hits on every position), row lengths cycled from `lens`, random distinct branches per row;
    `below_threshold`: share of scores under thr_log10 (a non-mono database)"""
    rng = np.random.default_rng(seed)
    space = alphabet ** k
    key_codes = synth.dense_to_code(alphabet, k, np.arange(space, dtype=np.uint64))
    rl = np.resize(np.asarray(lens, dtype=np.int64), space)
    off = np.zeros(space + 1, dtype=np.uint64)
    np.cumsum(rl, out=off[1:])
    br = np.concatenate([rng.choice(n_branches, size=int(n), replace=False) for n in rl]).astype(np.uint16)
    br[0] = 0  # the first row and the second touch both ends of the tree
    a, e = int(off[1]), int(off[2])
    if n_branches - 1 not in br[a:e]:
        br[a] = n_branches - 1
    thr, t = synth.thresholds(1.5, alphabet, k)
    sc = (t * rng.random(len(br), dtype=np.float32)).astype(np.float32)
    low = rng.random(len(br)) < below_threshold
    sc[low] = (t * (1.0 + rng.random(int(low.sum()), dtype=np.float32))).astype(np.float32)
    return synth.SynthDB(alphabet, k, n_branches, thr, t, key_codes, off, br, sc, seed)


def test_c1_and_c2_shaped_keep_at_most_and_variable_lengths(dev_lib, monkeypatch):
    c1 = synth.make_config_db("C1")
    seq, off = synth.make_reads(4, 3000, 150, seed=3)
    vs, vo = synth.make_reads(4, 3000, 150, seed=4, var_len=120)
    got = _both(c1, monkeypatch, [(seq, off, 7), (vs, vo, 1), (vs, vo, 16)])
    odb = O.OracleDB.from_synth(c1)
    compare_with_oracle(got[0], odb.place(seq, off), odb, seq, off)

    c2 = synth.make_config_db("C2")
    seq, off = synth.make_reads(4, 100_000, 150, seed=5)
    vs, vo = synth.make_reads(4, 20_000, 150, seed=6, var_len=100)
    got = _both(c2, monkeypatch, [(seq, off, 7), (vs, vo, 1), (vs, vo, 16)])
    sub = 2000
    s2, o2 = seq[: int(off[sub])], off[: sub + 1]
    odb = O.OracleDB.from_synth(c2)
    g = got[0]
    part = ra.Placements(g.n_rows[:sub], g.branch[:sub], g.score[:sub], g.lwr[:sub], g.flags[:sub], {})
    compare_with_oracle(part, odb.place(s2, o2), odb, s2, o2)


def test_clade_shaped_batches(dev_lib, monkeypatch):
    """a batch large enough for the re-tiling pre-pass: the dense kernel and the 16-entry one are launched side by side and the batch's
    shape, judged on the device, picks one; a uniform batch of the same size takes the other"""
    sdb, genome = synth.make_clade_db(seed=9)
    seq, off = synth.make_clade_reads(genome, 60_000, seed=10)
    us, uo = synth.make_reads(4, 60_000, 150, seed=11)
    got = _both(sdb, monkeypatch, [(seq, off, 7), (us, uo, 7)])
    sub = 1000
    s2, o2 = seq[: int(off[sub])], off[: sub + 1]
    odb = O.OracleDB.from_synth(sdb)
    g = got[0]
    part = ra.Placements(g.n_rows[:sub], g.branch[:sub], g.score[:sub], g.lwr[:sub], g.flags[:sub], {})
    compare_with_oracle(part, odb.place(s2, o2), odb, s2, o2)


def test_non_mono_database(dev_lib, monkeypatch):
    sdb = _rows_db(4, 6, 500, [3, 9, 14, 30], seed=11, below_threshold=0.3)
    seq, off = synth.make_reads(4, 2000, 150, seed=12, var_len=60)
    got = _both(sdb, monkeypatch, [(seq, off, 7), (seq, off, 16)])
    odb = O.OracleDB.from_synth(sdb)
    compare_with_oracle(got[0], odb.place(seq, off), odb, seq, off)


def test_row_lengths_around_the_unit_and_the_wide_row_fallback(dev_lib, monkeypatch):
    """rows of 1, 16, 17, 23, 24, 25, 48, 49 and 240 entries on a 1 023-branch tree (branch ids 0 and 1 022 included); every k-mer of a
    read has a row, so a batch of 144 positions carries more dense units than the hit list holds: the fallback that feeds the list
    in parts runs (asserted from the list capacity the kernel name reports)"""
    lens = [1, 16, 17, 23, 24, 25, 48, 49, 240]
    sdb = _rows_db(4, 4, 1023, lens, seed=21)
    seq, off = synth.make_reads(4, 1500, 150, seed=22)
    db = _make(sdb, monkeypatch, True)
    try:
        cap = int(re.search(r"cap=(\d+)", db.kernel_name()).group(1))
    finally:
        db.close()
    units = np.resize(np.asarray([-(-n // 24) for n in lens]), 4 ** 4)
    codes = synth.codes_of_reads(4, 4, seq[: int(off[1])], off[:2])
    dense_idx = np.array([int(c) for c in codes])  # DNA: the code is the dense index
    assert units[dense_idx[:144]].sum() > 2 * cap - 3 * 8 - 2  # the first batch of a read overflows an empty list
    got = _both(sdb, monkeypatch, [(seq, off, 7), (seq, off, 16)])
    odb = O.OracleDB.from_synth(sdb)
    compare_with_oracle(got[0], odb.place(seq, off), odb, seq, off)


def test_1024_branches_stay_on_16_entry_units(dev_lib, monkeypatch):
    sdb = _rows_db(4, 5, 1024, [1, 5, 17, 24, 25, 40], seed=31)
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        assert "ROW24" not in db.kernel_name() and "place_packed16_kernel<" in db.kernel_name(), db.kernel_name()
        seq, off = synth.make_reads(4, 1500, 150, seed=32)
        got = _place(db, seq, off)
    finally:
        db.close()
    odb = O.OracleDB.from_synth(sdb)
    compare_with_oracle(got, odb.place(seq, off), odb, seq, off)


def test_clone_and_saved_image_keep_the_dense_view(dev_lib, monkeypatch, tmp_path):
    sdb = synth.make_config_db("C1", seed=7)
    seq, off = synth.make_reads(4, 4000, 150, seed=8, var_len=30)
    db = _make(sdb, monkeypatch, True)
    try:
        want = _place(db, seq, off)
        cl = db.clone(0)
        db.save(tmp_path / "c1.rkdb")
        ld = ra.PhyloKmerDB.load(tmp_path / "c1.rkdb")
        for h in (cl, ld):
            try:
                assert "ROW24," in h.kernel_name(), h.kernel_name()
                _assert_same(_place(h, seq, off), want)
            finally:
                h.close()
    finally:
        db.close()
