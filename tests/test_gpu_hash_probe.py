"""The hashed k-mer table's probe on the device, on the planted tables of tests/hashplant.py: keys whose homes all lie in the last
eighth of the table, so that one cluster runs through the table's end and a lookup walks up to half the table -- through
lookup_desc<BITS, TM_HASH> (place_wg_kernel, the ambiguity kernel's per-alternative lookups, count_work_kernel, fetch_row_kernel) and
through the wave loop of place_packed_kernel, whose lanes walk on together while any of them has not met its key or an empty slot.
With 64-bit keys (DNA k = 17, amino acids k = 7): pairs of codes that differ in bit 32 only -- equal low words of key + 1 on one probe
path -- and the DNA codes whose key + 1 has a zero low word, with other keys stored behind them.

Every case reads the table back from the image the host writes and asserts its own census conditions (hashplant.assert_planted) before
it places anything; the expected values are the oracle's (tests/util.py: flags, n_rows and branches equal, scores bit-equal, LWR within
LWR_RTOL) and the CSR arrays.  Also here: the compact direct table's upper edge (rows of 255 units) and the fall-back beyond it."""
import functools

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib
from oracle import oracle as O
from tests import golden_util as GU
from tests import hashplant as H
from tests.util import compare_with_oracle

pytestmark = pytest.mark.gpu

LANES = (0, 8, 16, 32, 64)
DIRECT_TOO = ("dna6_16", "dna6_256", "dna8_1024")  # key spaces a direct table holds


def lengths(name):
    """one k-mer, k + 15, 150, and 300 symbols (packed records of more than 16 words)"""
    k = H.TABLES[name][1]
    return (k, k + 15, 150, 300)


_DIR = []  # where this module's image files go


@pytest.fixture(scope="module", autouse=True)
def _image_dir(tmp_path_factory):
    _DIR.append(tmp_path_factory.mktemp("hashplant"))
    yield
    _DIR.clear()


@functools.lru_cache(maxsize=None)
def planted(name, n_branches=399, min_row=1, max_row=24):
    """(database, its hashed table as the host writes it into an image, the image's path) -- made once"""
    sdb = H.database(name, n_branches, min_row, max_row)
    path = str(_DIR[0] / f"{name}_{n_branches}.rkimg")
    H.save_image(sdb, path)
    info, table = H.table_of_image(path)
    H.assert_table(info, table, sdb, unit=32 if n_branches > 16000 else 16)
    return sdb, table, path


@functools.lru_cache(maxsize=None)
def case(name, L, amb=False, **kw):
    """database, oracle database, reads -- after the case's own census conditions"""
    sdb, table, path = planted(name, **kw)
    seq, off = H.reads(name, L, amb)
    H.assert_planted(name, table, sdb, seq, off, f"L={L} amb={amb}")
    return sdb, oracle_db(name, **kw), seq, off


@functools.lru_cache(maxsize=None)
def oracle_db(name, **kw):
    return O.OracleDB.from_synth(planted(name, **kw)[0])


@functools.lru_cache(maxsize=None)
def oracle_place(name, L, amb, K, mode, kw=()):
    seq, off = H.reads(name, L, amb)
    return oracle_db(name, **dict(kw)).place(seq, off, keep_at_most=K, keep_factor=0.01, amb_mode=GU.AMB[mode])


def place(db, seq, off, K=7, mode="mean"):
    return ra.PlacementProcess(db).processQueries(seq, off, keepAtMost=K, keepFactor=0.01, treatAmbiguities=mode != "skip",
                                                  treatAmbiguitiesWithMax=mode == "max")


def same(a, b, what):
    for f in ("n_rows", "branch", "flags", "lwr"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)
    assert np.array_equal(a.score.view(np.uint32), b.score.view(np.uint32)), what


def check(db, name, L, amb=False, K=7, mode="mean", **kw):
    sdb, odb, seq, off = case(name, L, amb, **kw)
    got = place(db, seq, off, K, mode)
    ref = oracle_place(name, L, amb, K, mode, tuple(sorted(kw.items())))
    return got, compare_with_oracle(got, ref, odb, seq, off, amb_mode=GU.AMB[mode])


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", sorted(H.TABLES))
def test_dense_kernel_walks_the_planted_cluster(name, lanes):
    """place_packed_kernel's wave loop with 8 ... 64 lanes a read on a 399-branch tree: reads of one k-mer, k + 15, 150 and 300 symbols"""
    sdb, _, _ = planted(name)
    db = ra.PhyloKmerDB.from_synth(sdb, table_mode=ra.RK_TABLE_HASH)
    try:
        db.set_lanes_per_read(lanes)  # (a tree of 399 branches takes every width: a refusal here is a failure)
        kn = db.kernel_name()
        assert kn.startswith("place_packed_kernel<G=%d," % (lanes or 16)) and ",HASH," in kn, kn
        for L in lengths(name):
            _, st = check(db, name, L)
            assert st["placed"] >= 0.9 * st["n"], (L, st)
    finally:
        db.close()


@pytest.mark.parametrize("name", DIRECT_TOO)
def test_direct_tables_of_the_same_database_agree_field_for_field(name):
    sdb, _, _ = planted(name)
    handles = {m: ra.PhyloKmerDB.from_synth(sdb, table_mode=m) for m in (ra.RK_TABLE_HASH, ra.RK_TABLE_DIRECT, ra.RK_TABLE_DIRECT8)}
    try:
        names = {m: h.kernel_name() for m, h in handles.items()}
        assert ",HASH," in names[ra.RK_TABLE_HASH] and ",DIRECT8," in names[ra.RK_TABLE_DIRECT8], names
        assert ",DIRECT," in names[ra.RK_TABLE_DIRECT] or ",DIRECT4," in names[ra.RK_TABLE_DIRECT], names
        for L in lengths(name):
            for amb in (False, True):
                sdb, odb, seq, off = case(name, L, amb)
                got = {m: place(h, seq, off) for m, h in handles.items()}
                same(got[ra.RK_TABLE_HASH], got[ra.RK_TABLE_DIRECT], (name, L, amb, "direct"))
                same(got[ra.RK_TABLE_HASH], got[ra.RK_TABLE_DIRECT8], (name, L, amb, "direct8"))
    finally:
        for h in handles.values():
            h.close()


def test_mid_size_tree_with_a_hashed_table_takes_a_dense_kernel():
    """3 999 branches: the windowed kernels need the compact table, so a hashed table is served by place_packed_kernel"""
    kw = dict(n_branches=3999)
    sdb, _, _ = planted("dna8_1024", **kw)
    db = ra.PhyloKmerDB.from_synth(sdb, table_mode=ra.RK_TABLE_HASH)
    try:
        kn = db.kernel_name()
        assert kn.startswith("place_packed_kernel<G=") and ",HASH," in kn, kn
        for L in (150, 300):
            check(db, "dna8_1024", L, **kw)
    finally:
        db.close()


WG = dict(n_branches=19999, min_row=330, max_row=470)


@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("name", ["dna8_1024", "dna17_alias", "dna17_zero_low", "aa7_alias"])
def test_workgroup_per_read_kernel_walks_the_planted_cluster(name, K):
    """19 999 branches, rows of ~400 entries: place_wg_kernel, whose lookups go through lookup_desc<BITS, TM_HASH>"""
    sdb, _, _ = planted(name, **WG)
    db = ra.PhyloKmerDB.from_synth(sdb, table_mode=ra.RK_TABLE_HASH)
    try:
        kn = db.kernel_name()
        assert kn.startswith("place_wg_kernel<") and ",HASH," in kn, kn
        with pytest.raises(_lib.RkError) as e:  # the large-tree image has one kernel: a lane width is refused, not ignored
            db.set_lanes_per_read(16)
        assert e.value.code == _lib.RK_ERR_UNSUPPORTED
        for L in (sdb.k, 150):
            check(db, name, L, K=K, **WG)
    finally:
        db.close()


@pytest.mark.parametrize("mode", ["mean", "max", "skip"])
@pytest.mark.parametrize("name", ["dna6_256", "dna8_1024", "aa7_256", "dna17_alias", "aa7_alias", "dna17_zero_low"])
def test_ambiguity_kernel_looks_up_every_alternative(name, mode):
    """an N / X inside a written key k-mer: the key is one alternative, the others are absent codes that walk the cluster"""
    sdb, _, _ = planted(name)
    db = ra.PhyloKmerDB.from_synth(sdb, table_mode=ra.RK_TABLE_HASH)
    try:
        sdb, odb, seq, off = case(name, 150, True)
        got, st = check(db, name, 150, True, mode=mode)
        assert (got.flags & _lib.RK_FLAG_AMBIGUOUS).all() and got.counters["ambiguous"] == len(off) - 1
        if mode != "skip":  # the alternatives count: the results differ from those of the k-mers without the character alone
            skip = oracle_place(name, 150, True, 7, "skip")
            assert (skip["score"].view(np.uint32) != got.score.view(np.uint32)).any(axis=1).mean() > 0.5
    finally:
        db.close()


@pytest.mark.parametrize("name", sorted(H.TABLES))
def test_fetch_row_of_every_key_and_of_the_absent_codes_that_walk_furthest(name):
    """rk_db_fetch_row (fetch_row_kernel -> lookup_desc): every stored key's row bit for bit the CSR's; length 0 for every absent code
    of the reads that walks the longest chain or steps from the last slot to slot 0"""
    sdb, table, _ = planted(name)
    alphabet, k, slots, how = H.TABLES[name]
    seq, off = H.reads(name, k + 15)
    c = H.assert_planted(name, table, sdb, seq, off)
    pq = c["probe"]
    absent = ~pq["found"]
    ask = c["queries"][absent & ((pq["steps"] == c["longest_absent"]) | pq["wrapped"] | pq["alias"] | pq["zero_low"])]
    assert len(ask) >= 20 and c["longest_absent"] >= min(8, slots // 2)
    db = ra.PhyloKmerDB.from_synth(sdb, table_mode=ra.RK_TABLE_HASH)
    try:
        for i, code in enumerate(sdb.key_codes.tolist()):
            a, e = int(sdb.row_offsets[i]), int(sdb.row_offsets[i + 1])
            br, sc = db.fetch_row(code)
            assert np.array_equal(br, sdb.branch_ids[a:e]) and np.array_equal(sc.view(np.uint32), sdb.scores[a:e].view(np.uint32)), hex(code)
        for code in ask.tolist():
            assert len(db.fetch_row(code)[0]) == 0, hex(code)
        if how == "alias":
            for code in H.keys_of(name)[1].tolist():
                assert len(db.fetch_row(code)[0]) == 0, hex(code)
    finally:
        db.close()


@pytest.mark.parametrize("name", sorted(H.TABLES))
def test_work_counts_on_the_planted_reads(name):
    """count_work_kernel -> lookup_desc: k-mers probed, k-mers with a row and row entries equal a numpy count"""
    import torch
    sdb, table, _ = planted(name)
    alphabet, k, slots, how = H.TABLES[name]
    row_len = dict(zip(sdb.key_codes.tolist(), np.diff(sdb.row_offsets.astype(np.int64)).tolist()))
    db = ra.PhyloKmerDB.from_synth(sdb, table_mode=ra.RK_TABLE_HASH)
    try:
        pp = ra.PlacementProcess(db)
        dev = lambda x: torch.from_numpy(x.view(np.int32)).cuda()
        for L in (k, 150, 300):
            sdb, odb, seq, off = case(name, L)
            codes = np.concatenate(H.codes_of_reads(alphabet, k, seq, off))
            hits = [row_len[c] for c in codes.tolist() if c in row_len]
            want = {"kmers_probed": len(codes), "kmers_hit": len(hits), "entries": int(sum(hits))}
            assert want["kmers_probed"] == (len(off) - 1) * (L - k + 1) and want["kmers_hit"] >= 0.9 * (len(off) - 1)
            packed, lens, flags = pp.pack_reads_host(seq, off)
            assert pp.count_work(dev(packed), lens=dev(lens), flags_in=dev(flags)) == want, (name, L)
            assert pp.count_work(dev(packed), fixed_len=L) == want, (name, L)
    finally:
        db.close()


@pytest.mark.parametrize("name", ["dna6_256", "dna17_1024", "dna17_alias"])
def test_loaded_and_cloned_handles_probe_like_the_created_one(name):
    """the host-written image through PhyloKmerDB.load, and a clone of it: the table they probe is the one read back above"""
    sdb, _, path = planted(name)
    db = ra.PhyloKmerDB.from_synth(sdb, table_mode=ra.RK_TABLE_HASH)
    loaded = ra.PhyloKmerDB.load(path)
    clone = loaded.clone()
    try:
        for h in (loaded, clone):
            assert h.kernel_name() == db.kernel_name() and h.info.table_slots == db.info.table_slots == H.TABLES[name][2]
        for L, amb in ((150, False), (300, False), (150, True)):
            got, _ = check(db, name, L, amb)
            sdb, odb, seq, off = case(name, L, amb)
            same(got, place(loaded, seq, off), (name, L, amb, "loaded"))
            same(got, place(clone, seq, off), (name, L, amb, "clone"))
        for code in sdb.key_codes[:32].tolist():
            want = db.fetch_row(code)
            for h in (loaded, clone):
                g = h.fetch_row(code)
                assert len(g[0]) and np.array_equal(g[0], want[0]) and np.array_equal(g[1].view(np.uint32), want[1].view(np.uint32))
    finally:
        for h in (clone, loaded, db):
            h.close()


@pytest.mark.parametrize("longest", [4080, 4081])
def test_compact_table_at_its_upper_edge_and_one_entry_beyond(longest):
    """twelve rows of 255 units in one block of the compact table; with one row of 4 081 entries the table is RK_TABLE_DIRECT8"""
    sdb = H.compact_edge_db(longest)
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        kn = db.kernel_name()
        want_mode, tag = (ra.RK_TABLE_DIRECT, ",DIRECT,") if longest == 4080 else (ra.RK_TABLE_DIRECT8, ",DIRECT8,")
        assert db.info.table_mode == want_mode and tag in kn and kn.startswith("place_packed_kernel<"), kn
        where = {int(c): i for i, c in enumerate(sdb.key_codes.tolist())}
        for code in range(11, 25):
            br, sc = db.fetch_row(code)
            if code in (11, 24):
                assert code not in where and len(br) == 0
                continue
            i = where[code]
            a, e = int(sdb.row_offsets[i]), int(sdb.row_offsets[i + 1])
            assert e - a == (longest if code == 12 else 4080)
            assert np.array_equal(br, sdb.branch_ids[a:e]) and np.array_equal(sc.view(np.uint32), sdb.scores[a:e].view(np.uint32)), code
        # reads that hold those k-mers (and their absent neighbours)
        seq, off = H.planted_reads(4, 6, np.arange(11, 25), 64, 150, 7)
        codes = np.concatenate(H.codes_of_reads(4, 6, seq, off))
        assert np.isin(np.arange(11, 25), codes).all()
        odb = O.OracleDB.from_synth(sdb)
        got = place(db, seq, off)
        st = compare_with_oracle(got, odb.place(seq, off), odb, seq, off)
        assert st["placed"] == 64
    finally:
        db.close()
