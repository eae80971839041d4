"""GPU (-m gpu): the device-side synthetic database (rk_db_create_synth) -- what BASELINE config C5 (~200 GB) is built with.

The image is generated in HBM from (seed, k-mer index, entry index); rappas_amd.synth.SynthSpec regenerates the same rows
with numpy.  Checks: rows read back through rk_db_fetch_row equal the numpy twin's; placements against the generated image
equal the oracle's on a database rebuilt host-side from the rows the reads touch; and the same at C5's full size (an
image of ~200 GB, far beyond what a host array could carry)."""
import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import synth
from oracle import oracle as O
from tests import image_shapes
from tests.util import compare_with_oracle

pytestmark = pytest.mark.gpu

MODES = {"direct": ra.RK_TABLE_DIRECT, "direct8": ra.RK_TABLE_DIRECT8, "hash": ra.RK_TABLE_HASH}


def small_spec(alphabet=4, k=8, n_branches=999, mean=13.0, kf=0.75, seed=7):
    thr, t = synth.thresholds(1.5, alphabet, k)
    return synth.SynthSpec(alphabet, k, n_branches, thr, t, seed, kf, mean)


def check_rows(db, spec, dense):
    present, lens = spec.present_and_lens(dense)
    codes = synth.dense_to_code(spec.alphabet, spec.k, dense)
    for i, d in enumerate(dense):
        br, sc = db.fetch_row(int(codes[i]))
        if not present[i]:
            assert len(br) == 0
            continue
        off, wb, ws = spec.rows(np.array([d], np.uint64))
        assert len(br) == int(lens[i]) == len(wb)
        assert np.array_equal(br, wb)
        assert np.array_equal(sc.view(np.uint32), ws.view(np.uint32))


@pytest.mark.parametrize("table", ["direct", "direct8", "hash"])
@pytest.mark.parametrize("shape", ["small_tree", "large_tree", "protein"])
def test_device_rows_equal_the_host_twin(table, shape):
    spec = {"small_tree": small_spec(), "large_tree": small_spec(n_branches=19_999, mean=300.0, k=7),
            "protein": small_spec(alphabet=20, k=3, n_branches=399, mean=9.0, kf=0.4)}[shape]
    db = ra.PhyloKmerDB.synthetic(spec, table_mode=MODES[table])
    try:
        rng = np.random.default_rng(3)
        dense = np.unique(np.concatenate([rng.integers(0, spec.space, 60), [0, spec.space - 1]])).astype(np.uint64)
        check_rows(db, spec, dense)
        tab = spec.row_length_table()
        assert db.info.n_keys == int((tab > 0).sum()) and db.info.n_entries == int(tab.sum())
        assert db.info.max_row_len == int(tab.max())
    finally:
        db.close()


@pytest.mark.parametrize("shape", ["small_tree", "large_tree", "protein"])
@pytest.mark.parametrize("amb", ["mean", "max"])
def test_placements_against_generated_image_equal_oracle(shape, amb):
    """whole k-mer space rebuilt on the host (small k), so reads with ambiguity characters are covered too"""
    spec = {"small_tree": small_spec(), "large_tree": small_spec(n_branches=19_999, mean=300.0, k=7),
            "protein": small_spec(alphabet=20, k=3, n_branches=399, mean=9.0, kf=0.4)}[shape]
    sdb = spec.subset_db(np.arange(spec.space, dtype=np.uint64))
    odb = O.OracleDB.from_synth(sdb)
    rlen = 100 if spec.alphabet == 20 else 150
    seq, off = synth.make_reads(spec.alphabet, 600, rlen, seed=5, amb_rate=0.003, var_len=30)
    db = ra.PhyloKmerDB.synthetic(spec)
    try:
        got = ra.PlacementProcess(db).processQueries(seq, off, treatAmbiguitiesWithMax=amb == "max")
        mode = O.AMB_MAX if amb == "max" else O.AMB_MEAN
        ref = odb.place(seq, off, amb_mode=mode)
        st = compare_with_oracle(got, ref, odb, seq, off, amb_mode=mode)
        assert st["placed"] > 500
    finally:
        db.close()


def test_generated_image_equals_rk_db_create_of_the_same_rows():
    """the same database through the host-array entry point gives identical placements (two image builders, one result)"""
    spec = small_spec(k=9, n_branches=2_001, mean=20.0)
    sdb = spec.subset_db(np.arange(spec.space, dtype=np.uint64))
    seq, off = synth.make_reads(4, 3000, 150, seed=2)
    a = ra.PhyloKmerDB.synthetic(spec)
    b = ra.PhyloKmerDB.from_synth(sdb)
    try:
        ga = ra.PlacementProcess(a).processQueries(seq, off)
        gb = ra.PlacementProcess(b).processQueries(seq, off)
        assert a.info.n_entries == b.info.n_entries and a.info.rows_bytes == b.info.rows_bytes
        for f in ("n_rows", "branch", "flags"):
            assert np.array_equal(getattr(ga, f), getattr(gb, f))
        assert np.array_equal(ga.score.view(np.uint32), gb.score.view(np.uint32)) and np.array_equal(ga.lwr, gb.lwr)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("shape", ["small_tree", "large_tree", "large_tree_indexed", "protein", "windowed"])
def test_generated_image_survives_save_load_and_clone(shape, tmp_path):
    """a generated handle, the handle loaded from its file and a clone all save to the same bytes (the header pins everything the
    image is, the sections every byte the generator wrote), and the loaded handle and the clone hold the host twin's rows.
    (The large tree is a windowed image behind the compact table, which is what AUTO resolves to at k = 7, and the indexed
    large-tree image behind 8-byte descriptors: both are here.)"""
    large = small_spec(n_branches=19_999, mean=300.0, k=7)
    spec, table, kind = {"small_tree": (small_spec(), ra.RK_TABLE_AUTO, "dense"),
                         "large_tree": (large, ra.RK_TABLE_AUTO, "windowed"), "large_tree_indexed": (large, ra.RK_TABLE_DIRECT8, "indexed"),
                         "protein": (small_spec(alphabet=20, k=3, n_branches=399, mean=9.0, kf=0.4), ra.RK_TABLE_AUTO, "dense"),
                         "windowed": (small_spec(n_branches=7_999), ra.RK_TABLE_AUTO, "windowed")}[shape]
    path = str(tmp_path / "synth.rkimg")
    rng = np.random.default_rng(3)
    dense = np.unique(np.concatenate([rng.integers(0, spec.space, 60), [0, spec.space - 1]])).astype(np.uint64)
    db = ra.PhyloKmerDB.synthetic(spec, table_mode=table)
    try:
        name = db.kernel_name()
        assert ("windows=" in name, "place_wg_kernel" in name) == (kind == "windowed", kind == "indexed"), name
        db.save(path, user=b"tree")
        first = open(path, "rb").read()
        clone = db.clone()
        try:
            clone.save(path + ".clone", user=b"tree")
            assert open(path + ".clone", "rb").read() == first
            check_rows(clone, spec, dense)
        finally:
            clone.close()
        loaded = ra.PhyloKmerDB.load(path)
        try:
            loaded.save(path + ".loaded", user=b"tree")
            assert open(path + ".loaded", "rb").read() == first
            check_rows(loaded, spec, dense)
        finally:
            loaded.close()
    finally:
        db.close()


@pytest.mark.parametrize("table", sorted(image_shapes.MODES))
@pytest.mark.parametrize("shape", ["small_tree", "large_tree_900", "protein", "windowed"])
def test_generated_image_header_is_the_recorded_one(shape, table, tmp_path):
    """the saved header of a generated image -- every field of its shape, a checksum of its sections -- is the one recorded in
    tests/golden/image_headers.tsv before the synthetic builder took its plan from rk_image_plan.h"""
    path = str(tmp_path / "synth.rkimg")
    db = ra.PhyloKmerDB.synthetic(image_shapes.synth_cases()[shape], table_mode=image_shapes.MODES[table])
    try:
        assert ("place_wg_kernel" in db.kernel_name()) == (shape == "large_tree_900")
        db.save(path)
    finally:
        db.close()
    assert image_shapes.header_hex(path) == image_shapes.golden("synth")[(shape, table)]


@pytest.fixture(scope="module")
def host_rows():
    """the rows of a generated database as CSR arrays (the numpy twin), made once per spec"""
    made = {}

    def rows(shape):
        if shape not in made:
            spec = image_shapes.synth_cases()[shape]
            made[shape] = spec.subset_db(np.arange(spec.space, dtype=np.uint64))
        return made[shape]
    return rows


@pytest.mark.parametrize("table", sorted(image_shapes.MODES))
@pytest.mark.parametrize("shape", ["small_tree", "large_tree_900", "protein", "windowed"])
def test_one_generated_database_through_both_builders(shape, table, host_rows, tmp_path):
    """rk_db_create_synth of a spec and rk_db_create of the spec's rows, both saved: the same k-mer table byte for byte in every mode;
    the same rows, but for the reserved unit 0 of a large-tree image (64 bytes: all 0xFF from the generator, {0xFFFFFFFF, 0.0f} pairs
    from rk_db_create; no kernel reads it as an entry); the same header fields, but for those the builders differ in on purpose --
    has_pos / winspec_bytes (a generated image carries no position keys) and the plan's units_per_code (density from the spec) --
    DESIGN.md, "The image plan".  What was equal before the plan moved is equal now."""
    spec, mode = image_shapes.synth_cases()[shape], image_shapes.MODES[table]
    a = ra.PhyloKmerDB.synthetic(spec, table_mode=mode)
    b = ra.PhyloKmerDB.from_synth(host_rows(shape), table_mode=mode)
    pa, pb = str(tmp_path / "synth.rkimg"), str(tmp_path / "create.rkimg")
    try:
        a.save(pa)
        b.save(pb)
    finally:
        a.close()
        b.close()
    ha, hb = bytes.fromhex(image_shapes.header_hex(pa)), bytes.fromhex(image_shapes.header_hex(pb))
    # (header offsets: scalars ... windowed [24, 76), has_pos 76, n_keys ... wp_stream [80, 136), wp_units_per_code 136, table_bytes and rows_bytes [144, 160))
    assert ha[24:76] == hb[24:76] and ha[80:136] == hb[80:136] and ha[144:160] == hb[144:160]
    (ta, ra_, wa), (tb, rb, wb) = image_shapes.sections(pa), image_shapes.sections(pb)
    indexed = shape == "large_tree_900"
    assert int.from_bytes(ha[60:64], "little") == indexed
    assert ta == tb
    assert ra_[64 if indexed else 0:] == rb[64 if indexed else 0:] and len(ra_) == len(rb)
    if table == "hash" or (shape, table) == ("windowed", "auto"):   # no third section, or window spans: equal; position keys: rk_db_create only
        assert wa == wb


def test_argument_errors():
    import ctypes as C
    from rappas_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    bad = _lib.rk_synth_desc(4, 0, 8, 999, -3.0, 0.001, 1, 0.0, 10.0, 0, 0)
    assert lib.rk_db_create_synth(C.byref(bad), C.byref(h)) == _lib.RK_ERR_INVALID
    bad = _lib.rk_synth_desc(4, 0, 8, 999, -3.0, 0.001, 1, 0.5, 0.5, 0, 0)
    assert lib.rk_db_create_synth(C.byref(bad), C.byref(h)) == _lib.RK_ERR_INVALID
    bad = _lib.rk_synth_desc(4, 0, 8, 0, -3.0, 0.001, 1, 0.5, 5.0, 0, 0)
    assert lib.rk_db_create_synth(C.byref(bad), C.byref(h)) == _lib.RK_ERR_INVALID


def test_c5_full_size_image():
    """BASELINE config C5 at its stated size: DNA k=12, 19 999 branches, ~3.3e10 entries = a ~200 GB image in one GPU's HBM.
    Reads are placed against it and compared with the oracle on a database rebuilt host-side from exactly the rows they touch
    (regenerated by the numpy twin of the generator); rows are also read back through rk_db_fetch_row."""
    spec = synth.make_spec("C5")
    db = ra.PhyloKmerDB.synthetic(spec)
    try:
        assert db.info.rows_bytes > 190e9 and db.info.n_entries > 3.2e10, (db.info.rows_bytes, db.info.n_entries)
        assert "place_wg_kernel" in db.kernel_name() and "OFF64" in db.kernel_name()
        seq, off = synth.make_reads(4, 48, 250, seed=1)
        dense = np.unique(synth.codes_of_reads(4, 12, seq, off))
        sdb = spec.subset_db(dense)
        odb = O.OracleDB.from_synth(sdb)
        got = ra.PlacementProcess(db).processQueries(seq, off)
        ref = odb.place(seq, off)
        st = compare_with_oracle(got, ref, odb, seq, off)
        assert st["placed"] == 48
        # rows at the far end of the blob (64-bit offsets) and a few of the touched ones
        far = np.arange(spec.space - 40, spec.space, dtype=np.uint64)
        check_rows(db, spec, np.concatenate([far, dense[:10], dense[-10:]]))
    finally:
        db.close()
