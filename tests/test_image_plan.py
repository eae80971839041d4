"""The image a database gets from rk_db_save_desc (no GPU), for a grid of shapes in three table modes, against the headers recorded in
tests/golden/image_headers.tsv before the layout arithmetic moved into rappas_amd/csrc/rk_image_plan.h.  A header holds every field of
the image's shape and a checksum of its table, row and window sections: an equal header is an equal file."""
import pytest

import rappas_amd as ra
from tests import image_shapes as S

INFO_FIELDS = ("alphabet", "k", "n_branches", "table_mode", "thr_log10", "thr", "n_keys", "n_entries", "table_slots", "table_bytes",
               "rows_bytes", "bits_per_symbol", "max_row_len", "device")


@pytest.fixture(scope="module")
def cases():
    return S.desc_cases()


@pytest.fixture(scope="module")
def recorded():
    return S.golden("desc")


def test_the_table_covers_every_shape_in_every_mode(cases, recorded):
    assert sorted(recorded) == sorted((name, mode) for name in cases for mode in S.MODES)
    assert all(len(h) == 2 * S.HEADER_BYTES for h in recorded.values())


@pytest.mark.parametrize("mode", sorted(S.MODES))
@pytest.mark.parametrize("shape", ["nibble_edge", "byte_first", "row_256_units", "amino", "windowed", "large_tree", "one_key", "no_keys",
                                   "not_mono", "descending", "descending_dna"])
def test_image_header_is_the_recorded_one(shape, mode, cases, recorded, tmp_path):
    sdb = cases[shape]
    path = str(tmp_path / "db.rkimg")
    S.save_desc(sdb, path, S.MODES[mode])
    assert S.header_hex(path) == recorded[(shape, mode)]
    # rk_db_validate (the plan alone) and rk_db_image_info (the header read back) describe the same database
    info, user = ra.db_image_info(path)
    want = ra.validate_db(sdb.alphabet, sdb.k, sdb.n_branches, sdb.thr_log10, sdb.thr, sdb.key_codes, sdb.row_offsets, sdb.branch_ids,
                          sdb.scores, table_mode=S.MODES[mode])
    for f in INFO_FIELDS:
        assert getattr(info, f) == getattr(want, f), f
    assert user == b"" and info.n_keys == sdb.n_keys and info.n_entries == sdb.n_entries


def test_the_shapes_are_the_forms_they_are_named_for(recorded):
    """(header offsets: table_mode 48, indexed 60, mono 64, compact_nib 68, windowed 72)"""
    word = lambda shape, mode, at: int.from_bytes(bytes.fromhex(recorded[(shape, mode)])[at:at + 4], "little")
    assert (word("nibble_edge", "auto", 48), word("nibble_edge", "auto", 68)) == (ra.RK_TABLE_DIRECT, 1)
    assert (word("byte_first", "auto", 48), word("byte_first", "auto", 68)) == (ra.RK_TABLE_DIRECT, 0)
    assert word("row_256_units", "auto", 48) == ra.RK_TABLE_DIRECT8          # AUTO fell back: the compact table cannot hold 256 units
    assert word("windowed", "auto", 72) == 1 and word("windowed", "hash", 72) == 0
    assert all(word("large_tree", m, 60) == 1 for m in S.MODES)
    assert word("not_mono", "auto", 64) == 0 and word("nibble_edge", "auto", 64) == 1
