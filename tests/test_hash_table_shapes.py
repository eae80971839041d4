"""The lookup tables as build_table (rk_engine.hip) writes them, read back from the image file without a device.

Hashed table: the planted tables of tests/hashplant.py -- keys whose homes all lie in the last eighth of the table -- hold what the
builder promises (occupancy, every key reachable, descriptors) and the shapes tests/test_gpu_hash_probe.py needs on the device: one
cluster through the end of the table, long walks of absent codes, walks from the last slot to slot 0, and for 64-bit keys the
low-word aliases and the zero low words.  Seeds and read counts are settled here.

Compact direct table: every code's (first unit, units) decoded with a numpy restatement of both block forms equals the layout rule,
up to the form's upper edge -- a block of twelve rows of 255 units -- and the fall-back to 8-byte descriptors one entry beyond."""
import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import synth
from tests import hashplant as H
from tests.test_db_image import SHAPES


def test_mix64_known_values():
    """the finaliser of MurmurHash3 (fmix64): 0 is its fixed point, and it is a bijection -- its inverse restated here undoes it"""
    assert int(H.mix64(0)[0]) == 0
    x = np.random.default_rng(1).integers(0, 1 << 63, size=1000).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    y = H.mix64(x)
    assert len(np.unique(y)) == len(x)
    with np.errstate(over="ignore"):
        z = y ^ (y >> np.uint64(33))
        z *= np.uint64(0x9CB4B2F8129337DB)  # the inverse of 0xC4CEB9FE1A85EC53 modulo 2^64
        z ^= z >> np.uint64(33)
        z *= np.uint64(0x4F74430C22A54005)  # the inverse of 0xFF51AFD7ED558CCD
        z ^= z >> np.uint64(33)
    assert np.array_equal(z, x)
    assert (0x9CB4B2F8129337DB * 0xC4CEB9FE1A85EC53) & H.M64 == 1 and (0x4F74430C22A54005 * 0xFF51AFD7ED558CCD) & H.M64 == 1


@pytest.mark.parametrize("name", sorted(H.TABLES))
def test_planted_table_as_the_builder_writes_it(name, tmp_path):
    alphabet, k, slots, how = H.TABLES[name]
    sdb = H.database(name)
    keys = sdb.key_codes
    assert len(keys) == slots // 2 and H.valid_code(alphabet, k, keys).all()
    if how != "zero_low":
        assert (H.home(keys, slots) >= slots - slots // 8).all()
    path = tmp_path / "db.rkimg"
    H.save_image(sdb, path)
    info, table = H.table_of_image(path)
    assert info.table_mode == ra.RK_TABLE_HASH and info.table_slots == slots and info.table_bytes == 16 * slots
    p = H.assert_table(info, table, sdb)
    # every descriptor is its own row's: rows lie in ascending dense order from unit 1 on, a 128-byte unit = 16 eight-byte entries
    order = np.argsort(H.dense_index(alphabet, k, keys), kind="stable")
    units = (np.diff(sdb.row_offsets.astype(np.int64)) + 15) // 16
    first = np.zeros(len(keys), dtype=np.int64)
    first[order] = 1 + np.cumsum(units[order]) - units[order]
    assert np.array_equal((table[p["slot"], 1] >> np.uint64(24)).astype(np.int64), first * 16)
    for L, amb in ((150, False), (300, False), (150, True), (k + 15, False), (k, False)):
        seq, off = H.reads(name, L, amb)
        c = H.assert_planted(name, table, sdb, seq, off, f"L={L} amb={amb}")
        if L == k:  # one k-mer a read: a key (the alias tables' reads of two k-mers and more also ask for the absent partners)
            assert c["probe"]["found"].all()
    if how == "alias":
        # the variants: pairs stored whole, and half-stored pairs whose stored member sits on the absent one's path
        _, partners = H.keys_of(name)
        assert len(partners) >= 20 and not np.isin(partners, keys).any() and np.isin(partners ^ np.uint64(H.ALIAS_BIT), keys).all()
        whole = np.isin(keys ^ np.uint64(H.ALIAS_BIT), keys)
        assert whole.sum() >= 20
        seq, off = H.reads(name, 150)
        asked = np.unique(np.concatenate(H.codes_of_reads(alphabet, k, seq, off)))
        assert np.isin(partners, asked).all() and np.isin(keys, asked).all()
        pp = H.probe(table, partners)
        assert not pp["found"].any() and pp["alias"].sum() >= 20          # absent, and walked through its stored partner
        assert H.probe(table, keys[whole])["alias"].sum() >= 10          # stored behind its stored partner
    if how == "zero_low":
        special = H.zero_low_codes(k)
        assert np.isin(special, keys).all() and np.isin((special + np.uint64(1)), table[:, 0]).all()
        assert ((table[:, 0] != 0) & ((table[:, 0] & H.LOW) == 0)).sum() == 4
        seq, off = H.reads(name, 150)
        asked = np.unique(np.concatenate(H.codes_of_reads(alphabet, k, seq, off)))
        pk = H.probe(table, keys)
        assert np.isin(keys[pk["zero_low"]], asked).all() and np.isin(special, asked).all()


def test_census_counts_what_a_wrong_probe_would_get_wrong(tmp_path):
    """three wrong probes restated on the host -- low words compared only, a zero low word read as an empty slot, a walk given up
    after four steps -- each answer differently from the plain probe on the codes the census counts, and only there"""
    for name, wrong, at_least in (("dna17_alias", "low_word", 20), ("aa7_alias", "low_word", 20), ("dna17_zero_low", "zero_is_empty", 20),
                                  ("dna8_1024", "four_steps", 200), ("aa7_16", "four_steps", 3)):
        alphabet, k, slots, how = H.TABLES[name]
        sdb = H.database(name)
        H.save_image(sdb, tmp_path / name)
        _, table = H.table_of_image(tmp_path / name)
        seq, off = H.reads(name, 150)
        q = np.unique(np.concatenate(H.codes_of_reads(alphabet, k, seq, off)))
        right = H.probe(table, q)
        keep = right["found"] | right["alias"] | right["zero_low"] | (np.arange(len(q)) % 8 == 0)  # (of the other absent codes every 8th)
        q, right = q[keep], {f: v[keep] for f, v in right.items()}
        differs = 0
        for i, code in enumerate(q.tolist()):
            h, want, steps, ans = int(H.home([code], slots)[0]), code + 1, 0, None
            while ans is None:
                key = int(table[h, 0])
                if wrong == "low_word" and key and key & 0xFFFFFFFF == want & 0xFFFFFFFF:
                    ans = h
                elif key == want:
                    ans = h
                elif key == 0 or (wrong == "zero_is_empty" and key & 0xFFFFFFFF == 0) or (wrong == "four_steps" and steps == 4):
                    ans = -1
                h, steps = (h + 1) & (slots - 1), steps + 1
            truth = int(right["slot"][i]) if right["found"][i] else -1
            if ans != truth:
                differs += 1
                assert {"low_word": right["alias"][i], "zero_is_empty": right["zero_low"][i] and right["found"][i],
                        "four_steps": right["found"][i] and right["steps"][i] > 4}[wrong], (name, wrong, hex(code))
        assert differs >= at_least, (name, wrong, differs)


# ---- the compact direct table ----
def _decoded_equals_layout(sdb, mode, tmp_path):
    path = tmp_path / "compact.rkimg"
    H.save_image(sdb, path, mode)
    info, raw = H.table_bytes_of_image(path)
    assert info.table_mode == ra.RK_TABLE_DIRECT and info.table_slots == 4 ** sdb.k
    first, units, form = H.decode_compact(raw, 4 ** sdb.k)
    want_first, want_units = H.compact_layout(sdb)
    assert np.array_equal(units, want_units) and np.array_equal(first, want_first)
    assert int((units != 0).sum()) == sdb.n_keys
    return info, raw, form, units


@pytest.mark.parametrize("shape", ["dense_nibbles", "dense_bytes"])
def test_compact_table_decodes_to_the_layout_rule(shape, tmp_path):
    alphabet, k, nb, nk, ne, mode = SHAPES[shape]
    sdb = synth.make_db(alphabet, k, nb, nk, ne, seed=3)
    _, _, form, units = _decoded_equals_layout(sdb, mode, tmp_path)
    assert form == ("nibbles" if units.max() <= 15 else "bytes")
    if shape == "dense_nibbles":
        assert form == "nibbles"


def test_compact_table_at_its_upper_edge(tmp_path):
    """twelve rows of 4 080 entries in one block: 255 units each is the most a byte holds; one entry more and the table is DIRECT8"""
    sdb = H.compact_edge_db(4080)
    info, raw, form, units = _decoded_equals_layout(sdb, ra.RK_TABLE_AUTO, tmp_path)
    assert form == "bytes" and info.table_bytes == 5472 and info.max_row_len == 4080
    first_unit = 1 + int(units[:12].sum())
    assert raw[16:32] == first_unit.to_bytes(4, "little") + b"\xff" * 12
    assert (units[12:24] == 255).all() and units.max() == 255
    # rows before block 1 move its first unit: with none there it reads 01000000
    alone = H.rows_db(4, 6, 4500, H.EDGE_CODES, 5, lens=[4080] * 12)
    H.save_image(alone, tmp_path / "alone", ra.RK_TABLE_AUTO)
    assert H.table_bytes_of_image(tmp_path / "alone")[1][16:32] == bytes.fromhex("01000000") + b"\xff" * 12
    # 4 081 entries = 256 units
    over = H.compact_edge_db(4081)
    for mode in (ra.RK_TABLE_AUTO, ra.RK_TABLE_DIRECT):
        H.save_image(over, tmp_path / "over", mode)
        info8, raw8 = H.table_bytes_of_image(tmp_path / "over")
        assert info8.table_mode == ra.RK_TABLE_DIRECT8 and info8.table_bytes == 8 * 4 ** 6 and info8.max_row_len == 4081
        desc = np.frombuffer(raw8, dtype="<u8")
        want_first, want_units = H.compact_layout(over)
        assert np.array_equal(desc & np.uint64((1 << 24) - 1), want_units * np.uint64(16))
        assert np.array_equal((desc >> np.uint64(24))[want_units != 0], (want_first * np.uint64(16))[want_units != 0])
        assert (desc[want_units == 0] == 0).all()
