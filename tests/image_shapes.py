"""The databases whose image headers tests/golden/image_headers.tsv records, and the table itself.

A header (rappas_amd/csrc/rk_image_impl.h: ImageHeader, 192 bytes) carries every field of the image's shape and a checksum of the table,
row and window sections, so equal headers mean equal files.  The table was written at the commit its first line names, before the image
plan moved into rk_image_plan.h:  python -m tests.image_shapes record desc   (no GPU)  /  record synth   (rk_db_create_synth, on a GPU).

The inputs come from integer arithmetic of this file (a splitmix64 finaliser), not from a library generator: the table does not depend on
numpy's."""
import os
import sys

import numpy as np

import rappas_amd as ra
from rappas_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_headers.tsv")
MODES = {"auto": ra.RK_TABLE_AUTO, "direct8": ra.RK_TABLE_DIRECT8, "hash": ra.RK_TABLE_HASH}
HEADER_BYTES = 192


def mix(x):
    """splitmix64 finaliser of a u64 array"""
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def csr_db(alphabet, k, n_branches, dense, lens, seed, below_threshold=None):
    """SynthDB of the rows `dense` (in the order given) with the lengths `lens` (cycled): a row is a run of consecutive branches from a
    drawn start, every second row stored back to front; scores thr_log10 * u, u a 24-bit fraction.  below_threshold: the entry that
    gets a score below thr_log10."""
    dense = np.asarray(dense, dtype=np.uint64)
    n = len(dense)
    ln = np.resize(np.asarray(lens, dtype=np.int64), n) if n else np.zeros(0, np.int64)
    assert n == 0 or int(ln.max()) <= n_branches
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(ln, out=off[1:])
    total = int(off[-1])
    with np.errstate(over="ignore"):
        h = mix(np.uint64(seed) + (dense + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))
        b0 = (h % (np.uint64(n_branches) - ln.astype(np.uint64) + np.uint64(1))).astype(np.int64)
        within = np.arange(total, dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), ln)
        back = np.repeat(np.arange(n) % 2 == 1, ln)
        within = np.where(back, np.repeat(ln, ln) - 1 - within, within)
        hs = mix(np.repeat(h, ln) + (within.astype(np.uint64) + np.uint64(1)) * np.uint64(0xD6E8FEB86659FD93))
    thr, thr_log10 = synth.thresholds(1.5, alphabet, k)
    branch = (np.repeat(b0, ln) + within).astype(np.uint16)
    scores = (np.float32(thr_log10) * ((hs >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24))).astype(np.float32)
    if below_threshold is not None:
        scores[below_threshold] = np.float32(thr_log10) - np.float32(1.0)
    return synth.SynthDB(alphabet, k, n_branches, thr, thr_log10, synth.dense_to_code(alphabet, k, dense), off, branch, scores, seed)


def desc_cases():
    """name -> SynthDB, the shapes rk_db_save_desc writes"""
    every = lambda space, step: np.arange(0, space, step, dtype=np.uint64)
    return {
        "nibble_edge": csr_db(4, 6, 999, every(4096, 1), [1, 16, 17, 240], 1),      # 240 entries = 15 units: the last nibble form
        "byte_first": csr_db(4, 6, 999, every(4096, 3), [241, 5, 16], 2),           # 241 entries = 16 units: the first byte form
        "row_256_units": csr_db(4, 5, 4500, every(1024, 8), [4081] + [3] * 127, 3),  # 256 units: the compact table cannot hold it
        "amino": csr_db(20, 2, 399, every(400, 1), [9, 33], 4),
        "windowed": csr_db(4, 7, 7999, every(16384, 2), [13, 1, 40], 5),
        "large_tree": csr_db(4, 5, 19999, every(1024, 4), [900, 897, 928, 929], 6),  # lenp - len = 28, 31, 0, 31
        "one_key": csr_db(4, 6, 50, [1234], [7], 7),
        "no_keys": csr_db(4, 6, 99, [], [], 8),
        "not_mono": csr_db(4, 6, 999, every(4096, 4), [5], 9, below_threshold=77),
        "descending": csr_db(20, 2, 399, every(400, 1)[::-1], [9, 33], 10),
        "descending_dna": csr_db(4, 6, 999, every(4096, 3)[::-1], [17, 2], 11),
    }


def synth_spec(alphabet=4, k=8, n_branches=999, mean=13.0, kf=0.75, seed=7):
    thr, t = synth.thresholds(1.5, alphabet, k)
    return synth.SynthSpec(alphabet, k, n_branches, thr, t, seed, kf, mean)


def synth_cases():
    """name -> SynthSpec, the generated images rk_db_save writes"""
    return {"small_tree": synth_spec(), "large_tree_900": synth_spec(n_branches=19_999, mean=900.0, k=6),
            "protein": synth_spec(alphabet=20, k=3, n_branches=399, mean=9.0, kf=0.4), "windowed": synth_spec(n_branches=7_999)}


def save_desc(sdb, path, mode):
    ra.save_db_image(path, sdb.alphabet, sdb.k, sdb.n_branches, sdb.thr_log10, sdb.thr, sdb.key_codes, sdb.row_offsets, sdb.branch_ids,
                     sdb.scores, table_mode=mode)


def header_hex(path):
    with open(path, "rb") as f:
        return f.read(HEADER_BYTES).hex()


def sections(path):
    """(table, rows, winspec) bytes of an image file (sections start on 4 096-byte boundaries; the sizes are the header's last fields)"""
    data = open(path, "rb").read()
    sizes = np.frombuffer(data[144:168], dtype=np.uint64)
    out, at = [], 4096
    for n in map(int, sizes):
        out.append(data[at:at + n])
        at += (n + 4095) // 4096 * 4096
    return out


def golden(section):
    """{(shape, mode): header hex} of one section of the recorded table"""
    with open(GOLDEN) as f:
        rows = [l.rstrip("\n").split("\t") for l in f if not l.startswith("#")]
    return {(r[1], r[2]): r[3] for r in rows if r[0] == section}


def _record(section, tmp):
    lines = []
    if section == "desc":
        for name, sdb in desc_cases().items():
            for mode, m in MODES.items():
                save_desc(sdb, os.path.join(tmp, "img"), m)
                lines.append(f"desc\t{name}\t{mode}\t{header_hex(os.path.join(tmp, 'img'))}")
    else:
        for name, spec in synth_cases().items():
            for mode, m in MODES.items():
                db = ra.PhyloKmerDB.synthetic(spec, table_mode=m)
                db.save(os.path.join(tmp, "img"))
                db.close()
                lines.append(f"synth\t{name}\t{mode}\t{header_hex(os.path.join(tmp, 'img'))}")
    return lines


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        print("\n".join(_record(sys.argv[2], tmp)))
