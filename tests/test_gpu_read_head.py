"""GPU (-m gpu): what a packed read's length and incoming flags mean -- read_head in rk_kernels.hip -- in EVERY kernel that takes packed
reads.  The composed calls lean on it from outside (two-strand placement passes the output flag array as flags_in, six-frame
placement the DNA packer's flags), so a kernel that drifts would be a wrong answer on the trees it serves only.

The batch is a planted tree's own reads (tests/planted.py) plus edge reads, passed with a length per read:
  * lengths 0, k - 1, k, k + 1 and the full L;
  * a read that fills its record's words and whose length entry claims four times as many symbols: placed as the read its words hold;
  * reads with BAD_CHAR, TOO_LONG, AMBIGUOUS, AMBIGUOUS | TOO_LONG, BAD_CHAR on a read shorter than k, and TOO_SHORT alone in flags_in.
Without characters every flagged read is written with no rows and exactly the kept input bits (TOO_SHORT added below k symbols), and
TOO_SHORT alone is ignored: the read is placed.  With characters the plainly ambiguous read is place_ascii_kernel's and the
AMBIGUOUS | TOO_LONG one still the packed kernel's, with no rows.  Result buffers are pre-filled with 0xFF; the placed reads meet the
parity bar of tests/util.py against the oracle on the reads' own characters; the kernels that serve one tree agree exactly; and
rk_count_work_device counts the k-mers the oracle looks up: the sum of Q over the unflagged reads."""
import functools

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, synth
from tests import planted as P
from tests.test_gpu_tie_order import ROUTES, assert_same, route_db
from tests.util import compare_with_oracle

pytestmark = pytest.mark.gpu

KS = (7, 16)
BAD, SHORT, AMB, LONG = _lib.RK_FLAG_BAD_CHAR, _lib.RK_FLAG_TOO_SHORT, _lib.RK_FLAG_AMBIGUOUS, _lib.RK_FLAG_TOO_LONG


@functools.lru_cache(maxsize=None)
def batch(name):
    """characters, offsets, claimed lengths and forced flags_in of the batch on planted tree `name`, with the expectations' index sets"""
    sdb, odb, seq, off, vectors = P.tree(name)
    n0, L, k = len(off) - 1, int(off[1]), sdb.k
    words = (L * sdb.bits + 31) // 32
    cap = words * 32 // sdb.bits  # symbols the record's words hold
    letters = synth.AA_LETTERS if sdb.alphabet == 20 else synth.DNA_LETTERS
    src = next(seq[int(off[r]):int(off[r + 1])] for r in range(n0) if len(vectors[r][0]) >= 8)  # a read that touches several branches
    full = np.concatenate([src, letters[np.random.default_rng(5).integers(0, sdb.alphabet, cap - L)]])  # fills every word
    amb = src.copy()
    amb[-1] = ord("X") if sdb.alphabet == 20 else ord("N")
    reads = [seq[int(off[r]):int(off[r + 1])] for r in range(n0)]
    force = {}   # read -> flags_in instead of the packer's
    want = {}    # read -> flags of a read no kernel places
    reads += [src[:0], src[:k - 1], src[:k], src[:k + 1], src]
    over = len(reads)
    reads.append(full)
    for fin, read in ((BAD, src), (LONG, src), (AMB | LONG, amb), (BAD, src[:k - 1])):
        force[len(reads)] = fin
        want[len(reads)] = fin | (SHORT if len(read) < k else 0)
        reads.append(read)
    force[len(reads)] = SHORT  # alone: ignored on input, the read is placed
    reads.append(src)
    amb_at = len(reads)
    reads.append(amb)
    lens = np.array([len(r) for r in reads], np.uint32)
    claimed = lens.copy()
    claimed[over] = 4 * cap
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    clean = np.array([r for r in range(len(reads)) if r not in want and r != amb_at])
    return dict(seq=np.ascontiguousarray(np.concatenate(reads)), off=offs, lens=lens, claimed=claimed, cap=cap, force=force, want=want,
                clean=clean, amb_at=amb_at, with_amb=np.append(clean, amb_at))


@functools.lru_cache(maxsize=None)
def oracle(name, K):
    """the oracle on the characters of the placed reads, the ambiguous one last"""
    b, odb = batch(name), P.tree(name)[1]
    parts = [b["seq"][int(b["off"][r]):int(b["off"][r + 1])] for r in b["with_amb"]]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    return np.concatenate(parts), off, odb.place(np.concatenate(parts), off, keep_at_most=K)


def rows(got, idx):
    return ra.Placements(got.n_rows[idx], got.branch[idx], got.score[idx], got.lwr[idx], got.flags[idx], {})


def run_batch(name, route, monkeypatch):
    """{(K, characters handed over): Placements} of the batch through the kernel of `route`, every expectation of the module asserted"""
    b, odb = batch(name), P.tree(name)[1]
    k, n = P.tree(name)[0].k, len(b["lens"])
    res = {}
    with route_db(name, route, monkeypatch) as db:
        pp = ra.PlacementProcess(db)
        packed, lens, flags = pp.pack_reads_host(b["seq"], b["off"], max_len=b["cap"])
        assert np.array_equal(lens, b["lens"]) and packed.shape[1] * 32 // db.info.bits_per_symbol == b["cap"]
        # (the packer's own flags: the ambiguity code, and TOO_SHORT on the two reads below k symbols -- which the kernels take from the length)
        assert flags[b["amb_at"]] == AMB and not (flags[b["clean"]] & ~np.uint32(SHORT)).any()
        for r, fin in b["force"].items():
            flags[r] = fin
        for K in KS if route != "lanes8" else KS[:1]:  # (8 lanes serve keep_at_most <= 8)
            seq_o, off_o, ref = oracle(name, K)
            for chars in (False, True):
                what = f"{name} {route} K={K} characters={chars}"
                got = P.place_prefilled(pp, packed, n, 0, K, amb="mean", flags=flags, lens=b["claimed"],
                                        **(dict(seq=b["seq"], off=b["off"]) if chars else {}))
                for r, fl in b["want"].items():
                    assert got.n_rows[r] == 0 and got.flags[r] == fl, (what, r, got.n_rows[r], hex(got.flags[r]), hex(fl))
                if chars:
                    st = compare_with_oracle(rows(got, b["with_amb"]), ref, odb, seq_o, off_o)
                else:
                    assert got.n_rows[b["amb_at"]] == 0 and got.flags[b["amb_at"]] == AMB, what
                    m = len(b["clean"])
                    st = compare_with_oracle(rows(got, b["clean"]), {f: v[:m] for f, v in ref.items() if f != "counters"}, odb, seq_o, off_o[:m + 1])
                assert st["placed"] > len(b["clean"]) // 2, (what, st)
                res[K, chars] = got
        import torch
        dev = lambda a: torch.from_numpy(a.view(np.int32)).to(torch.device("cuda", 0))
        probed = pp.count_work(dev(packed), lens=dev(b["claimed"]), flags_in=dev(flags))["kmers_probed"]
        clean_lens = np.minimum(b["claimed"], b["cap"])[b["clean"]].astype(np.int64)
        assert probed == int(np.maximum(clean_lens - k + 1, 0).sum()), (name, route, probed)
        seq_o, off_o, _ = oracle(name, KS[0])
        m = len(b["clean"])
        assert probed == odb.place(seq_o[:int(off_o[m])], off_o[:m + 1], keep_at_most=1)["counters"]["kmers"], (name, route, probed)
    return res


@pytest.mark.parametrize("name,routes", [
    ("dna30", ["lanes0", "lanes8", "lanes32", "lanes64"]),
    ("aa399", ["lanes0", "lanes64"]),
    ("dna1277", ["windowed"]),
    ("dna4501", ["sorted"]),
    ("aa1999", ["sorted"]),
    ("dna2801", ["hash", "hash_small"]),
    ("wg13301", ["wg1", "wg2"]),
], ids=lambda v: v if isinstance(v, str) else None)
def test_read_head(name, routes, monkeypatch, dev_lib):
    assert all(r in ROUTES for r in routes)
    first = None
    for route in routes:
        res = run_batch(name, route, monkeypatch)
        if first is None:
            first, first_route = res, route
            continue
        for key, got in res.items():
            assert_same(got, first[key], f"{name}: {route} against {first_route}, keep_at_most {key[0]} characters {key[1]}")
