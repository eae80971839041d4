"""GPU (-m gpu): the fast select of 16-lane groups -- a scan that keeps scores only, rounds that name the winning streams, and a
pass that finds each winner's slot by reading its stream again (rk_kernels.hip: heads3_*).  Slot branch + 1 of the score vector
belongs to stream slot mod 64, so two branches 64 apart share a stream.

Small databases with planted rows make every read's score vector a known shape: several of the K best in one stream (different and
equal scores), equal scores across streams in either order of stream id against branch id, ties that straddle rank K (exact only
through the fallback), fewer than K branches touched down to none, K = 1 ... 16, trees of every (n_branches + 1) mod 4 and with
streams of unequal length, DNA and amino acids.  Every read goes through the product library into result buffers pre-filled with 0xFF
and is compared with the oracle bit for bit; where scores are equal the engine's order -- score descending, branch ascending -- is
checked against a plain sort of the oracle's score vector (tests/util.py alone compares such reads as sets)."""
import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import synth
from oracle import oracle as O
from tests.util import compare_with_oracle

pytestmark = pytest.mark.gpu

STREAMS = 64  # 4 streams in each of a group's 16 lanes


def planted_db(alphabet, k, nb, n_keys, seed):
    """rows of up to 24 entries: branches 64 apart (one stream), runs of neighbours, random sets and mixtures; scores drawn from
    1, 2, 3 or 8 dyadic fractions of the threshold, so that equal sums are everywhere.  Returns the database and the keys' digits."""
    rng = np.random.default_rng(seed)
    digits = rng.integers(0, alphabet, (n_keys, k))
    dense = (digits.astype(np.uint64) * (np.uint64(alphabet) ** np.arange(k, dtype=np.uint64))).sum(1).astype(np.uint64)
    _, first = np.unique(dense, return_index=True)
    first.sort()
    digits, dense = digits[first], dense[first]
    thr, thr_log10 = synth.thresholds(1.5, alphabet, k)
    rows_b, rows_s = [], []
    for _ in range(len(dense)):
        m = int(rng.integers(1, min(24, nb - 1) + 1))
        kind = int(rng.integers(0, 4))
        b = set()
        if kind in (0, 3) and nb > STREAMS + 2:  # one stream: b, b + 64, b + 128 ...
            b0 = int(rng.integers(1, min(STREAMS, nb - STREAMS - 1) + 1))
            same = np.arange(b0, nb, STREAMS)
            b.update(rng.choice(same, size=min(len(same), m if kind == 0 else 3), replace=False).tolist())
        if kind == 1:  # neighbours
            b0 = int(rng.integers(1, nb - m + 1))
            b.update(range(b0, b0 + m))
        if len(b) < m:  # anywhere
            b.update(rng.choice(np.arange(1, nb), size=m - len(b), replace=False).tolist())
        b = np.array(sorted(b), dtype=np.uint16)
        palette = int(rng.choice([1, 2, 3, 8]))
        s = (rng.integers(1, palette + 1, len(b)).astype(np.float32) / np.float32(8.0)) * np.float32(thr_log10)
        rows_b.append(b)
        rows_s.append(s.astype(np.float32))
    off = np.zeros(len(dense) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in rows_b], out=off[1:])
    sdb = synth.SynthDB(alphabet, k, nb, thr, thr_log10, synth.dense_to_code(alphabet, k, dense), off,
                        np.concatenate(rows_b).astype(np.uint16), np.concatenate(rows_s).astype(np.float32), seed)
    return sdb, digits


def planted_reads(alphabet, k, digits, n, L, seed):
    """random reads of L symbols carrying none, one, two or three of the keys"""
    rng = np.random.default_rng(seed)
    letters = synth.AA_LETTERS if alphabet == 20 else synth.DNA_LETTERS
    st = rng.integers(0, alphabet, (n, L))
    how_many = rng.choice([0, 1, 2, 3], size=n, p=[0.06, 0.5, 0.3, 0.14])
    slots = [0, L // 3, 2 * L // 3]
    for r in range(n):
        for j in range(how_many[r]):
            at = slots[j] + int(rng.integers(0, L // 3 - k))
            st[r, at:at + k] = digits[int(rng.integers(0, len(digits)))]
    seq = np.ascontiguousarray(letters[st.reshape(-1)])
    return seq, (np.arange(n + 1, dtype=np.uint64) * np.uint64(L))


def place_prefilled(pp, packed, n, L, K):
    """rk_place_packed_device into result tensors pre-filled with 0xFF bytes; every read must have been written"""
    import torch
    dev = torch.device("cuda", 0)
    out = dict(n_rows=torch.full((n,), 0xFF, dtype=torch.uint8, device=dev),
               branch=torch.full((n, K), -1, dtype=torch.int16, device=dev),
               score=torch.full((n, K), -1, dtype=torch.int32, device=dev).view(torch.float32),
               lwr=torch.full((n, K), -1, dtype=torch.int64, device=dev).view(torch.float64),
               flags=torch.full((n,), -1, dtype=torch.int32, device=dev))
    pp.place_packed(torch.from_numpy(packed.view(np.int32)).to(dev), fixed_len=L, out=out, keepAtMost=K)
    torch.cuda.synchronize()
    o = {f: t.cpu().numpy() for f, t in out.items()}
    unwritten = np.nonzero((o["n_rows"] == 0xFF) | (o["flags"] == -1))[0]
    assert len(unwritten) == 0, f"{len(unwritten)} of {n} reads never written (first: {unwritten[:8]})"
    return ra.Placements(o["n_rows"], o["branch"].view(np.uint16), o["score"], o["lwr"], o["flags"].view(np.uint32), {})


def sorted_vectors(odb, seq, off):
    """per read: the touched branches by (score descending, branch ascending) and their scores' bits"""
    res = []
    for r in range(len(off) - 1):
        S, touched, _ = odb.score_vector(bytes(seq[int(off[r]):int(off[r + 1])]))
        touched = np.sort(touched.astype(np.int64))
        order = touched[np.argsort(-S[touched].astype(np.float64), kind="stable")]
        res.append((order, S[order].view(np.uint32)))
    return res


def shapes_met(vectors, K, seen):
    """which of the cases this file is about the reads' score vectors hold, for keep_at_most K"""
    for order, bits in vectors:
        if len(order) == 0:
            seen["none"] += 1
            continue
        if len(order) < K:
            seen["fewer"] += 1
        if len(order) > K and bits[K - 1] == bits[K]:
            seen["straddle"] += 1
        top, tb = order[:K], bits[:K]
        stream = (top + 1) % STREAMS
        for i in range(len(top)):
            for j in range(i + 1, len(top)):
                if stream[i] == stream[j]:
                    seen["stream_equal" if tb[i] == tb[j] else "stream_differ"] += 1
                elif tb[i] == tb[j]:  # top is sorted: top[i] < top[j] here
                    seen["tie_ids_along" if stream[i] < stream[j] else "tie_ids_against"] += 1


def check_tree(alphabet, k, nb, L, n_reads, seed, need):
    sdb, digits = planted_db(alphabet, k, nb, 300, seed)
    odb = O.OracleDB.from_synth(sdb)
    seq, off = planted_reads(alphabet, k, digits, n_reads, L, seed + 1)
    vectors = sorted_vectors(odb, seq, off)
    seen = dict.fromkeys(["none", "fewer", "straddle", "stream_equal", "stream_differ", "tie_ids_along", "tie_ids_against"], 0)
    for lanes in (0, 16):
        db = ra.PhyloKmerDB.from_synth(sdb, device=0)
        try:
            db.set_lanes_per_read(lanes)
            pp = ra.PlacementProcess(db)
            packed, _, _ = pp.pack_reads_host(seq, off)
            for K in range(1, 17):
                ref = odb.place(seq, off, keep_at_most=K, keep_factor=0.01, ns_bound=pp.ns_bound)
                got = place_prefilled(pp, packed, n_reads, L, K)
                compare_with_oracle(got, ref, odb, seq, off)
                for r, (order, bits) in enumerate(vectors):
                    n = int(got.n_rows[r])
                    assert n <= min(K, len(order)), (r, K, n, len(order))
                    assert np.array_equal(got.branch[r, :n].astype(np.int64), order[:n]) and \
                        np.array_equal(got.score[r, :n].view(np.uint32), bits[:n]), \
                        f"{db.kernel_name()} K={K} read {r}: got {got.branch[r, :n]} {got.score[r, :n]}, sorted vector {order[:K]} {bits[:K].view(np.float32)}"
                if lanes == 0:
                    shapes_met(vectors, K, seen)
        finally:
            db.close()
    print(nb, seen)
    missing = [c for c in need if seen[c] == 0]
    assert not missing, f"{nb} branches: no read with {missing} ({seen})"


SMALL = ["none", "fewer", "straddle", "tie_ids_along"]  # (below 64 slots a slot is its own stream id: no pair against the order, none in one stream)
ALL = SMALL + ["tie_ids_against", "stream_equal", "stream_differ"]


@pytest.mark.parametrize("nb", [30, 62, 63, 64, 65])
def test_trees_within_one_quad_per_lane(nb):
    """n_branches + 1 = 31 ... 66: (n_branches + 1) mod 4 = 3, 3, 0, 1, 2; most lanes' streams are empty, a stream holds one word
    (two for the first slots of the 65- and 66-slot vectors)"""
    check_tree(4, 10, nb, 150, 400, 100 + nb, SMALL)


@pytest.mark.parametrize("nb", [399, 400, 997, 998, 999])
def test_trees_with_streams_of_unequal_length(nb):
    """(n_branches + 1) mod 4 = 0, 1, 2, 3, 0; 100 / 101 / 250 quads over 16 lanes: the first lanes' streams are a word longer"""
    check_tree(4, 10, nb, 150, 500, 200 + nb, ALL)


def test_amino_acid_tree():
    """the 5-bit instance of the same kernel (C4's shape: k = 5, 399 branches, 100 residues)"""
    check_tree(20, 5, 399, 100, 500, 7, ALL)
