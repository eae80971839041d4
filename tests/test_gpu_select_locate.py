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
from oracle import oracle as O
from tests.planted import place_prefilled, planted_db, planted_reads, shapes_met, sorted_vectors  # (shared with tests/test_gpu_tie_order.py)
from tests.util import compare_with_oracle

pytestmark = pytest.mark.gpu


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
