"""GPU (-m gpu): the accumulate step of the dense 24-entry row units (rk_slots24.h; accumulate_units<..., D24> in rk_kernels.hip) on
small DNA and amino-acid databases whose rows end on every side of the 8-, 16- and 24-entry marks of a unit, with branch ids 0 and
1 022 (the largest the view's ten-bit slots hold), once with every score at or above the threshold (the `mono` first touch) and once
with scores below it.  Bar: the oracle's placements for every read -- flags, n_rows, branches, score bits, LWR -- written into
0xFF-filled result buffers, so a read that was never placed fails; and the canonical 16-entry units' results, bit for bit."""
import numpy as np
import pytest

import rappas_amd as ra
from oracle import oracle as O
from rappas_amd import synth
from tests.util import compare_with_oracle

pytestmark = pytest.mark.gpu

ROW_LENS = [1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 48]
N_BRANCHES = 1023


def rows_db(alphabet, k, seed, below_threshold):
    """every k-mer present, row lengths cycled from ROW_LENS (11 is coprime to 4^k and 20^k: every length meets every lane phase),
    distinct random branches per row; the first two rows hold branch 0 and branch 1 022"""
    rng = np.random.default_rng(seed)
    space = alphabet ** k
    key_codes = synth.dense_to_code(alphabet, k, np.arange(space, dtype=np.uint64))
    rl = np.resize(np.asarray(ROW_LENS, dtype=np.int64), space)
    off = np.zeros(space + 1, dtype=np.uint64)
    np.cumsum(rl, out=off[1:])
    br = np.concatenate([rng.choice(N_BRANCHES, size=int(n), replace=False) for n in rl]).astype(np.uint16)
    br[0] = 0
    a, e = int(off[1]), int(off[2])
    if N_BRANCHES - 1 not in br[a:e]:
        br[a if br[a] != 0 else a + 1] = N_BRANCHES - 1
    # ... and in the last place of a 24- and a 48-entry row (entry 16 + 7 of a unit: lane 7's second slot)
    for r in (8, 10):
        a, e = int(off[r]), int(off[r + 1])
        if N_BRANCHES - 1 not in br[a:e]:
            br[e - 1] = N_BRANCHES - 1
    thr, t = synth.thresholds(1.5, alphabet, k)
    sc = (t * rng.random(len(br), dtype=np.float32)).astype(np.float32)
    low = rng.random(len(br)) < below_threshold
    sc[low] = (t * (1.0 + rng.random(int(low.sum()), dtype=np.float32))).astype(np.float32)
    assert bool((sc < t).any()) == (below_threshold > 0)
    return synth.SynthDB(alphabet, k, N_BRANCHES, thr, t, key_codes, off, br, sc, seed)


def place_into_filled_buffers(db, seq, off, L, K):
    import torch
    pp = ra.PlacementProcess(db)
    packed, _, _ = pp.pack_reads_host(seq, off)
    n = len(off) - 1
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
    return ra.Placements(o["n_rows"], o["branch"].view(np.uint16), o["score"], o["lwr"], o["flags"].view(np.uint32), {}), pp.ns_bound


@pytest.mark.parametrize("alphabet,k,L,n_reads", [(4, 5, 150, 3000), (20, 3, 100, 2000)], ids=["dna", "aa"])
@pytest.mark.parametrize("below_threshold", [0.0, 0.3], ids=["mono", "below_threshold"])
@pytest.mark.parametrize("K", [7])
def test_dense_step_against_the_oracle(dev_lib, monkeypatch, alphabet, k, L, n_reads, below_threshold, K):
    sdb = rows_db(alphabet, k, seed=61 + alphabet, below_threshold=below_threshold)
    seq, off = synth.make_reads(alphabet, n_reads, L, seed=62 + alphabet)
    odb = O.OracleDB.from_synth(sdb)
    monkeypatch.delenv("RK_NO_DENSE_UNITS", raising=False)
    dense = ra.PhyloKmerDB.from_synth(sdb, device=0)
    monkeypatch.setenv("RK_NO_DENSE_UNITS", "1")
    canon = ra.PhyloKmerDB.from_synth(sdb, device=0)
    monkeypatch.delenv("RK_NO_DENSE_UNITS", raising=False)
    try:
        assert dense.kernel_name().startswith("place_packed16_kernel<") and "ROW24," in dense.kernel_name(), dense.kernel_name()
        assert "ROW24," not in canon.kernel_name(), canon.kernel_name()
        got, ns_bound = place_into_filled_buffers(dense, seq, off, L, K)
        ref = odb.place(seq, off, keep_at_most=K, keep_factor=0.01, ns_bound=ns_bound)
        st = compare_with_oracle(got, ref, odb, seq, off)  # every read: nothing sampled
        assert st["n"] == n_reads and st["placed"] > n_reads // 2, st
        want, _ = place_into_filled_buffers(canon, seq, off, L, K)
        for f in ("n_rows", "branch", "flags"):
            assert np.array_equal(getattr(got, f), getattr(want, f)), f
        assert np.array_equal(got.score.view(np.uint32), want.score.view(np.uint32))
        assert np.array_equal(got.lwr.view(np.uint64), want.lwr.view(np.uint64))
    finally:
        dense.close()
        canon.close()
