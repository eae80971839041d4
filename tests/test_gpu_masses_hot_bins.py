"""GPU (-m gpu): the edge masses of trees above the LDS limit -- the variant of masses_kernel that keeps a per-block LDS table of the
busiest bins in front of the global atomics -- through pp.accumulate_masses on hand-made result sets uploaded with
torch, for equality with the numpy restatement of the definition (tests/masses_ref.py).  The sets put their rows on a hot set of H
branches: H around the table's slot count, the ids as arithmetic progressions of stride 1, 2^10, 2^11, 2^12 and as a random set, so
that any power-of-two indexing of the table meets its best and its worst case without the test knowing the slot function; alone and
mixed with a uniform background; with rows whose branch is >= B inside the hot reads.  B = 4 095 is the first tree above the limit.
Nothing expected comes from the engine."""
import functools

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import synth
from tests import masses_ref as MR

pytestmark = pytest.mark.gpu

TREES = (4095, 20001, 65535)
KS = (1, 7, 16)
SLOTS = 512  # MASS_CACHE_SLOTS in rappas_amd/csrc/rk_masses.h: the slots of a block's table
HOT = (1, 7, SLOTS - 1, SLOTS, SLOTS + 1, 4 * SLOTS)
STRIDES = (1, 1 << 10, 1 << 11, 1 << 12, "random")
SMALL = (1, 63, 65)
BIG = 100003


def open_db(B):
    """a tiny hand-made database: only its number of branches matters here"""
    return ra.PhyloKmerDB.from_synth(synth.make_db(4, 6, B, 300, 1500, seed=B))


@pytest.fixture(scope="module")
def handles():
    dbs = {B: open_db(B) for B in TREES}
    yield dbs
    for db in dbs.values():
        db.close()


def hot_ids(B, H, stride, seed):
    """H distinct branch ids below B (every B here is odd, so a progression with a power-of-two stride does not repeat before B terms)"""
    rng = np.random.default_rng([seed, B, H, 5])
    if stride == "random":
        return rng.choice(B, H, replace=False).astype(np.uint16)
    ids = (int(rng.integers(0, B)) + np.arange(H, dtype=np.int64) * stride) % B
    assert len(np.unique(ids)) == H
    return ids.astype(np.uint16)


def make_hot_set(B, K, n, H, stride, mixed, seed=0):
    """MR.make_set(..., "mixed") -- planted rows with a branch >= B in row 0 and in the last row, n_rows beyond K, garbage behind n_rows,
    the special LWRs -- with every branch id below B replaced by one of the hot ids; `mixed`: in half of the reads only"""
    s = MR.make_set(B, K, n, seed=seed + 3, shape="mixed")
    rng = np.random.default_rng([seed, B, K, n, H, 9])
    ids = hot_ids(B, H, stride, seed)
    take = s.branch < B
    if mixed:
        take &= (rng.random(n) < 0.5)[:, None]
    s.branch[take] = ids[rng.integers(0, H, (n, K))][take]
    return s


def case_list(B, K, H):
    """(n, H, stride, mixed, weights kind) for one size of hot set: every stride, alone and mixed, at every n -- the three that fit
    one block and the one that takes 391 of them, each claiming slots, overflowing to the global atomics and flushing into the one
    buffer; the weights kinds go round.  The tests are parametrised by H as well so that a case stays at a second or two."""
    hi = HOT.index(H)
    out = []
    for si, stride in enumerate(STRIDES):
        for n in SMALL + (BIG,):
            for mixed in (False, True):
                out.append((n, H, stride, mixed, (None, "mixed", "zero", "one", "max")[(hi + si + n + mixed) % 5]))
    for kind in ("zero", "one", "max", "mixed"):  # each kind on the small and on the large size
        out.append((65, H, "random", False, kind))
        out.append((BIG, H, 1, True, kind))
    return out


def inputs(B, K, c):
    n, H, stride, mixed, kind = c
    return make_hot_set(B, K, n, H, stride, mixed), MR.make_weights(n, kind, seed=K)


@functools.lru_cache(maxsize=None)
def reference(B, K, c):
    s, w = inputs(B, K, c)
    m = MR.masses_ref(B, s.n_rows, s.branch, s.lwr, w)
    m.setflags(write=False)
    return m


def upload(s):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(n_rows=t(s.n_rows), branch=t(s.branch.view(np.int16)), lwr=t(s.lwr))


def dev_weights(w):
    import torch
    return None if w is None else torch.from_numpy(w.view(np.int32)).cuda()


def words(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("H", HOT)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", TREES)
def test_hot_sets_equal_the_reference(handles, B, K, H):
    pp = ra.PlacementProcess(handles[B])
    seen_skips = seen_hot_best = False
    for c in case_list(B, K, H):
        s, w = inputs(B, K, c)
        want = reference(B, K, c)
        got = words(pp.accumulate_masses(upload(s), weights=dev_weights(w)))
        assert np.array_equal(got, want), (c, np.flatnonzero(got != want)[:8])
        seen_skips |= bool(want[2 * B + 3] > 0)
        seen_hot_best |= c[0] == BIG and int((want[B:2 * B] > 0).sum()) >= 1
    assert seen_skips and seen_hot_best  # rows with a branch >= B sat inside the hot reads; the large sets placed reads


def test_the_hot_sets_are_hot_and_the_progressions_distinct():
    """the inputs themselves: a hot set alone puts every counted row on H branches (the reference says so), mixed sets more"""
    B, K = 20001, 7
    for H in HOT:
        c = (BIG, H, 1 << 10, False, None)
        s, _ = inputs(B, K, c)
        m = MR.masses_ref(B, s.n_rows, s.branch, s.lwr)
        assert int((m[B:2 * B] > 0).sum()) == H or H > 1000 and int((m[B:2 * B] > 0).sum()) > 1000
        assert m[2 * B + 3] > 0 and m[2 * B + 1] < m[2 * B]
    s, _ = inputs(B, K, (BIG, 7, 1, True, None))
    m = MR.masses_ref(B, s.n_rows, s.branch, s.lwr)
    assert int((m[B:2 * B] > 0).sum()) > 1000


@pytest.mark.parametrize("B", TREES)
def test_prefilled_buffer_and_two_streams_into_one_buffer(handles, B):
    import torch
    K, cut = 7, 40001
    pp = ra.PlacementProcess(handles[B])
    a = make_hot_set(B, K, BIG, 7, 1, True, seed=1)
    b = make_hot_set(B, K, BIG - cut, SLOTS + 1, 1 << 11, False, seed=2)
    wa, wb = MR.make_weights(BIG, "mixed", seed=1), MR.make_weights(BIG - cut, "mixed", seed=2)
    start = np.arange(2 * B + 4, dtype=np.uint64) * np.uint64(5)
    both = MR.concat(a, b)
    want = MR.masses_ref(B, both.n_rows, both.branch, both.lwr, np.concatenate([wa, wb]), masses=start)
    oa, ob, da, db_ = upload(a), upload(b), dev_weights(wa), dev_weights(wb)
    m = torch.from_numpy(start.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        assert pp.accumulate_masses(oa, weights=da, masses=m, stream=sa.cuda_stream) is m
    with torch.cuda.stream(sb):
        assert pp.accumulate_masses(ob, weights=db_, masses=m, stream=sb.cuda_stream) is m
    sa.synchronize()
    sb.synchronize()
    got = words(m)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


@pytest.mark.parametrize("H", HOT)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", TREES)
def test_forced_variants_give_identical_words(B, K, H, monkeypatch, dev_lib):
    """developer build: RK_MASSES_VARIANT=global (the atomics straight into the buffer) and =cache on every case above"""
    db = open_db(B)
    try:
        pp = ra.PlacementProcess(db)
        for c in case_list(B, K, H):
            s, w = inputs(B, K, c)
            out, dw = upload(s), dev_weights(w)
            got = {}
            for variant in ("global", "cache"):
                monkeypatch.setenv("RK_MASSES_VARIANT", variant)
                got[variant] = words(pp.accumulate_masses(out, weights=dw))
            assert np.array_equal(got["global"], got["cache"]), (c, np.flatnonzero(got["global"] != got["cache"])[:8])
            assert np.array_equal(got["cache"], reference(B, K, c)), c
    finally:
        db.close()
