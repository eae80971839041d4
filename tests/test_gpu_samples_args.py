"""The cases of test_samples_args.py that need a tree handle: what every _device, _batch and _work_bytes call of the sample level
 answers to one bad argument -- return code and the whole text --, and the workspace sizes of the four analyses
against tests/golden/samples_work_bytes.tsv.  Every refused call fails before anything is launched; the sizes launch and allocate
nothing; the only kernels run are those of one small pooled batch, which leaves a buffer of two samples in the handle."""
import os

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, synth
from rappas_amd._lib import RK_ERR_INVALID
from tests import kr_ref as R
from tests import test_samples_args as A

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples_work_bytes.tsv")
SIZE_CALLS = {"rk_kr_work_bytes": False, "rk_squash_work_bytes": False, "rk_kmeans_work_bytes": True, "rk_epca_work_bytes": True}  # takes k
SIZER = {"rk_kr_distances_device": "rk_kr_work_bytes", "rk_squash_device": "rk_squash_work_bytes", "rk_kmeans_device": "rk_kmeans_work_bytes",
         "rk_epca_device": "rk_epca_work_bytes"}


def grid():
    """(call, B, S, k): B = 2048 | 2049 either side of the one-chunk rule; at B = 2049, S = 4096 the pair partials are 2^28 bytes and
    still used, at B = 6000 not; k = 0 where the call takes none.  A refused shape is in the table with 0 bytes.  Behind the grid of
    each call that takes k, the shape the refused calls below start from (k = 2)."""
    for call, has_k in SIZE_CALLS.items():
        for B in (5, 2048, 2049, 6000):
            for S in (1, 2, 3, 64, 65, 4096, 65535):
                for k in ((1, 8, 64) if has_k else (0,)):
                    yield call, B, S, k
        if has_k:
            yield call, A.B, A.S, 2


def golden():
    rows = {}
    with open(GOLDEN) as f:
        for line in f:
            if not line.startswith("#"):
                call, B, S, k, n = line.split()
                rows[call, int(B), int(S), int(k)] = int(n)
    return rows


def size_of(lib, call, tree, S, k):
    return int(getattr(lib, call)(tree, S, k) if SIZE_CALLS[call] else getattr(lib, call)(tree, S))


def test_workspace_sizes_are_the_recorded_ones():
    want, lib = golden(), _lib.load()
    assert set(want) == set(grid())
    assert want["rk_kr_work_bytes", 2049, 4096, 0] - want["rk_kr_work_bytes", 2048, 4096, 0] == 3 * 4096 * 8 + (1 << 28)  # two chunks of partials
    assert want["rk_kr_work_bytes", 6000, 4096, 0] == 3 * 4096 * 6000 * 8                                               # none
    trees = {}
    try:
        for call, B, S, k in grid():
            if B not in trees:
                trees[B] = ra.EdgeTree(*R.random_tree(B, B))
            assert size_of(lib, call, trees[B].handle, S, k) == want[call, B, S, k], (call, B, S, k)
    finally:
        for et in trees.values():
            et.close()


class Device:
    """a valid device call's arguments: the tree of test_samples_args.py and one of six nodes, a database of five branches, the arrays
    of A.values() on the device as addresses, a workspace larger than any of the calls needs"""

    def __init__(self):
        import torch
        v = A.values()
        self.tree = ra.EdgeTree(v["parent"], v["bl"])
        self.tree6 = ra.EdgeTree(np.array([-1, 0, 0, 2, 2, 1], np.int32), np.array([0, 1, 3, 2, 4, 1], np.float32))
        self.db = ra.PhyloKmerDB.from_synth(synth.make_db(4, 6, A.B, 40, 80, seed=1), device=0)
        self.keep = {n: torch.from_numpy(x.view(np.uint8)).cuda() for n, x in v.items() if isinstance(x, np.ndarray) and n not in ("parent", "bl")}
        self.keep.update({"res." + n: torch.from_numpy(x.view(np.uint8)).cuda() for n, x in v["res"].items()})
        self.keep["work"] = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
        self.at = {n: t.data_ptr() for n, t in self.keep.items()}
        self.res = {n: self.at["res." + n] for n in ("n_rows", "branch", "lwr")}
        want = golden()
        self.need = {c: want[c, A.B, A.S, 2 if has_k else 0] for c, has_k in SIZE_CALLS.items()}  # by the name of the _work_bytes call

    def base(self, call):
        """the device arrays and the exact workspace size for a _device call, the host arrays of A.values() for a _batch call"""
        if call.endswith("_batch"):
            return dict(db=self.db.handle, tree=self.tree.handle)
        own = {n: a for n, a in self.at.items() if "." not in n}
        own.update(tree=self.tree.handle, res=self.res, work_bytes=self.need.get(SIZER.get(call), 0))
        return own

    def close(self):
        self.tree.close()
        self.tree6.close()
        self.db.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


SAMPLES, SAMPLES_2 = A.SAMPLES, A.SAMPLES_2
NO_RESULT = "null result array (n_rows, branch and lwr are read)"
ROWS = "the rows must be 8-byte aligned, the count 4-byte aligned"
WORDS = "the doubles must be 8-byte aligned, the 32-bit words 4-byte aligned"
RAW = "the raw output must be 8-byte aligned, the info words 4-byte aligned"
OTHER_TREE = "the tree has 6 branches on device 0, the database 5 on device 0"
NO_BUFFER = "the handle holds the buffer of 0 samples, not of 3 (the last per-sample profile-only call leaves it)"


def workspace(d, call):
    """null, one byte short, off by 8 from 16-byte alignment"""
    need = d.need[SIZER[call]]
    return [(dict(work=None), f"workspace of 0 bytes, {need} needed ({SIZER[call]})"),
            (dict(work_bytes=need - 1), f"workspace of {need - 1} bytes, {need} needed ({SIZER[call]})"),
            (dict(work=d.at["work"] + 8), "the workspace must be 16-byte aligned")]


def refused(d):
    """call -> (what is changed, the text behind "<call>: ")"""
    at, no_lwr = d.at, dict(d.res, lwr=None)
    seeds_far, seeds_same = np.array([0, 3], np.uint32), np.array([1, 1], np.uint32)
    return {
        "rk_clade_masses_device": [
            (dict(tree=None), "null tree"), (dict(S=0), SAMPLES % 0), (dict(S=65536), SAMPLES % 65536),
            (dict(masses=None), "null mass buffer"), (dict(clade=None), "null output")],
        "rk_kr_distances_device": [
            (dict(tree=None), "null tree"), (dict(S=0), SAMPLES % 0), (dict(S=65536), SAMPLES % 65536),
            (dict(masses=None), "null mass buffer"), (dict(D=None), "null output")] + workspace(d, "rk_kr_distances_device"),
        "rk_squash_device": [
            (dict(tree=None), "null tree"), (dict(S=1), SAMPLES_2 % 1), (dict(S=4097), SAMPLES_2 % 4097),
            (dict(masses=None), "null mass buffer"), (dict(merges=None), "null output"), (dict(n_merges=None), "null output"),
            (dict(merges=at["merges"] + 4), ROWS), (dict(n_merges=at["n_merges"] + 2), ROWS)] + workspace(d, "rk_squash_device"),
        "rk_kmeans_device": [
            (dict(tree=None), "null tree"), (dict(S=0), SAMPLES % 0), (dict(S=65536), SAMPLES % 65536),
            (dict(k=0), "k=0 clusters must be in 1..64"), (dict(k=65), "k=65 clusters must be in 1..64"),
            (dict(rounds=0), "max_rounds=0 must be in 1..1024"), (dict(rounds=1025), "max_rounds=1025 must be in 1..1024"),
            (dict(masses=None), "null mass buffer"), (dict(assign=None), "null output"), (dict(dist=None), "null output"),
            (dict(sizes=None), "null output"), (dict(within=None), "null output"), (dict(info=None), "null output"),
            (dict(dist=at["dist"] + 4), WORDS), (dict(within=at["within"] + 4), WORDS), (dict(centroids=at["centroids"] + 4), WORDS),
            (dict(assign=at["assign"] + 2), WORDS), (dict(sizes=at["sizes"] + 2), WORDS), (dict(info=at["info"] + 2), WORDS),
            (dict(seeds=seeds_far), "seeds[1]=3, the buffer has 3 samples"),
            (dict(seeds=seeds_same), "seeds[0] and seeds[1] are both sample 1")] + workspace(d, "rk_kmeans_device"),
        "rk_epca_device": [
            (dict(tree=None), "null tree"), (dict(S=1), SAMPLES_2 % 1), (dict(S=4097), SAMPLES_2 % 4097),
            (dict(k=0), "k=0 components must be in 1..8"), (dict(k=9), "k=9 components must be in 1..8"),
            (dict(iters=0), "iters=0 must be in 1..10000"), (dict(iters=10001), "iters=10001 must be in 1..10000"),
            (dict(masses=None), "null mass buffer"), (dict(raw=None), "null output"), (dict(info=None), "null output"),
            (dict(raw=at["raw"] + 4), RAW), (dict(info=at["info"] + 2), RAW)] + workspace(d, "rk_epca_device"),
        "rk_edpl_device": [
            (dict(tree=None), "null tree"), (dict(K=0), "keep_at_most=0 outside 1..16"), (dict(K=17), "keep_at_most=17 outside 1..16"),
            (dict(n_reads=1 << 32), "n_reads=4294967296, at most 2^32 - 1 per call"), (dict(res=None), NO_RESULT), (dict(res=no_lwr), NO_RESULT),
            (dict(edpl=None), "null output")],
        "rk_kr_distances_batch": [
            (dict(db=None), "null handle"), (dict(tree=None), "null tree"), (dict(S=0), SAMPLES % 0), (dict(S=65536), SAMPLES % 65536),
            (dict(D=None), "null output"), (dict(tree=d.tree6.handle), OTHER_TREE), (dict(masses=None), NO_BUFFER)],
        "rk_squash_batch": [
            (dict(db=None), "null handle"), (dict(tree=None), "null tree"), (dict(S=1), SAMPLES_2 % 1), (dict(S=4097), SAMPLES_2 % 4097),
            (dict(merges=None), "null output"), (dict(n_merges=None), "null output"), (dict(tree=d.tree6.handle), OTHER_TREE),
            (dict(masses=None), NO_BUFFER)],
        "rk_kmeans_batch": [
            (dict(db=None), "null handle"), (dict(tree=None), "null tree"), (dict(S=0), SAMPLES % 0), (dict(S=65536), SAMPLES % 65536),
            (dict(k=0), "k=0 clusters must be in 1..64"), (dict(k=65), "k=65 clusters must be in 1..64"),
            (dict(rounds=0), "max_rounds=0 must be in 1..1024"), (dict(rounds=1025), "max_rounds=1025 must be in 1..1024"),
            (dict(assign=None), "null output"), (dict(dist=None), "null output"), (dict(sizes=None), "null output"),
            (dict(within=None), "null output"), (dict(info=None), "null output"), (dict(tree=d.tree6.handle), OTHER_TREE),
            (dict(masses=None), NO_BUFFER)],
        "rk_epca_batch": [
            (dict(db=None), "null handle"), (dict(tree=None), "null tree"), (dict(S=1), SAMPLES_2 % 1), (dict(S=4097), SAMPLES_2 % 4097),
            (dict(k=0), "k=0 components must be in 1..8"), (dict(k=9), "k=9 components must be in 1..8"),
            (dict(iters=0), "iters=0 must be in 1..10000"), (dict(iters=10001), "iters=10001 must be in 1..10000"),
            (dict(raw=None), "null output"), (dict(info=None), "null output"), (dict(tree=d.tree6.handle), OTHER_TREE),
            (dict(masses=None), NO_BUFFER)],
        "rk_edpl_batch": [
            (dict(db=None), "null handle"), (dict(tree=None), "null tree"), (dict(K=0), "keep_at_most=0 outside 1..16"),
            (dict(K=17), "keep_at_most=17 outside 1..16"), (dict(n_reads=1 << 32), "n_reads=4294967296, at most 2^32 - 1 per call"),
            (dict(res=None), NO_RESULT), (dict(res=dict(A.values()["res"], lwr=None)), NO_RESULT), (dict(edpl=None), "null output"),
            (dict(tree=d.tree6.handle), OTHER_TREE)],
    }


CALLS = [c for c in A.CALLS if c.endswith(("_device", "_batch"))]


@pytest.mark.parametrize("call", CALLS)
def test_one_bad_argument_is_refused_with_its_text(dev, call):
    for i, (change, text) in enumerate(refused(dev)[call]):
        assert A.run(_lib.load(), call, change, dev.base(call)) == (RK_ERR_INVALID, f"{call}: {text}"), (i, change)


def test_a_seed_the_batch_call_hands_down_is_refused_by_the_device_call(dev):
    """(the seeds are tested where the launches are made: the text names that call)"""
    got = A.run(_lib.load(), "rk_kmeans_batch", dict(seeds=np.array([0, 3], np.uint32)), dev.base("rk_kmeans_batch"))
    assert got == (RK_ERR_INVALID, "rk_kmeans_device: seeds[1]=3, the buffer has 3 samples")


def test_a_size_out_of_range_is_zero_with_its_text(dev):
    cases = {
        "rk_kr_work_bytes": [(dict(S=0), SAMPLES % 0), (dict(S=65536), SAMPLES % 65536)],
        "rk_squash_work_bytes": [(dict(S=1), SAMPLES_2 % 1), (dict(S=4097), SAMPLES_2 % 4097)],
        "rk_kmeans_work_bytes": [(dict(S=0), SAMPLES % 0), (dict(S=65536), SAMPLES % 65536), (dict(k=0), "k=0 clusters must be in 1..64"),
                                 (dict(k=65), "k=65 clusters must be in 1..64")],
        "rk_epca_work_bytes": [(dict(S=1), SAMPLES_2 % 1), (dict(S=4097), SAMPLES_2 % 4097), (dict(k=0), "k=0 components must be in 1..8"),
                               (dict(k=9), "k=9 components must be in 1..8")],
    }
    for call, rows in cases.items():
        for change, text in rows:
            assert A.run(_lib.load(), call, change, dict(tree=dev.tree.handle)) == (0, f"{call}: {text}"), (call, change)
        assert A.run(_lib.load(), call, {}, dict(tree=dev.tree.handle))[0] == dev.need[call]


def test_the_buffer_of_another_number_of_samples_is_refused():
    """a pooled batch of two samples leaves its buffer in the handle: the four batch calls refuse to read it as one of three"""
    v = A.values()
    db = ra.PhyloKmerDB.from_synth(synth.make_db(4, 6, A.B, 40, 80, seed=1), device=0)
    tree = ra.EdgeTree(v["parent"], v["bl"])
    try:
        rng = np.random.default_rng(5)
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 8 * 30)]
        ra.PlacementProcess(db).processQueriesMassesSamples(seq, np.arange(9, dtype=np.uint64) * 30, 2, np.arange(8, dtype=np.uint32) % 2)
        text = "the handle holds the buffer of 2 samples, not of 3 (the last per-sample profile-only call leaves it)"
        for call in ("rk_kr_distances_batch", "rk_squash_batch", "rk_kmeans_batch", "rk_epca_batch"):
            got = A.run(_lib.load(), call, dict(masses=None), dict(db=db.handle, tree=tree.handle))
            assert got == (RK_ERR_INVALID, f"{call}: {text}"), call
    finally:
        tree.close()
        db.close()
