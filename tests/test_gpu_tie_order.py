"""GPU (-m gpu): the engine's order among equal scores -- score descending, branch ascending ("Tie policy") -- in
EVERY placement kernel, against a plain sort of the oracle's score vector.  Since the first kernel of a windowed tree is chosen per
batch, a read can go through any of them; only this order makes its result independent of the kernel that placed it.

tests/planted.py plants the shapes that are hard for a select -- several of the K best in one stream or one lane (a whole quad of
them), equal scores whose stream order runs against the branch order, ties across rank K, fewer than K branches touched, none --
in each kernel's own layout (the stream stride of 8-, 32- and 64-lane groups, the windows of the windowed kernels, the hash table's
slots, a workgroup's wave ranges).  Every case runs every read for every listed keep_at_most and keep_factor 0.0 / 0.01 through
result buffers pre-filled with 0xFF and asserts: the parity bar of tests/util.py; rows equal to the first n_rows entries of the plain
sort, branch for branch and bit for bit; no read left unwritten; the kernel the case is meant for in kernel_name(); and that every
shape that can occur on the tree was met by a read (tests/test_planted_shapes.py asserts the same census without a GPU).  The kernels
that can serve one tree must also agree with each other exactly (n_rows, branch, flags, score bits, LWR)."""
import contextlib
import re

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib
from tests import golden_util as GU
from tests import planted as P
from tests.util import compare_with_oracle

pytestmark = pytest.mark.gpu

KNOBS = ["RK_NO_WSTREAM", "RK_NO_HASH", "RK_WSTREAM_ALWAYS", "RK_HASH_ALWAYS", "RK_HASH_SMALL_TABLE", "RK_HASH_KEY_SLACK", "RK_WG_PASSES",
         "RK_RETILE_MIN_READS", "RK_WINDOW_ALWAYS", "RK_NO_WINDOW", "RK_HASH_BIG_TABLE"]

# route: (developer knobs, lanes_per_read, what kernel_name() must say); the kernel's family: tests/planted.py, family()
ROUTES = {
    "lanes0": ({}, 0, "place_packed"),
    # kernel_name() names the packed kernel only.  That place_ascii_kernel placed the reads is shown by the reads themselves: the packer flags
    # every one AMBIGUOUS, the packed kernel leaves such reads unplaced (asserted below: without their characters n_rows stays 0), and the rows
    # equal the oracle's in the ambiguity mode asked for
    "ascii": ({}, 0, "place_packed"),
    "lanes8": ({}, 8, "place_packed_kernel<G=8,"),
    "lanes16": ({}, 16, "<G=16,"),
    "lanes32": ({}, 32, "place_packed_kernel<G=32,"),
    "lanes64": ({}, 64, "place_packed_kernel<G=64,"),
    "windowed": ({"RK_NO_WSTREAM": "1"}, 0, "place_packed16w_kernel<"),
    "sorted": ({"RK_NO_HASH": "1"}, 0, "place_packed16s_kernel<"),
    # (up to 4 500 DNA branches the image is built for place_packed16w_kernel; the knob builds it with the narrower windows of place_packed16s_kernel)
    "sorted_always": ({"RK_NO_HASH": "1", "RK_WSTREAM_ALWAYS": "1"}, 0, "place_packed16s_kernel<"),
    "hash": ({"RK_HASH_ALWAYS": "1"}, 0, ",LOGS=11> 2048 slots"),
    "hash_small": ({"RK_HASH_ALWAYS": "1", "RK_HASH_SMALL_TABLE": "1"}, 0, ",LOGS=10> 1024 slots"),
    # a table of 64 keys: most reads of the "many" trees bring more and are handed over to place_packed16w_kernel, some in the middle of a step
    "hash_slack": ({"RK_HASH_ALWAYS": "1", "RK_HASH_KEY_SLACK": "1984"}, 0, "2048 slots, <= 64 keys a read"),
    "wg1": ({}, 0, "place_wg_kernel<"),
    "wg2": ({"RK_WG_PASSES": "2"}, 0, "place_wg_kernel<"),
    "wg4": ({"RK_WG_PASSES": "4"}, 0, "place_wg_kernel<"),
}
KEEP_FACTORS = (0.0, 0.01)


@contextlib.contextmanager
def route_db(name, route, monkeypatch, sdb=None):
    """the database of planted tree `name` (or the database sdb: tests/test_gpu_weigh_planted.py), opened for the kernel of `route`; the
    route's developer knobs hold while it is open"""
    env, lanes, says = ROUTES[route]
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    for knob, v in env.items():
        monkeypatch.setenv(knob, v)
    db = ra.PhyloKmerDB.from_synth(P.tree(name)[0] if sdb is None else sdb, device=0)
    try:
        db.set_lanes_per_read(lanes)
        assert says in db.kernel_name(), (route, db.kernel_name())
        yield db
    finally:
        db.close()
        for knob in env:
            monkeypatch.delenv(knob, raising=False)


def run_route(name, route, Ks, monkeypatch, amb=None):
    """the reads of planted tree `name` through the kernel of `route`: {(K, keep_factor): Placements}, and the kernel's family"""
    sdb, odb, seq, off, _ = P.tree(name)
    if amb is not None:
        seq, _ = P.ambiguous(name, amb)
    n, L = len(off) - 1, int(off[1])
    with route_db(name, route, monkeypatch) as db:
        kn = db.kernel_name()
        fam = P.family(route, sdb.n_branches, sdb.bits)
        if fam.windows:  # the windows the census counts with are the image's
            got_w = tuple(int(x) for x in re.search(r"windows=(\d+) x (\d+)", kn).groups())
            assert got_w == ((sdb.n_branches - 1) // fam.W + 1, fam.W), (kn, fam.W)
        if isinstance(fam, P.Workgroup):
            got_g = tuple(int(x) for x in re.search(r"waves/WG=(\d+) .* passes=(\d+)", kn).groups())
            assert got_g == (fam.NW, fam.P), (kn, fam.NW, fam.P)
        pp = ra.PlacementProcess(db)
        packed, _, flags = pp.pack_reads_host(seq, off)
        if amb is not None:
            assert ((flags & _lib.RK_FLAG_AMBIGUOUS) != 0).all()  # every read is place_ascii_kernel's
            bare = P.place_prefilled(pp, packed, n, L, 7, amb=amb, flags=flags)  # no characters handed over: the packed kernel alone
            assert (bare.n_rows == 0).all() and ((bare.flags & _lib.RK_FLAG_AMBIGUOUS) != 0).all()
        res = {}
        for K in Ks:
            for kf in KEEP_FACTORS:
                res[K, kf] = P.place_prefilled(pp, packed, n, L, K, keep_factor=kf, amb=amb, flags=flags, seq=seq, off=off)
        return res, fam


def check_route(name, route, Ks, monkeypatch, amb=None):
    assert (name, route, tuple(Ks), amb) in P.CASES  # (tests/test_planted_shapes.py asserts the census of exactly these without a GPU)
    sdb, odb, seq, off, vectors = P.tree(name)
    if amb is not None:
        seq, vectors = P.ambiguous(name, amb)
    res, fam = run_route(name, route, Ks, monkeypatch, amb)
    what = f"{name} {route}" + (f" {amb}" if amb else "")
    for (K, kf), got in res.items():
        compare_with_oracle(got, P.oracle_place(name, K, kf, amb), odb, seq, off, amb_mode=GU.AMB[amb or "mean"])
        if amb is not None:
            assert ((got.flags & _lib.RK_FLAG_AMBIGUOUS) != 0).all()
        P.check_against_sorted_vectors(got, vectors, K, f"{what} keep_factor={kf}")
    print(what, P.assert_census(vectors, Ks, fam, sdb.n_branches, what))


def assert_same(a, b, what):
    assert np.array_equal(a.n_rows, b.n_rows) and np.array_equal(a.branch, b.branch) and np.array_equal(a.flags, b.flags), what
    assert np.array_equal(a.score.view(np.uint32), b.score.view(np.uint32)) and np.array_equal(a.lwr.view(np.uint64), b.lwr.view(np.uint64)), what


def check_agreement(name, routes, Ks, monkeypatch):
    """the kernels that can serve one tree, on the same reads: identical results (lanes8 serves keep_at_most <= 8)"""
    first = None
    for route in routes:
        res, _ = run_route(name, route, [K for K in Ks if K <= 8 or route != "lanes8"], monkeypatch)
        if first is None:
            first, first_route = res, route
            continue
        for key, got in res.items():
            assert_same(got, first[key], f"{name}: {route} against {first_route}, keep_at_most {key[0]} keep_factor {key[1]}")


# (the cases that set no developer knob run the product library, as tests/test_gpu_select_locate.py does; the others ask for dev_lib)
# ---- the dense kernels in 8-, 32- and 64-lane groups (heads_rounds of Heads4 through ds_bpermute / SGPRs, select_topk_scan and
#      rank_candidates outside 16-lane groups) ----
@pytest.mark.parametrize("nb", [30, 63, 64, 65, 399, 998])
def test_dense_8_lanes(nb, monkeypatch):
    check_route(f"dna{nb}", "lanes8", range(1, 9), monkeypatch)


@pytest.mark.parametrize("lanes", [32, 64])
@pytest.mark.parametrize("nb", [30, 63, 64, 65, 399, 998, 999, 1117])
def test_dense_32_and_64_lanes(nb, lanes, monkeypatch):
    check_route(f"dna{nb}", f"lanes{lanes}", P.K_ALL, monkeypatch)


def test_amino_acids_64_lanes(monkeypatch):
    check_route("aa399", "lanes64", P.K_ALL, monkeypatch)


# ---- place_ascii_kernel: the 64-lane select of reads that carry an ambiguity code ----
@pytest.mark.parametrize("amb", ["skip", "max", "mean"])
@pytest.mark.parametrize("name", ["dna64", "dna399", "dna999", "aa399"])
def test_ambiguity_kernel(name, amb, monkeypatch):
    check_route(name, "ascii", P.K_ALL, monkeypatch, amb=amb)


# ---- place_packed16w_kernel: the per-window scan, and the merge of the windows' winners in both forms (K <= 8: lane rotations; the LDS beyond) ----
@pytest.mark.parametrize("name", ["dna1277", "dna2801", "dna4500", "dna9001"])
def test_windowed_kernel(name, monkeypatch, dev_lib):
    check_route(name, "windowed", P.K_ALL, monkeypatch)


# ---- place_packed16s_kernel ----
@pytest.mark.parametrize("name", ["dna4501", "dna9001", "aa1999"])
def test_sorted_stream_kernel(name, monkeypatch, dev_lib):
    check_route(name, "sorted", P.K_ALL, monkeypatch)


# ---- place_hash64_kernel: both table sizes, and the tiles it hands over ----
@pytest.mark.parametrize("route", ["hash", "hash_small"])
@pytest.mark.parametrize("name", ["dna2801", "dna9001"])
def test_hash_kernel(name, route, monkeypatch, dev_lib):
    check_route(name, route, P.K_EDGES, monkeypatch)


@pytest.mark.parametrize("name", ["dna2801many", "dna9001many"])
def test_hash_kernel_hands_most_reads_over(name, monkeypatch, dev_lib):
    _, _, _, _, vectors = P.tree(name)
    assert sum(len(order) > 64 for order, _ in vectors) > len(vectors) // 2  # more branches than the table takes keys
    check_route(name, "hash_slack", P.K_EDGES, monkeypatch)


# ---- place_wg_kernel: level 1 (two candidates a lane, select_rounds64 beyond) and level 2 (the rounds; rank_candidates<64> with passes) ----
def test_workgroup_kernel_one_pass(monkeypatch, dev_lib):
    check_route("wg13301", "wg1", P.K_EDGES, monkeypatch)


@pytest.mark.parametrize("passes", [2, 4])
def test_workgroup_kernel_several_passes(passes, monkeypatch, dev_lib):
    check_route("wg13301", f"wg{passes}", (8, 16), monkeypatch)


# ---- every kernel that can serve a tree gives the same result ----
DENSE = ["lanes0", "lanes8", "lanes16", "lanes32", "lanes64"]  # (lanes0: the engine's own choice, 16 lanes on these trees)
WIDE = ["lanes16", "lanes32", "lanes64"]  # a forced lane width takes a windowed image through the dense kernels (8 lanes: keep_at_most <= 8 only, left to the small trees)


@pytest.mark.parametrize("name,routes,Ks", [
    *[(f"dna{nb}", DENSE, P.K_ALL) for nb in (30, 63, 64, 65, 399, 998, 999, 1117)],  # (1 117 branches: the largest tree the dense 16-lane geometry keeps)
    ("aa399", DENSE, P.K_ALL),
    ("dna1277", ["windowed", "sorted_always", "hash", "hash_small"] + WIDE, P.K_ALL),  # (the smallest tree in windows)
    ("dna2801", ["windowed", "sorted_always", "hash", "hash_small"] + WIDE, P.K_EDGES),
    ("dna2801many", ["hash_slack", "hash", "windowed", "sorted_always"] + WIDE, P.K_EDGES),
    ("dna4500", ["windowed", "sorted_always", "hash", "hash_small"] + WIDE, P.K_ALL),
    ("dna4501", ["sorted", "windowed", "hash", "hash_small"] + WIDE, P.K_ALL),
    ("dna9001", ["sorted", "windowed", "hash", "hash_small"] + WIDE, P.K_EDGES),
    ("dna9001many", ["hash_slack", "hash", "windowed", "sorted"] + WIDE, P.K_EDGES),
    ("aa1999", ["sorted", "windowed", "hash", "hash_small"] + WIDE, P.K_ALL),
    ("wg13301", ["wg1", "wg2", "wg4"], (8, 16)),  # (the large-tree image refuses a lane width: no dense kernel serves it)
], ids=lambda v: v if isinstance(v, str) else None)
def test_kernels_agree(name, routes, Ks, monkeypatch, dev_lib):
    check_agreement(name, routes, Ks, monkeypatch)
