"""GPU: rk_build_db on the code its seeded shapes (tests/test_gpu_build.py) never reach -- a lane's second explorer, chunk
turnover and the resize-and-rerun loop, k above 12 / 5, every compiled explore_kernel variant, every number of ranked states,
alignments of k - 1 and k sites, gap jumps that leave the alignment.  Every case equals oracle.build_db bit for bit (DESIGN.md
section 8b); nothing here has a tolerance."""
import functools
import os
import re

import numpy as np
import pytest

import rappas_amd as ra
from oracle import oracle as O
from rappas_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "rappas_amd", "csrc", "rk_build.hip")).read()


def _const(pattern):
    m = re.search(pattern, _SRC)
    assert m, f"rk_build.hip no longer holds {pattern!r}: restate first_capacity() from the launcher"
    return int(m.group(1))


# the launcher's own constants, read from its source: the cases below are built to pass them
TUPLE_CHUNK = _const(r"constexpr int TUPLE_CHUNK = (\d+);")
WAVES_PER_BLOCK = _const(r"constexpr int BUILD_WAVES_PER_BLOCK = (\d+);")
GENEROUS = _const(r"const u64 generous = (\d+);")
CAPACITY_FLOOR = 1 << _const(r"std::max<u64>\(capacity, 1u << (\d+)\)")
LANES_PER_BLOCK = 64 * WAVES_PER_BLOCK


def first_capacity(n_tasks, blocks):
    """Slots of the tuple buffer of a batch's first attempt while nothing has been measured (build_db_impl)."""
    return max(n_tasks * GENEROUS, CAPACITY_FLOOR) + blocks * WAVES_PER_BLOCK * TUPLE_CHUNK


def _as_ref(got):
    return dict(key_codes=got.key_codes, row_offsets=got.row_offsets, branch_ids=got.branch_ids, scores=got.scores,
                tuples=got.tuples, visits=got.visits)


def _same(got, ref):
    """What test_gpu_build._check compares, against a result already computed."""
    assert got.tuples == ref["tuples"] and got.visits == ref["visits"], (got.tuples, ref["tuples"], got.visits, ref["visits"])
    assert np.array_equal(got.key_codes, ref["key_codes"])
    assert np.array_equal(got.row_offsets, ref["row_offsets"])
    assert np.array_equal(got.branch_ids, ref["branch_ids"])
    assert np.array_equal(got.scores.view(np.uint32), ref["scores"].view(np.uint32))  # the running-float scores, bit for bit


def _check(alphabet, k, states, pp, nb, T, **kw):
    ref = O.build_db(alphabet, k, states, pp, nb, T, **kw)
    got = ra.build_db(alphabet, k, states, pp, nb, T, **kw)
    _same(got, ref)
    return got, ref


def _cut(states, pp, n_states):
    """The table cut to its n_states best states per site (a legal PProbasSorted: ranks stay descending)."""
    return np.ascontiguousarray(states[:, :, :n_states]), np.ascontiguousarray(pp[:, :, :n_states])


def _gap_rows(n_sites, seed, n_rows=6, n_runs=4, max_len=5):
    """Gap intervals of random alignment rows, as test_build_with_gap_jumps draws them."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n_rows):
        r = ["A"] * n_sites
        for _ in range(n_runs):
            s = int(rng.integers(1, max(2, n_sites - max_len - 2)))
            for t in range(s, min(n_sites - 1, s + int(rng.integers(1, max_len + 1)))):
                r[t] = "-"
        rows.append("".join(r))
    off, lens = synth.gap_intervals(rows)
    assert lens.size > 0
    return off, lens


def _gaps_at(n_sites, lists):
    """CSR gap intervals written by hand: {site: [lengths]}."""
    off = np.zeros(n_sites + 1, np.uint32)
    for s, v in lists.items():
        off[s + 1] = len(v)
    off = np.cumsum(off, dtype=np.uint32)
    lens = np.array([x for s in sorted(lists) for x in lists[s]], np.int32)
    return off, lens


# ---------------------------------------------------------------------------------------------------------------
# shared inputs: built once, their oracle result computed once and left unchanged
# ---------------------------------------------------------------------------------------------------------------
def _tables(alphabet, k, n_nodes, n_sites, seed, omega=1.5, n_states=None, gaps=None, limit1=True, T=None):
    states, pp, nb = synth.make_pp_tables(alphabet, n_nodes, n_sites, seed=seed)
    if n_states is not None:
        states, pp = _cut(states, pp, n_states)
    if T is None:
        _, T = synth.thresholds(omega, alphabet, k)
    kw = {}
    if gaps is not None:
        off, lens = _gap_rows(n_sites, gaps)
        kw = dict(gap_off=off, gap_len=lens, limit_to_1_jump=limit1)
    return (alphabet, k, states, pp, nb, np.float32(T)), kw


EVERYTHING = np.float32(-1e30)  # a threshold every word passes

CASES = {
    # 1. explorer reuse: many more explorers than one block has lanes
    "dna6": lambda: _tables(4, 6, 8, 300, 1),
    "dna6_all_jumps": lambda: _tables(4, 6, 8, 300, 1, gaps=31, limit1=False),
    "dna6_one_jump": lambda: _tables(4, 6, 8, 300, 1, gaps=31, limit1=True),
    "aa3": lambda: _tables(20, 3, 6, 200, 2),
    "dna5_3states": lambda: _tables(4, 5, 8, 300, 3, n_states=3),
    # 2. chunk turnover and buffer growth: everything registers
    "dna8_all_words": lambda: _tables(4, 8, 1, 107, 4, T=EVERYTHING),
    "dna9_all_words": lambda: _tables(4, 9, 1, 40, 5, T=EVERYTHING),
    "aa4_all_words": lambda: _tables(20, 4, 1, 40, 6, T=EVERYTHING),
    "dna8_all_words_2nodes": lambda: _tables(4, 8, 2, 107, 7, T=EVERYTHING),
    # 4. every compiled variant: shapes of test_gpu_build.test_build_matches_oracle / test_build_with_gap_jumps
    "variants_dna": lambda: _tables(4, 8, 40, 300, 2),
    "variants_aa": lambda: _tables(20, 5, 12, 80, 5),
    "variants_all_jumps": lambda: _tables(4, 6, 12, 90, 12, gaps=11, limit1=False),
    "variants_one_jump": lambda: _tables(4, 6, 12, 90, 12, gaps=11, limit1=True),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    args, kw = CASES[name]()
    ref = O.build_db(*args, **kw)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return args, kw, ref


def _n_tasks(args):
    k, states = args[1], args[2]
    return states.shape[0] * max(0, states.shape[1] - k + 2)


# ---------------------------------------------------------------------------------------------------------------
# 1. a lane's second explorer
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dna6", "dna6_all_jumps", "dna6_one_jump", "aa3", "dna5_3states"])
def test_one_block_runs_many_explorers_per_lane(name, monkeypatch, dev_lib):
    """RK_BUILD_BLOCKS=1: 256 lanes fetch 1 194 .. 2 368 explorers, so every lane goes through the `d == -2` reset several times
    with the previous explorer's frames and cursor behind it, next to lanes that are in the middle of theirs; in one-jump mode
    the previous explorer's firstJump must not reach the next.  Equal to the oracle and to the default grid."""
    args, kw, ref = _case(name)
    assert _n_tasks(args) > 4 * LANES_PER_BLOCK
    if kw:
        plain = O.build_db(*args)
        assert ref["visits"] > plain["visits"]  # the intervals are met
    wide = ra.build_db(*args, **kw)
    monkeypatch.setenv("RK_BUILD_BLOCKS", "1")
    one = ra.build_db(*args, **kw)
    _same(one, ref)
    _same(wide, ref)
    _same(one, _as_ref(wide))
    assert len(one.scores) > 0


def test_one_block_and_node_batches(monkeypatch, dev_lib):
    """The same with the input cut into batches of three nodes: lanes are reused inside every batch's launch."""
    args, kw, ref = _case("dna6")
    monkeypatch.setenv("RK_BUILD_BLOCKS", "1")
    monkeypatch.setenv("RK_BUILD_BATCH_NODES", "3")
    _same(ra.build_db(*args, **kw), ref)


# ---------------------------------------------------------------------------------------------------------------
# 2. chunk turnover, the resize-and-rerun loop
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tuples,entries", [
    ("dna8_all_words", 100 * 4 ** 8, 4 ** 8), ("dna9_all_words", 32 * 4 ** 9, 4 ** 9), ("aa4_all_words", 37 * 20 ** 4, None),
])
def test_tuple_buffer_overflows_and_the_kernel_runs_again(name, tuples, entries, monkeypatch, dev_lib):
    """Every word of every full-length explorer registers, through one block: each wave closes thousands of 1 024-slot chunks
    (the pad-the-remainder branch of append_tuples), the first buffer -- max(tasks * 4096, 2^20) + 4 * 1024 slots -- overflows,
    and the launcher sizes the buffer from the slot counter and runs the kernel again; the sort then takes millions of slots
    with pads among them.  (aa4: the unrolled 20-state leaf append.)"""
    args, kw, ref = _case(name)
    assert ref["tuples"] == tuples and (entries is None or len(ref["scores"]) == entries)
    monkeypatch.setenv("RK_BUILD_BLOCKS", "1")
    got = ra.build_db(*args, **kw)
    assert got.tuples > first_capacity(_n_tasks(args), blocks=1)  # more registrations than the first buffer has slots
    _same(got, ref)


def test_grown_batch_is_sorted_with_the_running_set(monkeypatch, dev_lib):
    """Two nodes on one branch, one node a batch: the first batch overflows its buffer and is rerun; the second one's millions
    of slots are sorted together with the 65 536 entries the first left, and every key takes the larger of two scores."""
    args, kw, ref = _case("dna8_all_words_2nodes")
    assert args[4].tolist() == [0, 0] and len(ref["scores"]) == 4 ** 8 and ref["tuples"] == 2 * 100 * 4 ** 8
    monkeypatch.setenv("RK_BUILD_BLOCKS", "1")
    monkeypatch.setenv("RK_BUILD_BATCH_NODES", "1")
    got = ra.build_db(*args, **kw)
    assert got.tuples // 2 > first_capacity(_n_tasks(args) // 2, blocks=1)
    _same(got, ref)


# ---------------------------------------------------------------------------------------------------------------
# 3. the k range of the ABI
# ---------------------------------------------------------------------------------------------------------------
K_RANGE = [  # alphabet, k, ranked states kept, nodes, sites
    (4, 13, 3, 1, 19), (4, 14, 2, 5, 24), (4, 15, 2, 5, 25), (20, 6, 3, 5, 16), (20, 7, 3, 5, 17), (20, 8, 2, 5, 18), (20, 9, 2, 5, 19),
]
K_RANGE_ALL_JUMPS = [(4, 14, 2, 1, 24)] + K_RANGE[3:]  # every jump at every level multiplies the visits: one DNA node


@pytest.mark.parametrize("alphabet,k,n_states,n_nodes,n_sites,gaps",
                         [c + (None,) for c in K_RANGE] + [c + ("one",) for c in K_RANGE] + [c + ("all",) for c in K_RANGE_ALL_JUMPS])
def test_largest_k_of_both_alphabets(alphabet, k, n_states, n_nodes, n_sites, gaps):
    """DNA k = 13 .. 15 and amino acids k = 6 .. 9: frames down to depth 13, codes of up to 45 bits (the sort's end bit 61).
    The reference's bound prunes at the last level only (DNA k = 13 on 4 nodes x 60 full-width sites: 7.6e9 visits), so the
    tables are cut to 2 or 3 ranked states, about n_states^k visits an explorer, on k + 10 sites (k + 6 for DNA k = 13 with
    three states: 1.3e6 visits an explorer).  Gap intervals are drawn as in test_build_with_gap_jumps.
    Oracle visits, plain / one jump / all jumps:
      DNA k=13, 3 states, 1 node   9.77e6 / 9.78e6 / -
      DNA k=14, 2 states, 5 nodes  1.47e6 / 1.47e6 / 5.64e6 (1 node)
      DNA k=15, 2 states, 5 nodes  2.92e6 / 2.93e6 / -
      AA  k=6,  3 states, 5 nodes  4.40e4 / 4.62e4 / 1.58e5
      AA  k=7,  3 states, 5 nodes  1.30e5 / 1.37e5 / 6.05e5
      AA  k=8,  2 states, 5 nodes  2.71e4 / 2.89e4 / 1.11e5
      AA  k=9,  2 states, 5 nodes  5.55e4 / 5.70e4 / 2.60e5"""
    bits = 2 if alphabet == 4 else 5
    args, kw = _tables(alphabet, k, n_nodes, n_sites, seed=40 + k, n_states=n_states, gaps=70 + k if gaps else None,
                       limit1=gaps != "all")
    got, ref = _check(*args, **kw)
    assert ref["visits"] < 1.2e7  # "about 10^7": the oracle replays this in well under a second
    assert len(got.key_codes) > 0
    assert int(got.key_codes.max()).bit_length() > bits * (k - 1)  # a registered word whose last letter is not state 0
    if gaps:
        assert ref["visits"] > O.build_db(*args)["visits"]  # the intervals are met


def test_k_beyond_the_range_is_refused():
    states, pp, nb = synth.make_pp_tables(20, 2, 14, seed=1)
    with pytest.raises(ra.RkError, match=r"k=10 outside supported range 2\.\.9"):
        ra.build_db(20, 10, states, pp, nb, np.float32(-10.0))
    states, pp, nb = synth.make_pp_tables(4, 2, 20, seed=1)
    with pytest.raises(ra.RkError, match=r"k=16 outside supported range 2\.\.15"):
        ra.build_db(4, 16, states, pp, nb, np.float32(-10.0))


# ---------------------------------------------------------------------------------------------------------------
# 4. every compiled variant of explore_kernel
# ---------------------------------------------------------------------------------------------------------------
VARIANTS = [{"RK_BUILD_INLINE_LEVELS": "1"}, {"RK_BUILD_INLINE_LEVELS": "2"}, {"RK_BUILD_NO_VEC": "1"},
            {"RK_BUILD_INLINE_LEVELS": "1", "RK_BUILD_NO_VEC": "1"}]


@pytest.mark.parametrize("knobs", VARIANTS, ids=lambda d: "+".join(f"{k[9:]}={v}" for k, v in d.items()))
@pytest.mark.parametrize("name", ["variants_dna", "variants_aa", "variants_all_jumps", "variants_one_jump"])
def test_every_compiled_variant(name, knobs, monkeypatch, dev_lib):
    """One and two levels in registers instead of three, and the generic tails instead of the register-resident site rows:
    kernels that are compiled into the library and that no default launch selects."""
    dev = open(ra.build.DEV_SO, "rb").read()
    args, kw, ref = _case(name)
    for knob, v in knobs.items():
        assert knob.encode() in dev
        monkeypatch.setenv(knob, v)
    _same(ra.build_db(*args, **kw), ref)
    assert len(ref["scores"]) > 0


# ---------------------------------------------------------------------------------------------------------------
# 5. the number of ranked states
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet,n_states", [(4, n) for n in range(1, 5)] + [(20, n) for n in range(1, 21)])
def test_every_number_of_ranked_states(alphabet, n_states):
    """k = 3 on 3 nodes x 12 sites with the table cut to its n_states best states.  Amino acids with four states is the case
    the launcher used to hand to the 2-bit register tail of the DNA kernel."""
    args, kw = _tables(alphabet, 3, 3, 12, seed=50 + n_states, omega=1.0, n_states=n_states)
    got, _ = _check(*args, **kw)
    assert len(got.key_codes) > 0


@pytest.mark.parametrize("k,gaps", [(2, False), (5, False), (5, True), (3, True)])
def test_four_ranked_states_of_twenty(k, gaps):
    """Amino acids cut to four states where only tails run (k = 2, 3) and where frames sit above them (k = 5), with and
    without gap jumps: 5-bit letters at every level."""
    args, kw = _tables(20, k, 3, 14, seed=60 + k, omega=1.0, n_states=4, gaps=80 + k if gaps else None)
    got, _ = _check(*args, **kw)
    assert len(got.key_codes) > 0 and int(got.key_codes.max()).bit_length() > 5 * (k - 1)
    assert int((np.asarray(args[2]) > 3).sum()) > 0  # states that do not fit two bits


def test_four_ranked_states_of_twenty_generic_kernel(monkeypatch, dev_lib):
    """The same table through RK_BUILD_NO_VEC: the generic kernel, whatever the launcher would have chosen."""
    args, kw = _tables(20, 3, 3, 12, seed=54, omega=1.0, n_states=4)
    monkeypatch.setenv("RK_BUILD_NO_VEC", "1")
    got, _ = _check(*args, **kw)
    assert len(got.key_codes) > 0


# ---------------------------------------------------------------------------------------------------------------
# 6. edges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet,k", [(4, 6), (4, 3), (20, 3)])
def test_alignment_of_k_minus_one_and_k_sites(alphabet, k):
    _, T = synth.thresholds(1.0, alphabet, k)
    states, pp, nb = synth.make_pp_tables(alphabet, 3, k - 1, seed=3)
    got, _ = _check(alphabet, k, states, pp, nb, T)  # one explorer a node; it runs off the end and registers nothing
    assert got.visits > 0 and got.tuples == 0 and len(got.key_codes) == 0 and got.row_offsets.tolist() == [0]
    states, pp, nb = synth.make_pp_tables(alphabet, 3, k, seed=4)
    got, _ = _check(alphabet, k, states, pp, nb, T)  # two explorers a node, the first one complete
    assert got.tuples > 0


@pytest.mark.parametrize("limit1", [True, False])
@pytest.mark.parametrize("k", [3, 6])
def test_gap_jumps_at_and_beyond_the_end(k, limit1):
    """Intervals at the last two sites (the jump from the last site lands on site n_sites: nothing there), an interval as long
    as the alignment (the largest the ABI admits) beside one that stays inside, and one that lands exactly on the last site."""
    S = 14
    states, pp, nb = synth.make_pp_tables(4, 3, S, seed=8)
    _, T = synth.thresholds(1.0, 4, k)
    off, lens = _gaps_at(S, {2: [S, 3], 5: [S - 6, S - 5], S - 2: [1, 2], S - 1: [1, S]})
    got, ref = _check(4, k, states, pp, nb, T, gap_off=off, gap_len=lens, limit_to_1_jump=limit1)
    # the intervals are met (a jump can also end a sibling loop early, so the visits may fall as well as rise)
    assert ref["visits"] != O.build_db(4, k, states, pp, nb, T)["visits"] and got.tuples > 0


def test_largest_branch_id():
    states, pp, nb = synth.make_pp_tables(4, 4, 20, seed=9)
    nb = np.array([65534, 0, 65534, 65533], np.uint16)
    got, _ = _check(4, 5, states, pp, nb, EVERYTHING)  # every 5-mer, the all-ones code included, beside the pad key
    assert int(got.branch_ids.max()) == 65534 and int(got.key_codes.max()) == 4 ** 5 - 1
    with pytest.raises(ra.RkError, match="65535 is reserved"):
        ra.build_db(4, 5, states, pp, np.array([0, 1, 2, 65535], np.uint16), EVERYTHING)


def test_two_nodes_with_one_table_on_one_branch():
    states, pp, _ = synth.make_pp_tables(4, 1, 40, seed=10)
    _, T = synth.thresholds(1.5, 4, 6)
    one, _ = _check(4, 6, states, pp, np.array([7], np.uint16), T)
    two, _ = _check(4, 6, np.concatenate([states, states]), np.concatenate([pp, pp]), np.array([7, 7], np.uint16), T)
    assert two.tuples == 2 * one.tuples > 0  # every key twice, with equal scores
    _same(two, dict(_as_ref(one), tuples=two.tuples, visits=2 * one.visits))
