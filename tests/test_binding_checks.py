"""The checks the Python binding makes itself in the host forms (rappas_amd/placement.py), one by one: the exception type and a
fragment of its text; and the places where it deliberately lets the C side speak (an RkError and its code).  Every case starts from
the valid call of test_samples_args.py -- the five-node tree, a buffer of three samples, a result set of four reads -- and breaks one
thing.  Also what the valid calls hand back: the shapes and dtypes of the arrays the binding allocates.  No GPU."""
import types

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import placement as P
from rappas_amd._lib import RK_ERR_INVALID

from tests.test_samples_args import B, K, N_READS, S, W, values

V = values()
PARENT, BL, MASSES = V["parent"], V["bl"], V["masses"]
SHORT_BL = BL[:4]


def rows(n=N_READS, k=K, flat=False):
    """a result set of n reads of k rows as the sums read it: anything with n_rows, branch and lwr"""
    shape = (n * k,) if flat else (n, k)
    return types.SimpleNamespace(n_rows=np.full(n, k, np.uint8), branch=np.tile(np.array([1, 3], np.uint16), n * k // 2).reshape(shape),
                                 lwr=np.full(shape, 0.5))


def refused(text, fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert text in str(e.value), str(e.value)


def rk_invalid(text, fn, *args, **kw):
    with pytest.raises(ra.RkError) as e:
        fn(*args, **kw)
    assert e.value.code == RK_ERR_INVALID and text in str(e.value), str(e.value)


# ---- the tree and the sample buffer of the sample-level calls ----
SAMPLE_CALLS = {
    "kr_distances_host": lambda p, bl, m, s: ra.kr_distances_host(p, bl, m, s),
    "squash_host": lambda p, bl, m, s: ra.squash_host(p, bl, m, s),
    "kmeans_host": lambda p, bl, m, s: ra.kmeans_host(p, bl, m, s, 2),
    "diversity_host": lambda p, bl, m, s: ra.diversity_host(p, bl, m, s),
    "epca_host": lambda p, bl, m, s: ra.epca_host(p, bl, m, s, 2, 5),
}


@pytest.mark.parametrize("call", sorted(SAMPLE_CALLS))
def test_branch_len_of_another_length(call):
    refused("branch_len holds 4 lengths, parent 5 nodes", SAMPLE_CALLS[call], PARENT, SHORT_BL, MASSES, S)


def test_branch_len_of_another_length_in_the_tree_calls():
    text = "branch_len holds 4 lengths, parent 5 nodes"
    refused(text, P.tree_validate, PARENT, SHORT_BL)
    refused(text, ra.edpl_host, PARENT, SHORT_BL, K, V["res"]["n_rows"], V["res"]["branch"], V["res"]["lwr"])
    refused(text, ra.tree_distance_host, PARENT, SHORT_BL, V["a"], V["b"])


@pytest.mark.parametrize("call", sorted(SAMPLE_CALLS) + ["clade_masses_host"])
def test_mass_buffer_word_count(call):
    fn = SAMPLE_CALLS.get(call) or (lambda p, bl, m, s: ra.clade_masses_host(p, m, s))
    with_word, without = fn(PARENT, BL, MASSES, S), fn(PARENT, BL, MASSES[:S * W], S)  # the skipped-entries word is optional
    flat = lambda r: [np.asarray(x).tobytes() for x in (r if isinstance(r, tuple) else (r,)) if x is not None and not isinstance(x, (int, tuple))]
    assert flat(with_word) == flat(without)
    refused(f"masses holds {S * W - 1} words, {S} samples on {B} branches have {S * W} (+ 1)", fn, PARENT, BL, MASSES[:S * W - 1], S)
    refused(f"masses holds {S * W + 2} words", fn, PARENT, BL, np.zeros(S * W + 2, np.uint64), S)


def test_seeds_not_of_k_entries():
    refused("seeds must hold k = 2 sample indices", ra.kmeans_host, PARENT, BL, MASSES, S, 2, seeds=[0, 1, 2])
    refused("seeds must hold k = 2 sample indices", ra.kmeans_host, PARENT, BL, MASSES, S, 2, seeds=[0])
    got = ra.kmeans_host(PARENT, BL, MASSES, S, 2, seeds=[2, 0])
    assert got.assign.tolist() in ([1, 1, 0], [1, 0, 0]) and int(got.info[0]) == 2


def test_the_c_side_speaks_for_the_ranges():
    """k = 0, S = 1 and an edge PCA out of range reach the C side (the binding sizes its arrays with max(.., 0) and max(.., 1) for that)"""
    rk_invalid("rk_kmeans_host: k=0 clusters must be in 1..64", ra.kmeans_host, PARENT, BL, MASSES, S, 0)
    rk_invalid("rk_kmeans_host: k=0 clusters", ra.kmeans_host, PARENT, BL, MASSES, S, 0, centroids=False)
    rk_invalid("rk_squash_host: n_samples=1 must be in 2..4096", ra.squash_host, PARENT, BL, MASSES[:W], 1)
    rk_invalid("rk_epca_host: k=9 components must be in 1..8", ra.epca_host, PARENT, BL, MASSES, S, 9, 5)
    rk_invalid("rk_epca_host: k=0 components must be in 1..8", ra.epca_host, PARENT, BL, MASSES, S, 0, 5)
    rk_invalid("rk_epca_host: n_samples=1 must be in 2..4096", ra.epca_host, PARENT, BL, MASSES[:W], 1, 2, 5)
    rk_invalid("rk_kr_distances_host: n_samples=0 must be in 1..65535", ra.kr_distances_host, PARENT, BL, MASSES[:0], 0)
    rk_invalid("rk_tree_validate: nodes 0 and 1 both have parent -1", P.tree_validate, np.array([-1, -1, 0, 2, 2], np.int32), BL)
    rk_invalid("theta", ra.diversity_host, PARENT, BL, MASSES, S, theta=[9.0])


def test_diversity_math_shapes():
    refused("x and y must hold one value each per element", ra.diversity_math_host, 2, [1.0, 2.0], [1.0])
    assert ra.diversity_math_host(0, [1.0, 8.0]).tolist() == [0.0, 3.0]
    got = ra.diversity_math_host(2, [[2.0, 3.0]], [2.0, 2.0])  # the shapes are compared after flattening
    assert got.shape == (2,) and got.tolist() == ra.diversity_math_host(2, [2.0, 3.0], [[2.0], [2.0]]).tolist()


def test_tree_distance_pairs():
    refused("a and b must hold one branch each per pair", ra.tree_distance_host, PARENT, BL, [1, 4], [3])
    d = ra.tree_distance_host(PARENT, BL, V["a"], V["b"])
    assert d.dtype == np.float64 and d.shape == (2,)


# ---- the rows of a result set ----
def test_branch_and_lwr_not_n_by_k():
    text = "branch and lwr must hold n_reads x K rows"
    short = rows()
    short.lwr = short.lwr[:, :1]
    refused(text, ra.accumulate_masses_host, B, short)
    refused(text, ra.accumulate_masses_samples_host, B, short, S, np.zeros(N_READS, np.uint32))
    ragged = rows(flat=True)
    ragged.branch = ragged.branch[:-1]  # flat, and no multiple of n
    refused(text, ra.accumulate_masses_host, B, ragged)
    refused(text, ra.accumulate_masses_samples_host, B, ragged, S, np.zeros(N_READS, np.uint32))
    r = V["res"]
    refused(f"branch and lwr must hold n_reads x K = {N_READS} x {K} rows", ra.edpl_host, PARENT, BL, K, r["n_rows"], r["branch"][:-1], r["lwr"])
    refused(f"branch and lwr must hold n_reads x K = {N_READS} x 3 rows", ra.edpl_host, PARENT, BL, 3, r["n_rows"], r["branch"], r["lwr"])


def test_flat_rows_are_read_as_n_by_k():
    want = ra.accumulate_masses_host(B, rows())
    assert np.array_equal(ra.accumulate_masses_host(B, rows(flat=True)), want) and want.dtype == np.uint64 and want.shape == (W,)
    sample = np.array([0, 1, 2, 0], np.uint32)
    want = ra.accumulate_masses_samples_host(B, rows(), S, sample)
    assert np.array_equal(ra.accumulate_masses_samples_host(B, rows(flat=True), S, sample), want) and want.shape == (S * W + 1,)
    none = types.SimpleNamespace(n_rows=np.zeros(0, np.uint8), branch=np.zeros(0, np.uint16), lwr=np.zeros(0))  # no reads, flat: K = 1
    assert not ra.accumulate_masses_host(B, none).any()
    assert np.array_equal(ra.edpl_host(PARENT, BL, K, V["res"]["n_rows"], V["res"]["branch"].reshape(N_READS, K), V["res"]["lwr"]),
                          ra.edpl_host(PARENT, BL, K, V["res"]["n_rows"], V["res"]["branch"], V["res"]["lwr"].reshape(N_READS, K)))


def test_weights_not_one_per_read():
    refused("weights must hold one uint32 per read", ra.accumulate_masses_host, B, rows(), weights=[1, 2, 3])
    refused("weights must hold one uint32 per read", ra.accumulate_masses_host, B, rows(), weights=np.ones((N_READS, 1), np.uint32))
    one, two = ra.accumulate_masses_host(B, rows()), ra.accumulate_masses_host(B, rows(), weights=[2] * N_READS)
    assert np.array_equal(two[:B], 2 * one[:B])


@pytest.mark.parametrize("samples", [False, True])
def test_masses_of_a_wrong_dtype_shape_or_contiguity(samples):
    words = S * W + 1 if samples else W
    call = (lambda m: ra.accumulate_masses_samples_host(B, rows(), S, np.zeros(N_READS, np.uint32), masses=m)) if samples else \
        (lambda m: ra.accumulate_masses_host(B, rows(), masses=m))
    text = f"masses must be a contiguous uint64 array of {words} words"
    refused(text, call, np.zeros(words, np.int64))
    refused(text, call, np.zeros(words + 1, np.uint64))
    refused(text, call, np.zeros((1, words), np.uint64))
    refused(text, call, np.zeros(2 * words, np.uint64)[::2])
    mine = np.zeros(words, np.uint64)
    assert call(mine) is mine and mine.any()  # added into the caller's buffer


def test_member_lists():
    sample = np.zeros(N_READS, np.uint32)
    refused(f"member_read must hold {N_READS} uint32 words", ra.accumulate_masses_samples_host, B, rows(), S, sample, member_read=[0, 1])
    refused(f"member_weight must hold {N_READS} uint32 words", ra.accumulate_masses_samples_host, B, rows(), S, sample, member_weight=[1] * 5)
    got = ra.accumulate_masses_samples_host(B, rows(), S, sample, member_read=[0, 1, 2, 3], member_weight=[1] * N_READS)
    assert np.array_equal(got, ra.accumulate_masses_samples_host(B, rows(), S, sample))


@pytest.mark.parametrize("n_branches", [0, 65536])
def test_n_branches_out_of_range(n_branches):
    assert ra.masses_words(n_branches) == 0 and ra.masses_samples_words(n_branches, S) == 0
    refused(f"n_branches={n_branches} must be in 1..65535", ra.accumulate_masses_host, n_branches, rows())
    refused(f"n_samples={S} on {n_branches} branches: both in 1..65535 and at most 2^29 words", ra.accumulate_masses_samples_host, n_branches, rows(), S,
            np.zeros(N_READS, np.uint32))


def test_n_samples_out_of_range_is_refused_before_the_rows():
    bad = rows()
    bad.lwr = bad.lwr[:, :1]
    refused(f"n_samples=0 on {B} branches", ra.accumulate_masses_samples_host, B, bad, 0, np.zeros(N_READS, np.uint32))
    refused(f"n_samples=65536 on {B} branches", ra.accumulate_masses_samples_host, B, bad, 65536, np.zeros(N_READS, np.uint32))


# ---- edge PCA ----
def test_epca_finish_raw_length():
    raw, info = ra.epca_host(PARENT, BL, MASSES, S, 2, 5)
    n = 1 + 2 * (3 + S + B)
    assert raw.shape == (n,) and raw.dtype == np.float64 and info.shape == (2,) and info.dtype == np.uint32
    refused(f"raw holds {n - 1} doubles, an edge PCA of 2 components of {S} samples on {B} branches has {n}", ra.epca_finish, B, S, 2, raw[:-1], info)
    rk_invalid(f"edge PCA: n_branches={B}, n_samples={S}, k=9: out of 1..65535, 2..4096, 1..8", ra.epca_finish, B, S, 9, raw, info)
    rk_invalid(f"edge PCA: n_branches={B}, n_samples=1, k=2", ra.epca_finish, B, 1, 2, raw[:-1])  # the range before the length
    e = ra.epca_finish(B, S, 2, raw, info)
    assert (e.n_active, e.k_eff) == (int(info[0]), int(info[1])) and e.projection.shape == (S, 2) and e.loading.shape == (B, 2)
    assert [x.shape for x in (e.eigenvalue, e.share, e.residual)] == [(2,)] * 3
    e = ra.epca_finish(B, S, 2, raw.reshape(1, -1))
    assert (e.n_active, e.k_eff) == (None, None)


# ---- a database's arrays ----
def test_database_arrays_that_do_not_fit_each_other():
    """refused by the binding before a handle is asked for: no GPU is touched"""
    keys, offs, br, sc = [1, 2], [0, 1, 2], [0, 1], [-1.0, -2.0]
    db = lambda *csr: ra.PhyloKmerDB(ra.RK_ALPHABET_DNA, 6, B, -1.5, 0.03, *csr)
    refused("row_offsets must have n_keys+1 entries", db, keys, offs[:2], br, sc)
    refused("row_offsets[-1] must equal len(branch_ids)", db, keys, [0, 1, 3], br, sc)
    refused("branch_ids and scores differ in length", db, keys, offs, br, sc[:1])


# ---- strands ----
def test_strand_words():
    refused("strand must be 'forward', 'reverse' or 'both', not 'sideways'", P._strand, "sideways")
    assert [P._strand(s) for s in ("forward", "fwd", "reverse", "rev", "both", 2, np.uint32(1))] == [0, 0, 1, 1, 2, 2, 1]


# ---- what the valid calls hand back ----
def test_outputs_of_the_sample_calls():
    d = ra.kr_distances_host(PARENT, BL, MASSES, S, threads=1)
    assert d.shape == (S, S) and d.dtype == np.float64
    c = ra.clade_masses_host(PARENT, MASSES, S)
    assert c.shape == (S, B) and c.dtype == np.uint64
    merges, n = ra.squash_host(PARENT, BL, MASSES, S)
    assert merges.dtype == ra.SQUASH_MERGE and merges.shape == (S - 1,) and type(n) is int and n == S - 1
    km = ra.kmeans_host(PARENT, BL, MASSES, S, 2, max_rounds=10)
    assert isinstance(km, ra.KMeans)
    assert [(x.shape, x.dtype) for x in km] == [((S,), np.uint32), ((S,), np.float64), ((2,), np.uint32), ((2,), np.float64), ((4,), np.uint32),
                                                ((2, 2, B), np.float64)]
    assert ra.kmeans_host(PARENT, BL, MASSES, S, 2, centroids=False).centroids is None
    dv = ra.diversity_host(PARENT, BL, MASSES, S, theta=[0.5, 1])
    assert isinstance(dv, ra.Diversity) and dv.values.shape == (S, 9) and dv.values.dtype == np.float64
    assert dv.columns == ("rooted_pd", "pd", "bwpd", "quadratic", "phylo_entropy", "rooted_pd_0.5", "bwpd_0.5", "rooted_pd_1", "bwpd_1")
    assert ra.diversity_host(PARENT, BL, MASSES, S, theta=None).values.shape == (S, 5) and ra.diversity_columns(None) == dv.columns[:5]
    e = ra.edpl_host(PARENT, BL, K, **V["res"])
    assert e.shape == (N_READS,) and e.dtype == np.float64


def test_outputs_of_the_packers():
    seq = np.frombuffer(b"ACGTACGTACGTAAC", np.uint8)
    off = np.array([0, 9, 15], np.uint64)
    packed, lens, flags = ra.pack_reads(ra.RK_ALPHABET_DNA, 4, seq, off)
    assert packed.shape == (2, 1) and [a.dtype for a in (packed, lens, flags)] == [np.uint32] * 3 and lens.tolist() == [9, 6]
    assert ra.pack_reads(ra.RK_ALPHABET_DNA, 4, seq, off, words_per_read=3)[0].shape == (2, 3)
    assert ra.pack_reads(ra.RK_ALPHABET_AA, 4, seq, off)[0].shape == (2, 2)  # 5 bits a residue
    assert ra.pack_reads(ra.RK_ALPHABET_DNA, 4, seq[:0], off[:1])[0].shape == (0, 1)
    aa, aa_lens = ra.translate_packed_host(packed, 0, lens=lens)
    assert aa.shape == (2, ra.translated_words(16)) and aa_lens.shape == (2,) and aa_lens.dtype == np.uint32
    assert ra.translate_packed_host(packed, 0, fixed_len=6, aa_words=2)[0].shape == (2, 2)
