"""The checks of the Python binding (rappas_amd/placement.py) that need a handle, and the parts of it no other test names: the tensor
checks of every device form, the seeds of kmeans_batch, a side stream for the calls that read host arrays during the call, the whole
buffer the _batch calls insist on, closed handles, the alphabet a work-size answer of 0 stands for, and the grow-only workspaces.
The five-node tree and three samples of test_samples_args.py, and one 75-branch clade database with a pooled batch of five samples:
this is about the binding, not the kernels."""
import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, synth
from tests import kr_ref as R
from tests import test_samples_args as A

pytestmark = pytest.mark.gpu
B, S, W = A.B, A.S, A.W
N75, S75, N_READS, READ_LEN = 75, 5, 600, 120


class Env:
    def __init__(self):
        import torch
        v = A.values()
        self.parent, self.bl, self.masses = v["parent"], v["bl"], v["masses"]
        self.tree = ra.EdgeTree(self.parent, self.bl)
        self.d_masses = torch.from_numpy(self.masses.view(np.int64)).cuda()
        sdb, genome = synth.make_clade_db(k=8, n_branches=N75, genome_len=12_000, mean_row=6, seed=13)
        self.seq, _ = synth.make_clade_reads(genome, N_READS, READ_LEN, seed=10)
        self.off = np.arange(N_READS + 1, dtype=np.uint64) * READ_LEN
        self.sample = np.random.default_rng(3).integers(0, S75 - 1, N_READS).astype(np.uint32)  # sample S75 - 1 stays empty
        self.parent75, self.bl75 = R.random_tree(N75, 5)
        self.db = ra.PhyloKmerDB.from_synth(sdb, device=0)
        self.tree75 = ra.EdgeTree(self.parent75, self.bl75)
        self.pp = ra.PlacementProcess(self.db)
        self.aa = ra.PhyloKmerDB.from_synth(synth.make_db(20, 3, B, 40, 80, seed=1), device=0)
        packed, lens, flags = ra.pack_reads(ra.RK_ALPHABET_DNA, 8, self.seq, self.off)
        dev = lambda a: torch.from_numpy(a.view(np.int32)).cuda()
        self.d_packed, self.d_lens, self.d_flags = dev(packed), dev(lens), dev(flags)
        torch.cuda.synchronize()

    def close(self):
        for h in (self.tree, self.tree75, self.db, self.aa):
            h.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def refused(text, fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert text in str(e.value), str(e.value)


def same(got, want):
    """bit for bit: a device tensor or host array against a host array (None against None)"""
    if got is None or want is None:
        return got is None and want is None
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    return got.nbytes == want.nbytes and got.tobytes() == np.ascontiguousarray(want).tobytes()


DEVICE_FORMS = {
    "clade_masses": lambda t, m, s: t.clade_masses(m, s),
    "kr_distances": lambda t, m, s: t.kr_distances(m, s),
    "squash": lambda t, m, s: t.squash(m, s),
    "kmeans": lambda t, m, s: t.kmeans(m, s, 2),
    "diversity": lambda t, m, s: t.diversity(m, s),
    "epca": lambda t, m, s: t.epca(m, s, 2, 5),
}


@pytest.mark.parametrize("form", sorted(DEVICE_FORMS))
def test_device_form_masses_tensor(env, form):
    import torch
    call = DEVICE_FORMS[form]
    text = f"masses must be a contiguous int64 tensor of {S * W} (+ 1) words on cuda:0"
    refused(text, call, env.tree, env.d_masses.view(torch.float64), S)                                       # dtype
    refused(text, call, env.tree, env.d_masses[:S * W - 1], S)                                               # word count
    refused(text, call, env.tree, torch.zeros(2 * S * W, dtype=torch.int64, device="cuda")[::2], S)          # not contiguous
    refused(text, call, env.tree, env.d_masses.cpu(), S)                                                     # on the host
    call(env.tree, env.d_masses, S)
    call(env.tree, env.d_masses[:S * W], S)   # the skipped-entries word is optional
    torch.cuda.synchronize()


def test_device_outputs_have_the_dtypes_of_the_host_twins(env):
    import torch
    t, m = env.tree, env.d_masses
    merges, n_merges = t.squash(m, S)
    assert merges.dtype == torch.uint8 and tuple(merges.shape) == (S - 1, 24) and n_merges.dtype == torch.int32 and tuple(n_merges.shape) == (1,)
    want, n_want = ra.squash_host(env.parent, env.bl, env.masses, S)
    assert same(merges, want) and int(n_merges.cpu()[0]) == n_want
    assert same(t.kr_distances(m, S), ra.kr_distances_host(env.parent, env.bl, env.masses, S))
    assert same(t.clade_masses(m, S), ra.clade_masses_host(env.parent, env.masses, S))
    raw, info = t.epca(m, S, 2, 5)
    want_raw, want_info = ra.epca_host(env.parent, env.bl, env.masses, S, 2, 5)
    assert raw.dtype == torch.float64 and info.dtype == torch.int32 and same(raw, want_raw) and same(info, want_info)
    fin, want_fin = ra.epca_finish(B, S, 2, raw, info), ra.epca_finish(B, S, 2, want_raw, want_info)   # device tensors are downloaded
    assert all(same(g, w) for g, w in zip(fin[:5], want_fin[:5])) and fin[5:] == want_fin[5:]
    km = t.kmeans(m, S, 2)
    assert km.centroids is None and [x.dtype for x in km[:5]] == [torch.int32, torch.float64, torch.int32, torch.float64, torch.int32]
    with pytest.raises(ra.RkError) as e:
        t.kmeans(m, S, 0)          # the size call answers 0: its text is the error
    assert e.value.code == _lib.RK_ERR_INVALID and "rk_kmeans_work_bytes: k=0 clusters" in str(e.value)
    with pytest.raises(ra.RkError) as e:
        t.epca(m, S, 9, 5)
    assert e.value.code == _lib.RK_ERR_INVALID and "rk_epca_work_bytes: k=9 components" in str(e.value)
    assert t.kr_work_bytes(S) > 0 and t.diversity_work_bytes(S) > 0 and t.diversity_work_bytes(S, n_theta=2) > 0 and t.edpl_lds_bytes() >= 0


def test_result_set_tensor_checks(env):
    import torch
    out = env.pp.place_packed(env.d_packed, lens=env.d_lens, flags_in=env.d_flags, keepAtMost=A.K)
    n, K = N_READS, A.K
    # EdgeTree.edpl: n_rows, branch, lwr in that order
    t75 = env.tree75
    refused(f"n_rows must be a contiguous torch.uint8 tensor of {n} elements on cuda:0", t75.edpl, dict(out, n_rows=out["n_rows"].view(torch.int8)), K)
    refused(f"branch must be a contiguous torch.int16 tensor of {n * 3} elements on cuda:0", t75.edpl, out, 3)
    refused(f"lwr must be a contiguous torch.float64 tensor of {n * K} elements on cuda:0", t75.edpl, dict(out, lwr=out["lwr"].cpu()), K)
    refused("branch must be a contiguous", t75.edpl, dict(out, branch=out["branch"].t().contiguous().t()), K)
    got = t75.edpl(out, K)
    want = ra.edpl_host(env.parent75, env.bl75, K, out["n_rows"].cpu().numpy(), out["branch"].cpu().numpy().view(np.uint16), out["lwr"].cpu().numpy())
    assert same(got, want)
    assert same(t75.edpl_batch(env.db, K, out["n_rows"].cpu().numpy(), out["branch"].cpu().numpy().view(np.uint16), out["lwr"].cpu().numpy()), want)
    refused(f"branch and lwr must hold n_reads x K = {n} x 3 rows", t75.edpl_batch, env.db, 3, out["n_rows"].cpu().numpy(),
            out["branch"].cpu().numpy().view(np.uint16), out["lwr"].cpu().numpy())
    # accumulate_masses: the mass buffer, then the weights
    pp, words = env.pp, ra.masses_words(N75)
    ones = torch.ones(n, dtype=torch.int32, device="cuda")
    refused(f"weights must be a contiguous int32 tensor of {n} words on cuda:0", pp.accumulate_masses, out, weights=ones.to(torch.int64))
    refused(f"weights must be a contiguous int32 tensor of {n} words", pp.accumulate_masses, out, weights=ones[:-1])
    refused(f"weights must be a contiguous int32 tensor of {n} words", pp.accumulate_masses, out, weights=ones.cpu())
    refused(f"masses must be a contiguous int64 tensor of {words} words on cuda:0", pp.accumulate_masses, out, masses=torch.zeros(words + 1, dtype=torch.int64, device="cuda"))
    refused(f"masses must be a contiguous int64 tensor of {words} words", pp.accumulate_masses, out, masses=torch.zeros(words, dtype=torch.int64))
    refused(f"masses must be a contiguous int64 tensor of {words} words", pp.accumulate_masses, out, weights=ones.cpu(), masses=torch.zeros(1, dtype=torch.int64))
    host = ra.Placements(out["n_rows"].cpu().numpy(), out["branch"].cpu().numpy().view(np.uint16), None, out["lwr"].cpu().numpy(), None, {})
    assert same(pp.accumulate_masses(out, weights=ones), ra.accumulate_masses_host(N75, host))
    # accumulate_masses_samples: the sample count, the buffer, then member_sample, member_read, member_weight
    d_sample = torch.from_numpy(env.sample.view(np.int32)).cuda()
    refused(f"n_samples=0 on {N75} branches: 1..65535 and at most 2^29 words", pp.accumulate_masses_samples, out, 0, d_sample)
    refused(f"member_sample must be a contiguous int32 tensor of {n} words on cuda:0", pp.accumulate_masses_samples, out, S75, d_sample.to(torch.int64))
    refused(f"member_read must be a contiguous int32 tensor of {n} words", pp.accumulate_masses_samples, out, S75, d_sample, member_read=ones[:-1])
    refused(f"member_weight must be a contiguous int32 tensor of {n} words", pp.accumulate_masses_samples, out, S75, d_sample, member_weight=ones.cpu())
    refused(f"masses must be a contiguous int64 tensor of {ra.masses_samples_words(N75, S75)} words", pp.accumulate_masses_samples, out, S75, d_sample,
            masses=torch.zeros(S75 * words, dtype=torch.int64, device="cuda"))
    got = pp.accumulate_masses_samples(out, S75, d_sample, member_read=torch.arange(n, dtype=torch.int32, device="cuda"), member_weight=ones)
    assert same(got, ra.accumulate_masses_samples_host(N75, host, S75, env.sample))


def test_profile_only_argument_checks(env):
    """the checks of the profile-only host forms, which need a database: all of them fire before anything is launched"""
    pp, n = env.pp, N_READS
    per_read = "must be a contiguous uint32 array with one word per read"
    refused("weights " + per_read, pp.processQueriesMasses, env.seq, env.off, weights=np.ones(n - 1, np.uint32))
    refused("weights " + per_read, pp.processQueriesMasses, env.seq, env.off, weights=np.ones(n, np.int32))
    refused("weights " + per_read, pp.processQueriesMasses, env.seq, env.off, weights=[1] * (n + 1))
    refused("flags_out " + per_read, pp.processQueriesMasses, env.seq, env.off, flags_out=np.zeros(n, np.int32))
    refused("flags_out " + per_read, pp.processQueriesMassesSamples, env.seq, env.off, S75, env.sample, flags_out=np.zeros(2 * n, np.uint32)[::2])
    refused(f"masses must be a contiguous uint64 array of {ra.masses_words(N75)} words", pp.processQueriesMasses, env.seq, env.off, masses=np.zeros(3, np.uint64))
    refused("member_off must hold n_reads + 1 uint64 words", pp.processQueriesMassesSamples, env.seq, env.off, S75, env.sample, member_off=np.arange(n))
    refused(f"member_sample must hold {n} uint32 words", pp.processQueriesMassesSamples, env.seq, env.off, S75, env.sample[:-1])
    refused(f"member_weight must hold {2 * n} uint32 words", pp.processQueriesMassesSamples, env.seq, env.off, S75, np.tile(env.sample, 2),
            member_off=np.arange(n + 1) * 2, member_weight=np.ones(n, np.uint32))
    refused(f"n_samples=0 on {N75} branches: both in 1..65535", pp.processQueriesMassesSamples, env.seq, env.off, 0, env.sample)
    refused("strand must be 'forward', 'reverse' or 'both', not 'up'", pp.processQueriesMasses, env.seq, env.off, strand="up")
    packed, lens, flags = pp.pack_reads_host(env.seq, env.off)
    refused("flags_out " + per_read, pp.processQueriesPackedMasses, packed, lens=lens, flags=flags, flags_out=np.zeros(n + 1, np.uint32))
    refused("member_off must hold", pp.processQueriesPackedMassesSamples, packed, S75, env.sample, member_off=np.arange(n), lens=lens, flags=flags)
    mine, my_flags = np.zeros(ra.masses_words(N75), np.uint64), np.zeros(n, np.uint32)
    masses, flags_out, counters = pp.processQueriesPackedMasses(packed, lens=lens, flags=flags, seq=env.seq, seq_off=env.off, weights=[1] * n, masses=mine,
                                                                flags_out=my_flags)
    assert masses is mine and flags_out is my_flags and counters["reads"] == n
    assert same(pp.processQueriesMasses(env.seq, env.off)[0], mine)


@pytest.mark.parametrize("centroids", [False, True])
def test_kmeans_batch_with_seeds_is_the_host_twin(env, centroids):
    words, _, _ = env.pp.processQueriesMassesSamples(env.seq, env.off, S75, env.sample)
    want = ra.kmeans_host(env.parent75, env.bl75, words, S75, 2, max_rounds=7, seeds=[2, 0], centroids=centroids)
    assert (want.centroids is not None) == centroids
    for got in (env.tree75.kmeans_batch(env.db, S75, 2, max_rounds=7, seeds=[2, 0], centroids=centroids),                 # the buffer where the call left it
                env.tree75.kmeans_batch(env.db, S75, 2, max_rounds=7, masses=words, seeds=np.array([2, 0]), centroids=centroids)):
        assert isinstance(got, ra.KMeans)
        for name, g, w in zip(ra.KMeans._fields, got, want):
            assert same(g, w), name
            assert g is None or (g.dtype == w.dtype and g.shape == w.shape), name
    other = env.tree75.kmeans_batch(env.db, S75, 2, masses=words, centroids=centroids)  # farthest-first: other seeds, the same clustering or not
    assert other.info[0] == 2
    refused("seeds must hold k = 2 sample indices", env.tree75.kmeans_batch, env.db, S75, 2, seeds=[0, 1, 2])


def test_host_arrays_read_during_the_call_on_a_side_stream(env):
    import torch
    s2 = torch.cuda.Stream()
    theta = [0.25, 2.0]
    got = env.tree.diversity(env.d_masses, S, theta=theta, stream=s2.cuda_stream)
    km = env.tree.kmeans(env.d_masses, S, 2, max_rounds=10, seeds=[2, 0], centroids=True, stream=s2.cuda_stream)
    kr = env.tree.kr_distances(env.d_masses, S, stream=s2.cuda_stream)
    s2.synchronize()
    want = ra.diversity_host(env.parent, env.bl, env.masses, S, theta=theta)
    assert isinstance(got, ra.Diversity) and got.columns == want.columns and tuple(got.values.shape) == (S, 9) and same(got.values, want.values)
    want = ra.kmeans_host(env.parent, env.bl, env.masses, S, 2, max_rounds=10, seeds=[2, 0], centroids=True)
    for name, g, w in zip(ra.KMeans._fields, km, want):
        assert same(g, w), name
    assert same(kr, ra.kr_distances_host(env.parent, env.bl, env.masses, S))
    refused("seeds must hold k = 2 sample indices", env.tree.kmeans, env.d_masses, S, 2, seeds=[0])


def test_batch_calls_want_the_whole_buffer(env):
    words, _, _ = env.pp.processQueriesMassesSamples(env.seq, env.off, S75, env.sample)
    t, db, short = env.tree75, env.db, words[:-1]
    assert short.shape[0] == S75 * (2 * N75 + 4)
    text = "masses must be a whole sample mass buffer (masses_samples_words)"
    refused(text, t.kr_distances_batch, db, S75, masses=short)
    refused(text, t.squash_batch, db, S75, masses=short)
    refused(text, t.kmeans_batch, db, S75, 2, masses=short)
    refused(text, t.diversity_batch, db, S75, masses=short)
    refused(text, t.epca_batch, db, S75, 2, 5, masses=short)
    refused(f"masses holds {short.shape[0] - 1} words", t.kr_distances_batch, db, S75, short[:-1])
    # the whole buffer, and the one in the handle: the host twins
    assert same(t.kr_distances_batch(db, S75, masses=words), ra.kr_distances_host(env.parent75, env.bl75, words, S75))
    merges, n_merges = t.squash_batch(db, S75, masses=words)
    want, n_want = ra.squash_host(env.parent75, env.bl75, words, S75)
    assert same(merges, want) and merges.dtype == ra.SQUASH_MERGE and type(n_merges) is int and n_merges == n_want == S75 - 2
    for got in (t.diversity_batch(db, S75, theta=[1.5]), t.diversity_batch(db, S75, theta=[1.5], masses=words)):
        want = ra.diversity_host(env.parent75, env.bl75, words, S75, theta=[1.5])
        assert got.columns == want.columns and same(got.values, want.values)
    raw, info = t.epca_batch(db, S75, 2, 5, masses=words)
    want_raw, want_info = ra.epca_host(env.parent75, env.bl75, words, S75, 2, 5)
    assert same(raw, want_raw) and same(info, want_info) and info.dtype == np.uint32
    with pytest.raises(ra.RkError) as e:
        t.epca_batch(db, S75, 9, 5)   # out of range: the array of one double, and the C side speaks
    assert e.value.code == _lib.RK_ERR_INVALID
    with pytest.raises(ra.RkError) as e:
        t.squash_batch(db, 1, words[:2 * N75 + 5])
    assert e.value.code == _lib.RK_ERR_INVALID


def test_closed_handles(env):
    db = env.db.clone()
    assert db.info.n_branches == N75 and db.kernel_name() == env.db.kernel_name()
    tree = ra.EdgeTree(env.parent, env.bl)
    tree.kr_distances(env.d_masses, S)
    assert db.handle and tree.handle
    db.close()
    tree.close()
    with pytest.raises(RuntimeError) as e:
        db.handle
    assert str(e.value) == "PhyloKmerDB is closed"
    with pytest.raises(RuntimeError) as e:
        tree.handle
    assert str(e.value) == "EdgeTree is closed"
    with pytest.raises(RuntimeError):
        db.packed_words(100)
    with pytest.raises(RuntimeError):
        tree.kr_work_bytes(S)
    db.close()      # a second close is silent
    tree.close()
    assert tree._work_buf is None


def test_a_work_size_of_zero_names_the_alphabet(env):
    """the strands need a DNA database and the six frames an amino-acid one: RK_ERR_UNSUPPORTED, not the RK_ERR_INVALID of a bad shape"""
    with pytest.raises(ra.RkError) as e:
        ra.PlacementProcess(env.aa).place_packed(env.d_packed, lens=env.d_lens, strand="both")
    assert e.value.code == _lib.RK_ERR_UNSUPPORTED
    with pytest.raises(ra.RkError) as e:
        env.pp.place_translated(env.d_packed, lens=env.d_lens, flags_in=env.d_flags)
    assert e.value.code == _lib.RK_ERR_UNSUPPORTED
    with pytest.raises(ra.RkError) as e:
        ra.PlacementProcess(env.aa).place_translated(env.d_packed, lens=env.d_lens, flags_in=env.d_flags, keepAtMost=17)
    assert e.value.code == _lib.RK_ERR_INVALID
    refused("strand must be", env.pp.place_packed, env.d_packed, lens=env.d_lens, strand="sideways")


def test_keywords_no_other_test_names(env, tmp_path):
    """stream= of the device helpers (what they give on the current stream), out= / threads= / keepFactor= where no other test passes
    them, device= / user= / convert_uo= of the database's constructors"""
    import torch
    pp, pa = env.pp, ra.PlacementProcess(env.aa)
    s2 = torch.cuda.Stream()
    d_seq, d_off = torch.from_numpy(env.seq).cuda(), torch.from_numpy(env.off.view(np.int64)).cuda()
    torch.cuda.synchronize()

    def both(fn):
        """(on the side stream, on the current one), both finished"""
        there = fn(stream=s2.cuda_stream)
        s2.synchronize()
        here = fn()
        torch.cuda.synchronize()
        return there, here

    there, here = both(lambda **kw: pp.pack_reads(d_seq, d_off, READ_LEN, **kw))
    assert all(torch.equal(a, b) for a, b in zip(there, here)) and [t.dtype for t in here] == [torch.int32] * 3
    assert tuple(here[0].shape) == (N_READS, env.db.packed_words(READ_LEN))
    there, here = both(lambda **kw: pp.revcomp_packed(env.d_packed, lens=env.d_lens, **kw))
    assert torch.equal(there, here) and here.shape == env.d_packed.shape
    there, here = both(lambda **kw: pp.revcomp_ascii(d_seq, d_off, **kw))
    assert torch.equal(there, here) and here.dtype == torch.uint8
    there, here = both(lambda **kw: pp.count_work(env.d_packed, lens=env.d_lens, flags_in=env.d_flags, **kw))
    assert there == here and here["kmers_probed"] > 0
    there, here = both(lambda **kw: pa.translate_packed(env.d_packed, 1, lens=env.d_lens, **kw))
    assert all(torch.equal(a, b) for a, b in zip(there, here)) and tuple(here[0].shape) == (N_READS, ra.translated_words(env.d_packed.shape[1] * 16))
    assert tuple(pa.translate_packed(env.d_packed, 1, fixed_len=READ_LEN, aa_words=9)[0].shape) == (N_READS, 9)
    out = pa.place_translated(env.d_packed, fixed_len=READ_LEN, flags_in=env.d_flags, keepAtMost=3, keepFactor=0.5)
    frame = out["frame"]
    assert pa.place_translated(env.d_packed, fixed_len=READ_LEN, flags_in=env.d_flags, out=out, keepAtMost=3, keepFactor=0.5) is out and out["frame"] is frame
    # host forms
    got = pa.processQueriesTranslated(env.seq, env.off, keepAtMost=3, keepFactor=0.5)
    assert got.frame.shape == (N_READS,) and got.frame.dtype == np.uint8 and got.branch.shape == (N_READS, 3) and got.counters["reads"] == N_READS
    want = pp.pack_reads_host(env.seq, env.off)
    mine = tuple(np.full_like(a, 0xFF) for a in want)
    got = pp.pack_reads_host(env.seq, env.off, max_len=READ_LEN, threads=2, out=mine)
    assert all(g is m and same(g, w) for g, m, w in zip(got, mine, want))
    rule = dict(keepAtMost=3, keepFactor=0.5, treatAmbiguities=False, treatAmbiguitiesWithMax=False)
    want = pp.processQueries(env.seq, env.off, **rule)
    got = pp.processQueriesMulti([env.db], env.seq, env.off, **rule)
    assert pp.processQueriesMulti([env.db], env.seq, env.off, out=got, **rule) is got and got.counters == want.counters
    assert all(same(getattr(got, f), getattr(want, f)) for f in ("n_rows", "branch", "score", "lwr", "flags")) and got.branch.shape == (N_READS, 3)
    # the constructors
    path = tmp_path / "db.img"
    env.db.save(path, user=b"a tree")
    info, user = ra.db_image_info(path)
    assert user == b"a tree" and info.n_branches == N75
    loaded = ra.PhyloKmerDB.load(path, device=0)
    clone = loaded.clone(device=0)
    spec = ra.PhyloKmerDB.synthetic(synth.make_spec("C5tiny", mean_row_len=4.0), device=0, convert_uo=False)
    try:
        assert loaded.info.n_keys == clone.info.n_keys == env.db.info.n_keys and clone.info.device == 0
        assert spec.info.n_branches == 19999 and spec.kernel_name()
    finally:
        for h in (loaded, clone, spec):
            h.close()


def test_workspaces_grow_and_stay(env):
    import torch
    pp = ra.PlacementProcess(env.db)
    half = N_READS // 2
    out = pp.place_packed(env.d_packed[:half], lens=env.d_lens[:half], flags_in=env.d_flags[:half], strand="both")
    first = pp._strand_work
    at, size = first.data_ptr(), first.numel()
    pp.place_packed(env.d_packed[:10], lens=env.d_lens[:10], flags_in=env.d_flags[:10], strand="reverse", out={f: t[:10] for f, t in out.items()})
    assert pp._strand_work is first and (first.data_ptr(), first.numel()) == (at, size)      # a smaller call: the same block
    pp.place_packed(env.d_packed, lens=env.d_lens, flags_in=env.d_flags, strand="both")
    assert pp._strand_work.numel() > size                                                     # a larger one: a larger block
    at, size = pp._strand_work.data_ptr(), pp._strand_work.numel()
    pp.place_packed(env.d_packed[:half], lens=env.d_lens[:half], flags_in=env.d_flags[:half], strand="both")
    assert (pp._strand_work.data_ptr(), pp._strand_work.numel()) == (at, size)
    assert getattr(pp, "_translated_work", None) is None                                      # one workspace per entry point
    # the six frames on the amino-acid database
    pa = ra.PlacementProcess(env.aa)
    out = pa.place_translated(env.d_packed[:half], lens=env.d_lens[:half], flags_in=env.d_flags[:half])
    assert out["frame"].dtype == torch.uint8 and tuple(out["frame"].shape) == (half,)
    at, size = pa._translated_work.data_ptr(), pa._translated_work.numel()
    pa.place_translated(env.d_packed[:10], lens=env.d_lens[:10], flags_in=env.d_flags[:10])
    assert (pa._translated_work.data_ptr(), pa._translated_work.numel()) == (at, size)
    pa.place_translated(env.d_packed, lens=env.d_lens, flags_in=env.d_flags)
    assert pa._translated_work.numel() > size
    # the tree's
    tree = ra.EdgeTree(env.parent75, env.bl75)
    try:
        zeros = lambda s: torch.zeros(s * (2 * N75 + 4), dtype=torch.int64, device="cuda")
        tree.kr_distances(zeros(8), 8)
        at, size = tree._work_buf.data_ptr(), tree._work_buf.numel()
        assert size >= tree.kr_work_bytes(8)
        tree.kr_distances(zeros(2), 2)
        assert (tree._work_buf.data_ptr(), tree._work_buf.numel()) == (at, size)
        tree.kr_distances(zeros(64), 64)
        assert tree._work_buf.numel() >= tree.kr_work_bytes(64) > size
        torch.cuda.synchronize()
    finally:
        tree.close()
