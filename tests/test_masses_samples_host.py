"""CPU: the per-sample edge masses on the host -- rk_masses_accumulate_samples_host against the numpy restatement of the definition
(tests/masses_samples_ref.py: the entries of each sample gathered, then tests/masses_ref.py) for equality of all S * W + 1 words, its
error paths, rk_masses_samples_words at its limits, and the drivers' helpers (sample names, the membership of the unique reads, the
table text) in `rk_place` and in hostio, byte for byte.  No GPU, no handle."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, build, hostio
from tests import masses_ref as MR
from tests import masses_samples_ref as SR

POISON = np.uint64(0xA5A5A5A5DEADBEEF)
N = 3000
SHAPES = [(5, 300), (999, 4), (999, 5), (65535, 3)]


def host(B, S, s, mem, weight=None, masses=None, threads=0):
    return ra.accumulate_masses_samples_host(B, s, S, mem.sample, member_read=mem.read, member_weight=weight, masses=masses, threads=threads)


def test_words_at_the_limits():
    assert ra.masses_samples_words(999, 4) == 8009 and ra.masses_samples_words(999, 5) == 10011 and ra.masses_samples_words(1, 1) == 7
    assert ra.masses_samples_words(0, 1) == 0 and ra.masses_samples_words(65536, 1) == 0
    assert ra.masses_samples_words(5, 0) == 0 and ra.masses_samples_words(5, 65536) == 0
    assert ra.masses_samples_words(5, 65535) == 65535 * 14 + 1
    # S * W + 1 <= 2^29: with W = 131074 (B = 65535) that is S <= 4095, with W = 8196 (B = 4096) the whole 65535 samples fit
    assert ra.masses_samples_words(65535, 4095) == 4095 * 131074 + 1 <= 2 ** 29
    assert 4096 * 131074 + 1 > 2 ** 29 and ra.masses_samples_words(65535, 4096) == 0
    assert ra.masses_samples_words(4094, 65535) == 65535 * 8192 + 1 <= 2 ** 29
    assert 65535 * 8194 + 1 > 2 ** 29 and ra.masses_samples_words(4095, 65535) == 0
    # (W is even, so S * W + 1 is odd and never 2^29 itself)
    assert ra.masses_samples_words(32766, 8191) == 8191 * 65536 + 1 == 2 ** 29 - 65536 + 1


@pytest.mark.parametrize("K", [1, 7, 16])
@pytest.mark.parametrize("B,S", SHAPES)
def test_host_call_equals_the_reference(B, S, K):
    s = MR.make_set(B, K, N, seed=K)
    for kind in SR.KINDS:
        mem = SR.make_members(kind, N, N + N // 3, S, seed=K)
        SR.assert_not_trivial(mem, N, S)
        m = len(mem.sample)
        for wk in (None, "zero", "max", "mixed"):
            w = MR.make_weights(m, wk, seed=K)
            want = SR.masses_samples_ref(B, S, s, mem.sample, mem.read, w)
            got = host(B, S, s, mem, w)
            assert got.dtype == np.uint64 and got.shape == (SR.words(B, S),)
            assert np.array_equal(got, want), (kind, wk, np.flatnonzero(got != want)[:8])
            assert want[-1] == mem.n_planted > 0
            if wk is None:  # the planted rows of the set were met in some sample, and a profile came out
                W = 2 * B + 4
                per = want[:-1].reshape(S, W)
                assert per[:, 2 * B + 3].sum() > 0 and (per[:, 2 * B] > 0).all() and per[:, :B].sum() > 0


@pytest.mark.parametrize("B,S", SHAPES)
def test_adding_into_a_poisoned_buffer_wraps_as_uint64_does(B, S):
    K = 7
    s = MR.make_set(B, K, N, seed=2)
    mem = SR.make_members("csr", N, 0, S, seed=2)
    SR.assert_not_trivial(mem, N, S)
    w = MR.make_weights(len(mem.sample), "mixed", 3)
    start = np.full(SR.words(B, S), POISON, np.uint64) + np.arange(SR.words(B, S), dtype=np.uint64) * np.uint64(0x0123456789ABCDEF)
    tot = np.arange(S) * (2 * B + 4) + 2 * B  # every sample's sum of weights starts one below the wrap
    start[tot] = np.uint64(2 ** 64 - 1)
    want = SR.masses_samples_ref(B, S, s, mem.sample, mem.read, w, masses=start)
    got = host(B, S, s, mem, w, masses=start.copy())
    assert np.array_equal(got, want) and (want[tot] < start[tot]).all()


@pytest.mark.parametrize("B,S", SHAPES)
def test_two_calls_equal_one_and_the_thread_count_plays_no_part(B, S):
    K, n = 7, 3000
    s = MR.make_set(B, K, n, seed=9)
    mem = SR.make_members("csr", n, 0, S, seed=9)
    # enough entries for sixteen threads to have a share each: the list twelve times over, with weights of its own each time
    rd, sm = np.tile(mem.read, 12), np.tile(mem.sample, 12)
    big = SR.SimpleNamespace(read=rd, sample=sm)
    SR.assert_not_trivial(big, n, S)
    m = len(sm)
    assert m > 16 * 4096
    w = MR.make_weights(m, "mixed", 9)
    one = host(B, S, s, big, w, threads=1)
    assert np.array_equal(one, SR.masses_samples_ref(B, S, s, sm, rd, w))
    for t in (3, 16, 0):
        assert np.array_equal(one, host(B, S, s, big, w, threads=t)), t
    cut = m // 3 + 1
    a = SR.SimpleNamespace(read=rd[:cut], sample=sm[:cut])
    b = SR.SimpleNamespace(read=rd[cut:], sample=sm[cut:])
    two = host(B, S, s, a, w[:cut], threads=3)
    assert host(B, S, s, b, w[cut:], masses=two, threads=16) is two
    assert np.array_equal(one, two)


def test_a_read_twice_in_one_sample_counts_twice_the_skipped_rows_included():
    B, K, S = 50, 4, 2
    s = MR.SimpleNamespace(n_rows=np.array([0, 200, 2], np.uint8), branch=np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 0xFFFF, 10, 11]], np.uint16),
                           lwr=np.array([[np.nan, 1e9, 0.5, 0.5], [0.5, 0.25, 0.125, 0.0625], [1.0, 0.5, 0.5, 0.5]]))
    mem = SR.SimpleNamespace(read=np.array([2, 1, 2, 0, 2], np.uint32), sample=np.array([1, 0, 1, 0, 0], np.uint32))
    got = host(B, S, s, mem, np.array([3, 2, 4, 9, 1], np.uint32))
    W = 2 * B + 4
    want = np.zeros(S * W + 1, np.uint64)
    for x, l in zip((5, 6, 7, 8), (0.5, 0.25, 0.125, 0.0625)):
        want[x] = int(2 * l * 2 ** 30)
    want[9], want[B + 5], want[B + 9] = 2 ** 30, 2, 1
    want[2 * B:2 * B + 4] = [2 + 9 + 1, 2 + 1, 2 * 4 + 1, 1]  # read 0 has no rows: weighed in the first total alone
    want[W + 9], want[W + B + 9] = 7 * 2 ** 30, 7
    want[W + 2 * B:W + 2 * B + 4] = [7, 7, 7, 2]
    assert np.array_equal(got, want)
    assert np.array_equal(SR.masses_samples_ref(B, S, s, mem.sample, mem.read, np.array([3, 2, 4, 9, 1], np.uint32)), want)


def test_errors_leave_a_poisoned_buffer_untouched():
    lib = _lib.load()
    B, K, n, S = 999, 7, 100, 4
    s = MR.make_set(B, K, n, seed=4)
    mem = SR.make_members("runs", n, 150, S, seed=4)
    m = len(mem.sample)
    buf = np.full(SR.words(B, S), POISON, np.uint64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(B=B, K=K, n=n, S=S, m=m, n_rows=s.n_rows, branch=s.branch, lwr=s.lwr, read=mem.read, sample=mem.sample, masses=buf, res=True):
        r = _lib.rk_result(p(n_rows), p(branch), None, p(lwr), None)
        return lib.rk_masses_accumulate_samples_host(B, K, n, C.byref(r) if res else None, S, m, p(read), p(sample), None, p(masses), 0)

    for kw in (dict(n_rows=None), dict(branch=None), dict(lwr=None), dict(masses=None), dict(sample=None), dict(res=False), dict(K=0), dict(K=17),
               dict(n=2 ** 32), dict(m=2 ** 32), dict(m=2 ** 40), dict(B=0), dict(B=65536), dict(S=0), dict(S=65536), dict(B=65535, S=4096),
               dict(read=None), dict(read=None, m=n + 1)):
        assert call(**kw) == _lib.RK_ERR_INVALID, kw
        assert lib.rk_last_error() != b"", kw
        assert (buf == POISON).all(), kw
    # no entries: fine, nothing is touched (not even looked at)
    assert lib.rk_masses_accumulate_samples_host(B, K, n, None, S, 0, p(mem.read), None, None, None, 0) == _lib.RK_OK
    assert call(m=0) == _lib.RK_OK and (buf == POISON).all()
    buf[:] = 0
    assert call() == _lib.RK_OK and np.array_equal(buf, SR.masses_samples_ref(B, S, s, mem.sample, mem.read))
    # the identity list: n_members == n_reads
    buf[:] = 0
    assert call(read=None, m=n, sample=mem.sample[:n].copy()) == _lib.RK_OK
    assert np.array_equal(buf, SR.masses_samples_ref(B, S, s, mem.sample[:n]))


# ---- the drivers' helpers: sample names, the membership of the unique reads, the table text -- in both languages ----
NEWICK = "((A:0.1,B:0.2,C:0.3)inner1:0.05,(D:0.1,(E:0.2,F:0.1):0.3,G:0.2,H:0.01)poly:0.1,I:0.4,(J:1,K:2)jk:0.5);"
FASTA = "\n".join([
    ">gut_1 first", "ACGTACGTAC",
    ">soil_1", "ACGTACGTAC",          # the same sequence in a second sample
    ">gut_2 again", "ACGT-ACGTAC",    # ... and once more in the first (a gap does not make it another read)
    ">Zebra_9", "TTTTGGGGCC",         # upper case sorts before lower case: byte-wise order
    ">gut_3", "GGGGCCCCAA",
    ">a_b_c", "GGGGCCCCAA",           # the FIRST separator ends the name
    ">_leading", "CCCCAAAATT",        # an empty sample name
    ">soil_2", "TTTTGGGGCC",
    ">soil_3", "TTTTGGGGCC",
    ">été_1", "CCCCAAAATT",  # bytes above 0x7F sort last
]) + "\n"


def test_sample_members_in_both_languages(tmp_path):
    exe = build.build_host_tools()
    records = hostio.read_fasta(FASTA)
    unique, _ = hostio.dedup_reads(records)
    names, off, sample, weight = hostio.sample_members(records, unique, "_")
    assert names == ["", "Zebra", "a", "gut", "soil", "été"]
    assert [len(unique), off.tolist()] == [4, [0, 2, 4, 6, 8]]
    assert list(zip(sample.tolist(), weight.tolist())) == [(3, 2), (4, 1), (1, 1), (4, 2), (2, 1), (3, 1), (0, 1), (5, 1)]
    (tmp_path / "q.fasta").write_text(FASTA, encoding="utf-8")
    r = subprocess.run([exe, "--sample-members", str(tmp_path / "q.fasta"), "_"], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr
    want = "".join(f"#sample\t{n}\t{i}\n" for i, n in enumerate(names))
    for u in range(len(unique)):
        want += str(u) + "".join(f"\t{sample[e]}:{weight[e]}" for e in range(int(off[u]), int(off[u + 1]))) + "\n"
    assert r.stdout == want.encode("utf-8")
    # a header without the separator is an error that names the header, in both
    bad = FASTA + ">nosep here\nACGT\n"
    (tmp_path / "bad.fasta").write_text(bad, encoding="utf-8")
    r = subprocess.run([exe, "--sample-members", str(tmp_path / "bad.fasta"), "_"], capture_output=True, text=True, timeout=60)
    msg = "--sample-sep: the header 'nosep here' does not contain the separator '_'"
    assert r.returncode != 0 and msg in r.stderr
    with pytest.raises(ValueError, match="nosep here") as ei:
        hostio.sample_members(hostio.read_fasta(bad), hostio.dedup_reads(hostio.read_fasta(bad))[0], "_")
    assert str(ei.value) == msg


def test_both_sample_table_writers_agree_byte_for_byte(tmp_path):
    exe = build.build_host_tools()
    tree = hostio.parse_newick(NEWICK)
    B = len(tree.nodes)
    W = 2 * B + 4
    names = ["", "Zebra", "gut", "été"]
    rng = np.random.default_rng(3)
    m = rng.integers(0, 2 ** 40, len(names) * W + 1).astype(np.uint64)
    m[W + 1], m[2 * W + B + 2], m[-1] = 2 ** 63 + 5, 2 ** 64 - 1, 2 ** 64 - 2
    (tmp_path / "t.nwk").write_text(NEWICK + "\n")
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names), encoding="utf-8")
    m.astype("<u8").tofile(tmp_path / "m.bin")
    args = [exe, "--masses-samples-table", str(tmp_path / "t.nwk"), str(tmp_path / "names.txt"), str(tmp_path / "m.bin")]
    r = subprocess.run(args + [str(tmp_path / "out.tsv")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    text = hostio.masses_samples_table(tree, names, m)
    assert (tmp_path / "out.tsv").read_bytes() == text.encode("utf-8")
    # for each sample: its line, then exactly masses_table of its slice; a last line with the skipped entries
    want = "".join(f"#sample\t{n}\t{s}\n" + hostio.masses_table(tree, m[s * W:(s + 1) * W]) for s, n in enumerate(names))
    assert text == want + f"#skipped_entries\t{2 ** 64 - 2}\n"
    # a buffer of the wrong size is refused by both
    m[:-1].astype("<u8").tofile(tmp_path / "m.bin")
    r = subprocess.run(args + [str(tmp_path / "o2.tsv")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "masses_samples_table" in r.stderr
    with pytest.raises(ValueError):
        hostio.masses_samples_table(tree, names, m[:-1])
