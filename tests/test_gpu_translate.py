"""GPU (-m gpu): DNA reads on amino-acid databases -- rk_translate_packed_device against its host twin,
rk_place_packed_device_translated / rk_place_batch_translated against the oracle run on every frame's residues and merged by the
rule of the header (tests/translate_ref.py: nothing expected comes from the engine), the frame tie, the error paths and the
drivers' --translate flag.  Comparisons go through tests/util.py (scores as bit patterns, branches with its tie handling, LWR within
1e-9, flags, n_rows and frame bytes exactly).  Child processes run under a time limit."""
import ctypes as C
import functools
import json
import subprocess

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, hostio, synth
from rappas_amd.tools import place as place_tool
from oracle import oracle as O
from tests import translate_ref as TR
from tests.test_translate_host import grid_reads

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300
AA = "RHKDESTNQCGPAILMFWYV"


def to_host(out):
    return ra.Placements(out["n_rows"].cpu().numpy(), out["branch"].cpu().numpy().view(np.uint16), out["score"].cpu().numpy(),
                         out["lwr"].cpu().numpy(), out["flags"].cpu().numpy().view(np.uint32), {}, out["frame"].cpu().numpy())


def same_arrays(a, b):
    assert np.array_equal(a.n_rows, b.n_rows) and np.array_equal(a.branch, b.branch) and np.array_equal(a.flags, b.flags)
    assert np.array_equal(a.score.view(np.uint32), b.score.view(np.uint32)) and np.array_equal(a.lwr.view(np.uint64), b.lwr.view(np.uint64))
    assert np.array_equal(a.frame, b.frame)


def device_place(db, reads, K=7, ns_bound=float("-inf"), stream=None):
    """characters -> host pack (2 bits a base) -> rk_place_packed_device_translated -> Placements with frame bytes"""
    import torch
    seq, off = TR.batch(reads)
    packed, lens, flags = ra.pack_reads(4, 1, seq, off)
    out = ra.PlacementProcess(db, ns_bound=ns_bound).place_translated(
        torch.from_numpy(packed.view(np.int32)).cuda(), lens=torch.from_numpy(lens.view(np.int32)).cuda(),
        flags_in=torch.from_numpy(flags.view(np.int32)).cuda(), keepAtMost=K, stream=stream)
    torch.cuda.synchronize()
    return to_host(out)


# ---- 1. the device kernel against the host twin ----
def test_device_translation_equals_the_host_twin():
    import torch
    reads = grid_reads()
    seq, off = TR.batch(reads)
    dna, lens, _ = ra.pack_reads(4, 1, seq, off)
    sdb = synth.make_config_db("C4", scale=0.02)
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        pp = ra.PlacementProcess(db)
        d_dna, d_lens = torch.from_numpy(dna.view(np.int32)).cuda(), torch.from_numpy(lens.view(np.int32)).cuda()
        side = torch.cuda.Stream()
        for frame in range(6):
            want, want_lens = ra.translate_packed_host(dna, frame, lens=lens)
            assert db.packed_words(dna.shape[1] * 16 // 3) == want.shape[1]
            aa, aa_lens = pp.translate_packed(d_dna, frame, lens=d_lens)
            torch.cuda.synchronize()
            assert np.array_equal(aa_lens.cpu().numpy().view(np.uint32), want_lens), frame
            assert np.array_equal(aa.cpu().numpy().view(np.uint32), want), frame
            # wider records: the same words, zero beyond; on a stream of its own
            with torch.cuda.stream(side):
                wide, wide_lens = pp.translate_packed(d_dna, frame, lens=d_lens, aa_words=want.shape[1] + 2, stream=side.cuda_stream)
            side.synchronize()
            wide = wide.cpu().numpy().view(np.uint32)
            assert np.array_equal(wide[:, :want.shape[1]], want) and not wide[:, want.shape[1]:].any()
            assert np.array_equal(wide_lens.cpu().numpy().view(np.uint32), want_lens)
        # the fixed_len form, several blocks' worth of reads
        rng = np.random.default_rng(3)
        for R in (0, 2, 3, 47, 48, 49, 150):
            m = 700
            fixed = ["".join("ACGT"[i] for i in rng.integers(0, 4, R)) for _ in range(m)]
            fd, _ = TR.pack_dna(fixed, words=max(1, (2 * R + 31) // 32))
            for frame in (1, 5):
                want, want_lens = ra.translate_packed_host(fd, frame, fixed_len=R)
                aa, aa_lens = pp.translate_packed(torch.from_numpy(fd.view(np.int32)).cuda(), frame, fixed_len=R)
                assert np.array_equal(aa.cpu().numpy().view(np.uint32), want) and np.array_equal(aa_lens.cpu().numpy().view(np.uint32), want_lens), (R, frame)
        with pytest.raises(ra.RkError):  # records too narrow for the longest frame
            pp.translate_packed(d_dna, 0, lens=d_lens, aa_words=want.shape[1] - 1)
        with pytest.raises(ra.RkError):
            pp.translate_packed(d_dna, 6, lens=d_lens)
    finally:
        db.close()


# ---- 2. end to end against the oracle ----
@functools.lru_cache(maxsize=None)
def planted_case(k):
    """an amino-acid database over the k-mers of a random protein 'genome', and ~2 000 DNA reads: stretches of the genome
    back-translated and planted in each of the six frames with 0..2 flanking bases and sometimes a stop codon near one end, random
    DNA, reads shorter than 3k, reads carrying N (and one unsupported character).  -> (sdb, reads, planted frame per read or -1)"""
    n_branches, genome_len = (49, 1500) if k == 3 else (399, 20000)
    sdb, genome = synth.make_clade_db(k=k, n_branches=n_branches, genome_len=genome_len, mean_row=6, seed=20 + k, alphabet=20)
    rng = np.random.default_rng(100 + k)
    reads, planted = [], []
    for i in range(1560):
        L = int(rng.integers(12, 34))
        s = int(rng.integers(0, genome_len - L))
        res = "".join(AA[int(x)] for x in genome[s:s + L])
        if i % 5 == 0:  # a stop codon near one end: the run is the longer side
            cut = int(rng.integers(1, 4)) if i % 10 == 0 else L - int(rng.integers(1, 4))
            res = res[:cut] + "*" + res[cut:]
        f = i % 6
        flank = lambda n: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))
        dna = flank(f % 3) + TR.back_translate(res, rng) + flank(int(rng.integers(0, 3)))
        reads.append(dna if f < 3 else TR.revcomp(dna))
        planted.append(f)
    for i in range(300):  # random DNA
        reads.append("".join("ACGT"[int(x)] for x in rng.integers(0, 4, int(rng.integers(40, 152)))))
    for i in range(60):  # shorter than 3k bases: no frame has a k-mer
        reads.append("".join("ACGT"[int(x)] for x in rng.integers(0, 4, int(rng.integers(0, 3 * k)))))
    for i in range(60):  # an ambiguity code: unplaced, flagged
        r = list(reads[i * 7])
        r[int(rng.integers(0, len(r)))] = "N"
        reads.append("".join(r))
    reads.append(reads[3][:20] + "@" + reads[3][21:])
    planted += [-1] * (len(reads) - len(planted))
    order = rng.permutation(len(reads))
    return sdb, [reads[i] for i in order], np.array(planted)[order]


@functools.lru_cache(maxsize=None)
def planted_expectation(k, K=7):
    sdb, reads, planted = planted_case(k)
    odb = O.OracleDB.from_synth(sdb)
    want, frames = TR.oracle_translated(odb, k, reads, keep_at_most=K)
    return odb, want, frames


def check_planted_conditions(k, want, planted):
    """on the oracle's side alone: the test would pass vacuously if one frame always won or nothing was placed"""
    is_planted = planted >= 0
    placed = want["n_rows"] > 0
    share = [float(((want["frame"] == f) & is_planted).sum()) / is_planted.sum() for f in range(6)]
    print(f"k={k}: planted {is_planted.sum()}, placed {placed[is_planted].mean():.3f} of them; winning frame shares {np.round(share, 3)}; "
          f"planted frame wins {(want['frame'][is_planted] == planted[is_planted]).mean():.3f}")
    assert min(share) >= 0.05, share
    assert placed[is_planted].mean() >= 0.9
    assert ((want["flags"] & TR.AMBIGUOUS) != 0).sum() >= 60 and ((want["flags"] & TR.BAD_CHAR) != 0).sum() == 1
    assert ((want["flags"] & TR.TOO_SHORT) != 0).sum() >= 60


@pytest.mark.parametrize("k", [3, 5])
def test_six_frames_equal_the_oracle_on_every_frame_merged(k, monkeypatch, dev_lib):
    sdb, reads, planted = planted_case(k)
    odb, want, _ = planted_expectation(k)
    check_planted_conditions(k, want, planted)
    monkeypatch.setenv("RK_CHUNK_READS", "1024")  # the host path: ~2 000 reads = two chunks
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        got = device_place(db, reads)
        st = TR.compare(got, got.frame, want, odb)
        assert st["placed"] >= 1400
        seq, off = TR.batch(reads)
        host = ra.PlacementProcess(db).processQueriesTranslated(seq, off)
        same_arrays(host, got)
        fl = host.flags
        assert host.counters == dict(reads=len(reads), placed=int((fl & 1 != 0).sum()), unplaced=int((fl & 1 == 0).sum()), bad_char=int((fl & 2 != 0).sum()),
                                     too_short=int((fl & 4 != 0).sum()), ambiguous=int((fl & 8 != 0).sum()))
    finally:
        db.close()


def test_host_path_over_five_chunks_equals_the_device_call_and_a_fresh_handle(monkeypatch, dev_lib):
    """rk_place_batch_translated through the chunk pipeline: 5 000 ragged DNA reads (0..200 bases, ambiguity codes, unsupported
    characters) in chunks of 1 024 -- five chunks over four workspaces, so the fifth reuses the first -- from pageable arrays and
    from page-locked ones (characters and results both).  Results, frame bytes and counters are bit-equal to
    rk_place_packed_device_translated on rk_pack_reads records of the whole batch (one record width for all reads, where the host
    path's is per chunk) and to the same host call on a fresh handle."""
    import torch
    sdb, _, _ = planted_case(3)
    n, K = 5000, 7
    seq, off = synth.make_reads(4, n, 200, amb_rate=0.01, bad_rate=0.01, var_len=200)
    monkeypatch.setenv("RK_CHUNK_READS", "1024")
    db, fresh = ra.PhyloKmerDB.from_synth(sdb), ra.PhyloKmerDB.from_synth(sdb)
    try:
        packed, lens, flags = ra.pack_reads(4, 1, seq, off)
        want = to_host(ra.PlacementProcess(db).place_translated(
            torch.from_numpy(packed.view(np.int32)).cuda(), lens=torch.from_numpy(lens.view(np.int32)).cuda(),
            flags_in=torch.from_numpy(flags.view(np.int32)).cuda(), keepAtMost=K))
        fl = want.flags
        counters = dict(reads=n, placed=int((fl & 1 != 0).sum()), unplaced=int((fl & 1 == 0).sum()), bad_char=int((fl & 2 != 0).sum()),
                        too_short=int((fl & 4 != 0).sum()), ambiguous=int((fl & 8 != 0).sum()))
        assert counters["placed"] > 0 and counters["bad_char"] > 0 and counters["ambiguous"] > 0 and counters["too_short"] > 0
        h_seq, h_off = ra.host_alloc(seq.shape, np.uint8), ra.host_alloc(off.shape, np.uint64)
        h_seq[:], h_off[:] = seq, off

        def locked_out():
            return ra.Placements(ra.host_alloc(n, np.uint8), ra.host_alloc((n, K), np.uint16), ra.host_alloc((n, K), np.float32),
                                 ra.host_alloc((n, K), np.float64), ra.host_alloc(n, np.uint32), {}, ra.host_alloc(n, np.uint8))

        for handle in (db, fresh):
            pp = ra.PlacementProcess(handle)
            for got in (pp.processQueriesTranslated(seq, off, keepAtMost=K), pp.processQueriesTranslated(h_seq, h_off, keepAtMost=K, out=locked_out())):
                same_arrays(got, want)
                assert got.counters == counters
    finally:
        db.close()
        fresh.close()


def test_a_bound_gates_every_frame_on_its_own():
    k = 3
    sdb, reads, planted = planted_case(k)
    odb, free, _ = planted_expectation(k)
    best = free["score"][:, 0][free["n_rows"] > 0]
    bound = float(np.quantile(best, 0.3))
    want, frames = TR.oracle_translated(odb, k, reads, ns_bound=bound)
    gated = np.array([(fr["flags"] & ra.RK_FLAG_BELOW_NSBOUND) != 0 for fr in frames])
    assert (gated.any(axis=0) & (want["n_rows"] > 0)).sum() > 100  # reads that lose some frames to the bound and keep another
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        got = device_place(db, reads, ns_bound=bound)
        TR.compare(got, got.frame, want, odb)
    finally:
        db.close()


# ---- 3. a score tie between two frames keeps the earlier one ----
def test_a_tie_between_two_frames_keeps_the_earlier():
    k = 3
    sdb, _, _ = planted_case(k)
    rng = np.random.default_rng(9)
    reads = []
    for _ in range(300):  # a read that is its own reverse complement, of 3m bases: frame 3 + o reads what frame o reads
        half = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, 3 * int(rng.integers(4, 25))))
        reads.append(half + TR.revcomp(half))
    assert all(TR.revcomp(r) == r and len(r) % 3 == 0 for r in reads)
    odb = O.OracleDB.from_synth(sdb)
    want, frames = TR.oracle_translated(odb, k, reads)
    assert all(frames[0]["chars"][i] == frames[3]["chars"][i] for i in range(len(reads)))
    assert (want["n_rows"] > 0).sum() > 150 and (want["frame"] == 0).sum() > 20
    assert not ((want["frame"] >= 3) & (want["frame"] <= 5)).any()  # every frame 3 + o ties with frame o
    db = ra.PhyloKmerDB.from_synth(sdb)
    try:
        got = device_place(db, reads)
        assert not (got.flags & ra.RK_FLAG_REVERSE).any()
        TR.compare(got, got.frame, want, odb)
    finally:
        db.close()


# ---- 4. error paths ----
def test_errors_touch_nothing_and_keep_at_most_1_and_16_work():
    import torch
    k = 3
    sdb, reads, _ = planted_case(k)
    reads = reads[:500]
    odb = O.OracleDB.from_synth(sdb)
    lib = _lib.load()
    n, K = len(reads), 7
    seq, off = TR.batch(reads)
    packed, lens, flags = ra.pack_reads(4, 1, seq, off)
    wpr = packed.shape[1]
    d_packed, d_lens = torch.from_numpy(packed.view(np.int32)).cuda(), torch.from_numpy(lens.view(np.int32)).cuda()
    d_flags = torch.from_numpy(flags.view(np.int32)).cuda()
    filled = lambda nbytes: torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    outs = [filled(n), filled(n * K * 2), filled(n * K * 4), filled(n * K * 8), filled(n * 4), filled(n)]
    res = _lib.rk_result(*[t.data_ptr() for t in outs[:5]])
    p = _lib.rk_params(K, 0.01, _lib.RK_AMB_MEAN, float("-inf"))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def untouched(*more):
        torch.cuda.synchronize()
        return all(bool((t == 0xFF).all()) for t in list(outs) + list(more))

    aa = ra.PhyloKmerDB.from_synth(sdb)
    dna = ra.PhyloKmerDB.from_synth(synth.make_config_db("C1"))
    try:
        need = lib.rk_translated_work_bytes(aa.handle, n, wpr, K)
        aa_words = aa.packed_words(wpr * 16 // 3)
        assert need >= n * aa_words * 4 + n * 4 + n * (1 + K * 14 + 4)
        assert lib.rk_translated_work_bytes(aa.handle, n, 0, K) == 0 and lib.rk_translated_work_bytes(aa.handle, n, wpr, 17) == 0
        assert lib.rk_translated_work_bytes(aa.handle, n, wpr, 0) == 0 and b"rk_translated_work_bytes" in lib.rk_last_error()
        work = filled(need)
        place = lambda h, wb, w=work: lib.rk_place_packed_device_translated(h, C.byref(p), n, d_packed.data_ptr(), wpr, d_lens.data_ptr(), 0, d_flags.data_ptr(),
                                                                            C.byref(res), outs[5].data_ptr(), w.data_ptr() if w is not None else None, wb, st)
        # a DNA handle: every new entry point that takes one
        assert place(dna.handle, need) == _lib.RK_ERR_UNSUPPORTED and b"amino-acid" in lib.rk_last_error()
        assert lib.rk_translated_work_bytes(dna.handle, n, wpr, K) == 0
        assert lib.rk_translate_packed_device(dna.handle, 0, n, d_packed.data_ptr(), wpr, d_lens.data_ptr(), 0, work.data_ptr(), aa_words, outs[4].data_ptr(), st) == _lib.RK_ERR_UNSUPPORTED
        assert lib.rk_merge_frames_device(dna.handle, K, n, C.byref(res), outs[5].data_ptr(), C.byref(res), 1, st) == _lib.RK_ERR_UNSUPPORTED
        h = [np.full(s, 0xFF, np.uint8) for s in (n, n * K * 2, n * K * 4, n * K * 8, n * 4, n)]
        hres = _lib.rk_result(*[a.ctypes.data for a in h[:5]])
        ct = _lib.rk_counters()
        assert lib.rk_place_batch_translated(dna.handle, C.byref(p), n, seq.ctypes.data, off.ctypes.data, C.byref(hres), h[5].ctypes.data, C.byref(ct)) == _lib.RK_ERR_UNSUPPORTED
        with pytest.raises(ra.RkError) as e:
            ra.PlacementProcess(dna).processQueriesTranslated(seq, off)
        assert e.value.code == _lib.RK_ERR_UNSUPPORTED
        # a workspace one byte short, or none; a candidate frame that is none
        assert place(aa.handle, need - 1) == _lib.RK_ERR_INVALID and b"rk_translated_work_bytes" in lib.rk_last_error()
        assert place(aa.handle, need, None) == _lib.RK_ERR_INVALID
        assert lib.rk_merge_frames_device(aa.handle, K, n, C.byref(res), outs[5].data_ptr(), C.byref(res), 6, st) == _lib.RK_ERR_INVALID
        # the DNA flags in the output flag array: every frame reads them, the first frame's result would overwrite them
        assert lib.rk_place_packed_device_translated(aa.handle, C.byref(p), n, d_packed.data_ptr(), wpr, d_lens.data_ptr(), 0, outs[4].data_ptr(), C.byref(res),
                                                     outs[5].data_ptr(), work.data_ptr(), need, st) == _lib.RK_ERR_INVALID
        assert untouched(work) and all((a == 0xFF).all() for a in h)
        # ... and with exactly the bytes asked for the call goes through
        assert place(aa.handle, need) == _lib.RK_OK
        torch.cuda.synchronize()
        assert not bool((outs[4] == 0xFF).all())
        for K2 in (1, 16):
            want, _ = TR.oracle_translated(odb, k, reads, keep_at_most=K2)
            got = device_place(aa, reads, K=K2)
            assert TR.compare(got, got.frame, want, odb)["placed"] > 300
    finally:
        aa.close()
        dna.close()


# ---- 5. the drivers ----
def test_drivers_translate_flag(tmp_path):
    from rappas_amd import build
    exe = build.build_host_tools()
    k = 3
    sdb, reads, _ = planted_case(k)
    nwk = synth.make_newick(sdb.n_branches, seed=6)
    tree = hostio.parse_newick(nwk)
    ra.save_db_image(str(tmp_path / "db.rkimg"), sdb.alphabet, sdb.k, sdb.n_branches, sdb.thr_log10, sdb.thr, sdb.key_codes, sdb.row_offsets,
                     sdb.branch_ids, sdb.scores, user=hostio.tree_to_blob(tree))
    lines = []
    for i, r in enumerate(reads[:240]):
        r = r.replace("@", "A")
        if not r:
            continue
        lines += [f">read{i} sample=x/{i}", r[:60]] + ([r[60:]] if len(r) > 60 else [])
        if i % 10 == 3 and len(r) > 8:  # a duplicate with a gap inserted and another header
            lines += [f">dup{i} of read{i}", r[:7] + "-" + r[7:]]
    (tmp_path / "q.fasta").write_text("\n".join(lines) + "\n")
    base = ["--dbimage", str(tmp_path / "db.rkimg"), "--fasta", str(tmp_path / "q.fasta"), "--out", str(tmp_path / "out.jplace")]
    log = tmp_path / "logs" / "frames_q.fasta.tsv"

    assert place_tool.main(base + ["--translate"]) == 0
    py, py_log = (tmp_path / "out.jplace").read_bytes(), log.read_text()
    log.unlink()
    (tmp_path / "out.jplace").unlink()
    for extra in ([], ["--classic-io"]):
        r = subprocess.run([exe] + base + ["--translate"] + extra, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "out.jplace").read_bytes().replace(b" --classic-io", b"") == py
        assert log.read_text() == py_log
    # placed reads and frames are the reference's
    records = hostio.read_fasta((tmp_path / "q.fasta").read_text())
    unique, _ = hostio.dedup_reads(records)
    odb = O.OracleDB.from_synth(sdb)
    want, _ = TR.oracle_translated(odb, k, [s for _, s in unique])
    index = {s.replace("-", ""): i for i, (_, s) in enumerate(unique)}
    name = lambda f: ("+" if f < 3 else "-") + str(f % 3 + 1)
    want_log = "".join(f"{h}\t{name(int(want['frame'][index[s.replace('-', '')]]))}\n" for h, s in records if want["frame"][index[s.replace("-", "")]] <= 5)
    assert py_log == want_log and "dup" in py_log and all(("\t" + name(f) + "\n") in py_log for f in range(6))
    assert len(json.loads(py)["placements"]) == int((want["n_rows"] > 0).sum()) > 150
    # a DNA database refuses the flag, in both drivers
    dsdb = synth.make_config_db("C1")
    (tmp_path / "dna.json").write_text(hostio.dump_jsondb(dsdb, synth.make_newick(dsdb.n_branches, seed=6)))
    dna_base = ["--jsondb", str(tmp_path / "dna.json")] + base[2:]
    r = subprocess.run([exe] + dna_base + ["--translate"], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode != 0 and "--translate needs an amino-acid database" in r.stderr
    assert place_tool.main(dna_base + ["--translate"]) != 0
