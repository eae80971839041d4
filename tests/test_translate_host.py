"""CPU: the host side of placing DNA reads on amino-acid databases -- the codon table, rk_translate_packed_host against the
pure-Python reference (tests/translate_ref.py) and the numpy twin (hostio.translate_frames), the frames log, the drivers'
--translate flag, and the argument checks of the new entry points that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, build, hostio
from rappas_amd.tools import check_isa
from rappas_amd.tools import place as place_tool
from tests import translate_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# hand-written: codon -> residue, the 64 answers of NCBI table 1 grouped by residue ('*' = stop)
KNOWN = {
    "F": "TTT TTC", "L": "TTA TTG CTT CTC CTA CTG", "I": "ATT ATC ATA", "M": "ATG", "V": "GTT GTC GTA GTG",
    "S": "TCT TCC TCA TCG AGT AGC", "P": "CCT CCC CCA CCG", "T": "ACT ACC ACA ACG", "A": "GCT GCC GCA GCG",
    "Y": "TAT TAC", "*": "TAA TAG TGA", "H": "CAT CAC", "Q": "CAA CAG", "N": "AAT AAC", "K": "AAA AAG",
    "D": "GAT GAC", "E": "GAA GAG", "C": "TGT TGC", "W": "TGG", "R": "CGT CGC CGA CGG AGA AGG", "G": "GGT GGC GGA GGG",
}
STATE = "RHKDESTNQCGPAILMFWYV"


def grid_reads():
    """the length and stop grid of the issue: lengths 0..70 and 150..152 of random DNA, stops first / last / adjacent / only, two
    runs of equal length, runs of 6, 7, 12, 13, 19, 20 residues (residues 6, 12 and 19 straddle word boundaries)"""
    rng = np.random.default_rng(11)
    reads = ["".join("ACGT"[i] for i in rng.integers(0, 4, L)) for L in list(range(71)) + [150, 151, 152] * 3]
    sense = lambda n: "".join(TR.back_translate(STATE[int(i)], rng) for i in rng.integers(0, 20, n))
    reads += ["TAA" + sense(9), sense(9) + "TGA", sense(4) + "TAATAG" + sense(5), "TAATAGTGA", "TAG", "TGATAA" + "TAG" * 20,
              sense(5) + "TAA" + sense(5), sense(5) + "TAG" + sense(5) + "TGA" + sense(4), "C" + sense(6) + "TAA" + sense(6) + "GG"]
    for n in (6, 7, 12, 13, 19, 20, 25, 26, 32):
        reads += [sense(n), "TAA" + sense(n) + "TAG" + sense(2), "A" + sense(n), TR.revcomp(sense(n)), TR.revcomp("GT" + sense(n) + "TGA")]
    return reads


def test_codon_table_against_64_hand_written_answers():
    seen = 0
    for aa, codons in KNOWN.items():
        for codon in codons.split():
            idx = sum("ATCG".index(b) << (2 * t) for t, b in enumerate(codon))
            want = hostio.CODON_STOP if aa == "*" else STATE.index(aa)
            assert hostio.CODON_TABLE[idx] == want, codon
            assert TR.CODE[codon] == aa, codon
            # ... and the engine's own table, through the host twin: one codon -> one residue (a stop: none)
            dna, lens = TR.pack_dna([codon])
            rec, n = ra.translate_packed_host(dna, 0, lens=lens)
            assert (int(n[0]), int(rec[0, 0])) == ((0, 0) if aa == "*" else (1, want)), codon
            seen += 1
    assert seen == 64 and len({c for v in KNOWN.values() for c in v.split()}) == 64


@pytest.mark.parametrize("frame", range(6))
def test_host_twin_equals_the_reference_and_the_numpy_twin(frame):
    reads = grid_reads()
    dna, lens = TR.pack_dna(reads)
    aa_words = ra.translated_words(dna.shape[1] * 16)
    want, want_lens = TR.expected_records(reads, frame, aa_words)
    got, got_lens = ra.translate_packed_host(dna, frame, lens=lens)
    assert got.shape == want.shape
    assert np.array_equal(got_lens, want_lens)
    assert np.array_equal(got, want)
    np_aa, np_lens = hostio.translate_frames(dna, lens)
    assert np.array_equal(np_aa[frame], want) and np.array_equal(np_lens[frame], want_lens)
    assert want_lens.max() >= 32 and (want_lens == 0).sum() >= 3  # (reads of 0, 1, 2 bases have no codon in any frame)
    # aa_words larger than needed: the same words, then zeros
    wide, wide_lens = ra.translate_packed_host(dna, frame, lens=lens, aa_words=aa_words + 3)
    assert np.array_equal(wide[:, :aa_words], want) and not wide[:, aa_words:].any() and np.array_equal(wide_lens, want_lens)
    # a record in a buffer filled with ones comes back with every bit from 5 * len on zero
    lib = _lib.load()
    buf = np.full((len(reads), aa_words + 1), 0xFFFFFFFF, np.uint32)
    out_lens = np.full(len(reads), 0xFFFFFFFF, np.uint32)
    assert lib.rk_translate_packed_host(frame, len(reads), dna.ctypes.data, dna.shape[1], lens.ctypes.data, 0, buf.ctypes.data, aa_words + 1,
                                        out_lens.ctypes.data) == _lib.RK_OK
    assert np.array_equal(buf[:, :aa_words], want) and not buf[:, aa_words:].any()


@pytest.mark.parametrize("R", [0, 1, 2, 3, 4, 5, 6, 47, 48, 49, 150])
def test_fixed_len_without_lens(R):
    rng = np.random.default_rng(R)
    reads = ["".join("ACGT"[i] for i in rng.integers(0, 4, R)) for _ in range(40)]
    dna, _ = TR.pack_dna(reads, words=max(1, (2 * R + 31) // 32) + 1)
    for frame in range(6):
        aa_words = ra.translated_words(R)
        got, got_lens = ra.translate_packed_host(dna, frame, fixed_len=R)
        want, want_lens = TR.expected_records(reads, frame, aa_words)
        assert got.shape == want.shape and np.array_equal(got, want) and np.array_equal(got_lens, want_lens)
        np_aa, np_lens = hostio.translate_frames(dna, fixed_len=R)
        assert np.array_equal(np_aa[frame], want) and np.array_equal(np_lens[frame], want_lens)


def test_two_runs_of_equal_length_keep_the_first():
    a, b = "GCTGCTGCTGCT", "GGTGGTGGTGGT"  # AAAA, GGGG
    dna, lens = TR.pack_dna([a + "TAA" + b, b + "TGA" + a + "TAG"])
    rec, n = ra.translate_packed_host(dna, 0, lens=lens)
    assert n.tolist() == [4, 4]
    assert rec[0, 0] == sum(12 << (5 * i) for i in range(4)) and rec[1, 0] == sum(10 << (5 * i) for i in range(4))


def test_lengths_beyond_the_record_are_cut_to_it():
    dna, _ = TR.pack_dna(["GCT" * 16])  # 48 bases in 3 words
    rec, n = ra.translate_packed_host(dna, 0, lens=np.array([1000], np.uint32))
    assert n[0] == 16 and rec.shape == (1, 3)


def test_argument_checks_that_need_no_device():
    lib = _lib.load()
    dna = np.zeros((2, 3), np.uint32)
    lens = np.array([48, 48], np.uint32)
    aa = np.full((2, 4), 0xFFFFFFFF, np.uint32)
    out_lens = np.full(2, 0xFFFFFFFF, np.uint32)
    host = lambda frame, dna_words, lens_p, fixed, aa_words: lib.rk_translate_packed_host(frame, 2, dna.ctypes.data, dna_words, lens_p, fixed, aa.ctypes.data,
                                                                                          aa_words, out_lens.ctypes.data)
    # 48 bases = 16 residues = 80 bits = 3 words; with lengths the record's capacity counts, without them fixed_len
    assert host(0, 3, lens.ctypes.data, 0, 2) == _lib.RK_ERR_INVALID and b"aa_words" in lib.rk_last_error()
    assert host(0, 3, None, 48, 2) == _lib.RK_ERR_INVALID
    assert host(0, 3, None, 38, 2) == _lib.RK_OK  # 12 residues = 60 bits
    assert host(6, 3, lens.ctypes.data, 0, 3) == _lib.RK_ERR_INVALID and b"frame" in lib.rk_last_error()
    assert host(0, 3, None, 49, 3) == _lib.RK_ERR_INVALID  # fixed_len beyond the record
    assert host(0, 0, lens.ctypes.data, 0, 3) == _lib.RK_ERR_INVALID
    assert lib.rk_translate_packed_host(0, 2, None, 3, None, 48, aa.ctypes.data, 3, out_lens.ctypes.data) == _lib.RK_ERR_INVALID
    aa[:] = 0xFFFFFFFF
    out_lens[:] = 0xFFFFFFFF
    assert host(0, 3, lens.ctypes.data, 0, 2) == _lib.RK_ERR_INVALID
    assert (aa == 0xFFFFFFFF).all() and (out_lens == 0xFFFFFFFF).all()  # a refused call writes nothing
    # the entry points that take a handle refuse a null one before they look at a device
    p = _lib.rk_params(7, 0.01, _lib.RK_AMB_MEAN, float("-inf"))
    buf = (C.c_uint8 * 64)()
    a = C.addressof(buf)
    res = _lib.rk_result(*[a] * 5)
    ct = _lib.rk_counters()
    assert lib.rk_translated_work_bytes(None, 1000, 10, 7) == 0 and b"rk_translated_work_bytes" in lib.rk_last_error()
    assert lib.rk_translate_packed_device(None, 0, 1, a, 1, None, 4, a + 32, 1, a + 48, None) == _lib.RK_ERR_INVALID
    assert b"null handle" in lib.rk_last_error()
    assert lib.rk_merge_frames_device(None, 7, 1, C.byref(res), a, C.byref(res), 1, None) == _lib.RK_ERR_INVALID
    assert lib.rk_place_packed_device_translated(None, C.byref(p), 1, a, 1, None, 4, None, C.byref(res), a, a, 64, None) == _lib.RK_ERR_INVALID
    assert lib.rk_place_batch_translated(None, C.byref(p), 1, a, a, C.byref(res), a, C.byref(ct)) == _lib.RK_ERR_INVALID
    assert bytes(buf) == bytes(64)  # nothing was written


def test_header_constants_and_binding_agree():
    src = open(os.path.join(ROOT, "include", "rappas_place.h")).read()
    assert int(re.search(r"#define\s+RK_VERSION\s+(\d+)", src).group(1)) == 101
    assert int(re.search(r"#define\s+RK_FRAME_NONE\s+0x([0-9A-Fa-f]+)", src).group(1), 16) == _lib.RK_FRAME_NONE == TR.NONE
    for name in ("rk_translate_packed_device", "rk_translate_packed_host", "rk_merge_frames_device", "rk_translated_work_bytes",
                 "rk_place_packed_device_translated", "rk_place_batch_translated"):
        assert name in _lib.EXPORTS and re.search(r"\b" + name + r"\s*\(", src)
    assert "without a bump" in src


def test_frames_log_follows_the_reversed_log():
    records = [("r0 first", "ACGT"), ("r1", "GGGG"), ("r2 dup of r0", "AC-GT"), ("r3", "TTTT"), ("r4", "CCCC")]
    unique, _ = hostio.dedup_reads(records)
    assert [h for h, _ in unique] == ["r0 first", "r1", "r3", "r4"]
    assert hostio.frames_log(records, unique, np.array([4, 0xFF, 0, 2], np.uint8)) == "r0 first\t-2\nr2 dup of r0\t-2\nr3\t+1\nr4\t+3\n"
    assert hostio.frames_log(records, unique, np.array([3, 5, 1, 0xFF], np.uint8)) == "r0 first\t-1\nr1\t-3\nr2 dup of r0\t-1\nr3\t+2\n"
    assert hostio.frames_log(records, unique, np.full(4, 0xFF, np.uint8)) == ""


def test_place_tool_parses_translate(tmp_path, capsys):
    base = ["--jsondb", str(tmp_path / "missing.json"), "--fasta", str(tmp_path / "missing.fa"), "--out", str(tmp_path / "o.jplace")]
    for strand in ("rev", "both"):
        with pytest.raises(SystemExit) as e:
            place_tool.main(base + ["--translate", "--strand", strand])
        assert e.value.code == 2
        assert "--translate" in capsys.readouterr().err
    for extra in (["--translate"], ["--translate", "--strand", "fwd"]):
        with pytest.raises(FileNotFoundError):  # past the parser: the first thing main does is open the database
            place_tool.main(base + extra)
    import inspect
    assert inspect.signature(place_tool.place_file).parameters["translate"].default is False
    with pytest.raises(ValueError, match="--strand"):
        place_tool.place_file(b"", b"", strand="both", translate=True)


def test_native_driver_names_the_flag_and_refuses_it_with_strand():
    exe = build.build_host_tools()
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--translate" in r.stdout and "frames_<query>.tsv" in r.stdout
    for strand in ("rev", "both"):
        r = subprocess.run([exe, "--jsondb", "x", "--fasta", "y", "--out", "z", "--translate", "--strand", strand], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--translate" in r.stderr and "--strand" in r.stderr


def test_new_kernels_hold_no_64_bit_shift_by_a_per_lane_count():
    build.build_engine()
    census = check_isa.variable_shift_census(build.ENGINE_SO)
    for kern in ("translate_frame_kernel", "merge_results_kernel", "init_frame_kernel"):
        found = {k: n for k, n in census.items() if re.match(r"^_ZN2rk\d+" + kern + r"E", k)}
        assert found, f"{kern} is not in the library"
        assert all(n == 0 for n in found.values()), found
