"""CPU: the host side of placing DNA reads on either strand -- the numpy reverse complement, the drivers' --strand flag, the new
kernels' ISA census, and the argument checks of the new entry points that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rappas_amd import _lib, build, hostio
from rappas_amd.tools import check_isa
from rappas_amd.tools import place as place_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# hand-written: character -> complement, upper case (the lower-case letters map to the lower-case answers)
KNOWN = {"A": "T", "T": "A", "U": "A", "C": "G", "G": "C", "R": "Y", "Y": "R", "K": "M", "M": "K", "B": "V", "V": "B", "D": "H", "H": "D",
         "S": "S", "W": "W", "N": "N"}


def test_revcomp_known_answers_for_every_mapped_character():
    for c, want in KNOWN.items():
        assert hostio.revcomp(c.encode()) == want.encode(), c
        assert hostio.revcomp(c.lower().encode()) == want.lower().encode(), c
    assert hostio.revcomp(b".") == b"." and hostio.revcomp(b"-") == b"-"
    for junk in (b"@", b"!", b"X", b"x", b"0", b" ", b"\x00", b"\xff", b"E", b"z"):
        assert hostio.revcomp(junk) == junk  # copied: an unsupported character stays one
    assert hostio.revcomp(b"AACGTN-ry.u@") == b"@a.ry-NACGTT"
    assert hostio.revcomp("GATTACA") == "TGTAATC"
    assert hostio.revcomp(b"") == b""
    arr = hostio.revcomp(np.frombuffer(b"ACCGu", np.uint8))
    assert arr.dtype == np.uint8 and arr.tobytes() == b"aCGGT"


def test_revcomp_is_an_involution_without_u():
    rng = np.random.default_rng(3)
    letters = np.frombuffer(b"ACGTRYKMBVDHSWNacgtrykmbvdhswn.-@x", np.uint8)
    for n in (0, 1, 2, 15, 16, 17, 150, 1001):
        s = letters[rng.integers(0, len(letters), n)].tobytes()
        assert hostio.revcomp(hostio.revcomp(s)) == s
    assert hostio.revcomp(hostio.revcomp(b"ACGU")) == b"ACGT"  # (U comes back as T: why the involution is stated without it)


def test_revcomp_batch_equals_read_by_read():
    rng = np.random.default_rng(4)
    lens = np.array([0, 1, 7, 16, 0, 33, 150, 2], np.int64)
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    seq = np.frombuffer(b"ACGTNRYacgu-.@", np.uint8)[rng.integers(0, 14, int(off[-1]))]
    got = hostio.revcomp_batch(seq, off)
    want = b"".join(hostio.revcomp(seq[int(off[i]):int(off[i + 1])].tobytes()) for i in range(len(lens)))
    assert got.tobytes() == want
    assert hostio.revcomp_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64)).shape == (0,)


def test_reversed_log_follows_the_notplaced_log():
    records = [("r0 first", "ACGT"), ("r1", "GGGG"), ("r2 dup of r0", "AC-GT"), ("r3", "TTTT")]
    unique, _ = hostio.dedup_reads(records)
    assert [h for h, _ in unique] == ["r0 first", "r1", "r3"]
    flags = np.array([1 | 32, 1, 32], np.uint32)
    assert hostio.reversed_log(records, unique, flags) == "r0 first\nr2 dup of r0\nr3\n"
    assert hostio.reversed_log(records, unique, np.array([1, 1, 0], np.uint32)) == ""


def test_place_tool_parses_strand(tmp_path):
    base = ["--jsondb", str(tmp_path / "missing.json"), "--fasta", str(tmp_path / "missing.fa"), "--out", str(tmp_path / "o.jplace")]
    with pytest.raises(SystemExit) as e:
        place_tool.main(base + ["--strand", "sideways"])
    assert e.value.code == 2
    for s in ("fwd", "rev", "both"):
        with pytest.raises(FileNotFoundError):  # past the parser: the first thing main does is open the database
            place_tool.main(base + ["--strand", s])
    import inspect
    assert inspect.signature(place_tool.place_file).parameters["strand"].default == "fwd"


def test_native_driver_names_the_flag_in_its_help():
    exe = build.build_host_tools()
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--strand fwd|rev|both" in r.stdout
    r = subprocess.run([exe, "--jsondb", "x", "--fasta", "y", "--out", "z", "--strand", "sideways"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--strand" in r.stderr


def test_header_constants_and_binding_agree():
    src = open(os.path.join(ROOT, "include", "rappas_place.h")).read()
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", src).group(1))
    assert (val("RK_STRAND_FORWARD"), val("RK_STRAND_REVERSE"), val("RK_STRAND_BOTH")) == (0, 1, 2)
    assert (_lib.RK_STRAND_FORWARD, _lib.RK_STRAND_REVERSE, _lib.RK_STRAND_BOTH) == (0, 1, 2)
    assert val("RK_FLAG_REVERSE") == 32 == _lib.RK_FLAG_REVERSE
    assert val("RK_VERSION") == 101
    for name in ("rk_revcomp_packed_device", "rk_revcomp_ascii_device", "rk_merge_strands_device", "rk_strands_work_bytes",
                 "rk_place_packed_device_strands", "rk_place_batch_strands"):
        assert name in _lib.EXPORTS and re.search(r"\b" + name + r"\s*\(", src)


def test_new_kernels_hold_no_64_bit_shift_by_a_per_lane_count():
    build.build_engine()
    census = check_isa.variable_shift_census(build.ENGINE_SO)
    for kern in ("revcomp_packed_kernel", "revcomp_ascii_kernel", "merge_results_kernel", "mark_reverse_kernel"):
        found = {k: n for k, n in census.items() if re.match(r"^_ZN2rk\d+" + kern + r"E", k)}
        assert found, f"{kern} is not in the library"
        assert all(n == 0 for n in found.values()), found


def test_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    p = _lib.rk_params(7, 0.01, _lib.RK_AMB_MEAN, float("-inf"))
    buf = (C.c_uint8 * 64)()
    res = _lib.rk_result(*[C.addressof(buf)] * 5)
    ct = _lib.rk_counters()
    a = C.addressof(buf)
    assert lib.rk_revcomp_packed_device(None, 1, a, 1, None, 4, a + 32, None) == _lib.RK_ERR_INVALID
    assert b"null handle" in lib.rk_last_error()
    assert lib.rk_revcomp_ascii_device(None, 1, a, a, a + 32, None) == _lib.RK_ERR_INVALID
    assert lib.rk_merge_strands_device(None, 7, 1, C.byref(res), C.byref(res), None) == _lib.RK_ERR_INVALID
    assert lib.rk_strands_work_bytes(None, 1000, 10, 7, 0) == 0
    assert b"rk_strands_work_bytes" in lib.rk_last_error()
    for strand in (0, 1, 2, 3):
        assert lib.rk_place_packed_device_strands(None, C.byref(p), strand, 1, a, 1, None, 4, None, None, None, C.byref(res), a, 64, None) == _lib.RK_ERR_INVALID
        assert lib.rk_place_batch_strands(None, C.byref(p), strand, 1, a, a, C.byref(res), C.byref(ct)) == _lib.RK_ERR_INVALID
    assert bytes(buf) == bytes(64)  # nothing was written
