"""The pure rules of the host path (rappas_amd/csrc/rk_chunks.h: how a batch is cut into chunks, how a chunk's flags become the
counters of the call) compiled for the host and held against their definitions by tests/chunks.cpp.  Integer arithmetic: no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++")


def build(tmp_path_factory, name, *flags):
    if not CXX:
        pytest.skip("no C++ compiler (g++)")
    exe = str(tmp_path_factory.mktemp(name) / "chunks")
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "rappas_amd", "csrc"),
                    os.path.join(ROOT, "tests", "chunks.cpp"), "-o", exe], check=True)
    return exe


def run(exe, seed, n_batches):
    r = subprocess.run([exe, str(seed), str(n_batches)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) chunks and counts checked, 0 wrong", r.stdout)
    assert m and int(m.group(1)) >= n_batches + 200, r.stdout


@pytest.mark.parametrize("seed", [1, 20261019])
def test_every_chunking_follows_the_rule_and_the_counters_the_recount(tmp_path_factory, seed):
    """batches of n = 0, 1, max_reads - 1, max_reads, max_reads + 1 and 3 max_reads + 7 reads (max_reads = 8, max_bytes = 64) without
    offsets, of all-empty reads, of reads that fill the byte limit exactly, with one read of exactly max_bytes / max_bytes + 1 at the
    start, in the middle and at the end; runs whose bytes hit the limit exactly; 400 seeded ragged batches.  Each chunking: a partition,
    within both limits unless a single read, maximal, max_len the longest read.  count_flags on every combination of the five low flag
    bits against a per-bit recount, at every split into two chunks, and add()."""
    run(build(tmp_path_factory, "chunks", "-O2"), seed, 400)


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path_factory):
    run(build(tmp_path_factory, "chunks_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"), 7, 300)


def test_header_has_no_hip_dependency():
    src = open(os.path.join(ROOT, "rappas_amd", "csrc", "rk_chunks.h")).read()
    assert "hip_runtime" not in src and "#include <cstdint>" in src
