"""The 32-bit compact-table lookup of the pipelined small-tree kernel (rappas_amd/csrc/rk_compact32.h: block and position from the
dense index, first unit and units of the row from the gathered block) compiled for the host and swept by tests/compact_decode.cpp
against a plain prefix sum over the layout rk_device.h defines.  Pure integer arithmetic: no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++")


@pytest.fixture(scope="module")
def compact_decode(tmp_path_factory):
    if not CXX:
        pytest.skip("no C++ compiler (g++)")
    exe = str(tmp_path_factory.mktemp("compact") / "compact_decode")
    subprocess.run([CXX, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "rappas_amd", "csrc"),
                    os.path.join(ROOT, "tests", "compact_decode.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("seed", [1, 20261018])
def test_every_position_of_a_block_decodes_to_its_prefix_sum(compact_decode, seed):
    """both forms x every position (nibble form j = 0..23: the word boundaries 7/8 and 15/16 and the odd 12-block j >= 12; byte form
    i = 0..11: 3/4 and 7/8) x (all zero; all 15 -- a prefix of 345 > 255; all 255; one non-zero entry at each position; one zero among
    full counts; ramps; 1 000 seeded random blocks, three quarters of them with absent k-mers), and the index split on the first 4 096
    indices, around 2^24 blocks, at the top of the 31-bit range and on 100 000 random indices"""
    r = subprocess.run([compact_decode, str(seed), "1000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) positions checked, 0 wrong", r.stdout)
    assert m and int(m.group(1)) >= 1000 * (24 + 12) + 100000 + 4096, r.stdout


def test_header_has_no_hip_dependency():
    src = open(os.path.join(ROOT, "rappas_amd", "csrc", "rk_compact32.h")).read()
    assert "hip_runtime" not in src and "#include <cstdint>" in src
