"""The slot-word arithmetic of the dense 24-entry row units (rappas_amd/csrc/rk_slots24.h: which two words of the score vector a lane
updates in one accumulate step, from the word the masked DPP leaves it) compiled for the host and swept by tests/dense_slot_words.cpp
against the format rk_device.h defines.  Pure integer arithmetic: no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++")


@pytest.fixture(scope="module")
def slot_words(tmp_path_factory):
    if not CXX:
        pytest.skip("no C++ compiler (g++)")
    exe = str(tmp_path_factory.mktemp("slots") / "dense_slot_words")
    subprocess.run([CXX, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "rappas_amd", "csrc"),
                    os.path.join(ROOT, "tests", "dense_slot_words.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("seed", [1, 20261016])
def test_every_lane_gets_the_slots_the_format_defines(slot_words, seed):
    """16 lanes x (each triple of 0, 1, 511, 512, 1 022, 1 023 in the three fields of each of the eight slot words, among zero and
    all-ones neighbours; the same triple in every word; an all-zero padding unit; 200 000 seeded random units): lanes 0..7 get
    slot(li) and slot(16 + li), lanes 8..15 slot(li) and the scratch word; the increments in lanes 0..7 never leak into a slot"""
    r = subprocess.run([slot_words, str(seed), "200000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) lanes checked, 0 wrong", r.stdout)
    assert m and int(m.group(1)) >= 16 * (2 * 8 * 216 + 216 + 1 + 200000), r.stdout


def test_header_has_no_hip_dependency():
    src = open(os.path.join(ROOT, "rappas_amd", "csrc", "rk_slots24.h")).read()
    assert "hip_runtime" not in src and "#include <cstdint>" in src
