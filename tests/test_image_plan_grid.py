"""The image plan (rappas_amd/csrc/rk_image_plan.h: row layout, k-mer tables, the amino-acid dense index) compiled for the host and swept
over its inputs by tests/image_plan_grid.cpp.  Pure host arithmetic: no GPU.  (The images the plan gives whole databases are compared
with their recorded headers in tests/test_image_plan.py.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++")


@pytest.fixture(scope="module")
def image_plan_grid(tmp_path_factory):
    if not CXX:
        pytest.skip("no C++ compiler (g++)")
    exe = str(tmp_path_factory.mktemp("image_plan") / "image_plan_grid")
    subprocess.run([CXX, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "rappas_amd", "csrc"),
                    os.path.join(ROOT, "tests", "image_plan_grid.cpp"), "-o", exe], check=True)
    return exe


def test_every_image_keeps_the_rules_its_kernels_read_it_by(image_plan_grid):
    """row lengths 1 ... 70, 239 ... 242, 4 079 ... 4 082 and n_branches, both forms of the layout, both alphabets, every table mode:
    descriptors inside the blob, rows apart and on unit boundaries behind their index line, the compact table's counts summing to the
    blob's units block by block, hash tables at load <= 0.5 with every key found by the device's probe, and the amino-acid code <->
    dense index a bijection for k = 2 and 3 (tests/image_plan_grid.cpp: rule)"""
    r = subprocess.run([image_plan_grid], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 rules violated" in r.stdout
