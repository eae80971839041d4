"""The host twin of the phylogenetic k-means (rappas_amd/csrc/rk_samples_host.h) compiled on its own by tests/kmeans_host.cpp and run
plain and under the address and undefined-behaviour sanitizers.  No GPU, and nothing loaded into Python."""
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
    exe = str(tmp_path_factory.mktemp(name) / "kmeans_host")
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "rappas_amd", "csrc"),
                    os.path.join(ROOT, "tests", "kmeans_host.cpp"), "-o", exe], check=True)
    return exe


def run(exe, seed):
    r = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 wrong", r.stdout)
    assert m and int(m.group(1)) > 400, r.stdout


def test_kmeans_runs_hold_their_definition(tmp_path_factory):
    run(build(tmp_path_factory, "kmeans", "-O2"), 1)


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path_factory):
    run(build(tmp_path_factory, "kmeans_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"), 7)


def test_header_declares_the_kmeans_twin_without_hip():
    src = open(os.path.join(ROOT, "rappas_amd", "csrc", "rk_samples_host.h")).read()
    assert "hip_runtime" not in src
    for name in ("kmeans_seed", "kmeans_distances", "kmeans_assign", "kmeans_update", "kmeans_rounds"):
        assert "inline" in src and name + "(" in src, name
