"""The launch plan of windowed trees with short rows (rappas_amd/csrc/rk_plan.h: the first kernel of each class of batch the re-tiling
pre-pass finds on the device, and the tiles place_packed16w_kernel takes behind it) compiled for the host and swept over a dense grid
by tests/plan_grid.cpp.  Pure host arithmetic: no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++")


@pytest.fixture(scope="module")
def plan_grid(tmp_path_factory):
    if not CXX:
        pytest.skip("no C++ compiler (g++)")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_grid")
    subprocess.run([CXX, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "rappas_amd", "csrc"),
                    os.path.join(ROOT, "tests", "plan_grid.cpp"), "-o", exe], check=True)
    return exe


def plan_of(exe, bits, k, wpr, lens, fixed_len, units_per_code, entries_per_key, n_branches, hash_capable=1, stream=1, verdict=1,
            first_ok=1, marked_list=1):
    args = [bits, k, wpr, lens, fixed_len, units_per_code, entries_per_key, n_branches, hash_capable, stream, verdict, first_ok, marked_list]
    out = subprocess.run([exe, "case", *map(str, args)], check=True, capture_output=True, text=True).stdout
    return dict(line.split("=", 1) for line in out.split())


F_NONE, F_SORTED, F_HASH_BIG, F_HASH_SMALL = "0", "1", "2", "3"


def test_every_class_of_batch_is_placed_on_the_whole_grid(plan_grid):
    """n_branches 1 117 ... 65 535, est_units 0 ... 400, DNA and amino acids, ragged and fixed-length reads of every record size, all
    the booleans of the plan and its developer knobs: each class the pre-pass can find (uniform, sparse-hit, clade-shaped) is served by
    a first kernel or taken whole by place_packed16w_kernel (never both), no sorted-stream kernel without sorted_fits, no hash kernel
    without hash_fits, and without a verdict the three classes share one kernel"""
    r = subprocess.run([plan_grid], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 rules violated" in r.stdout


def test_long_protein_records_on_a_mid_size_tree(plan_grid):
    """amino acids, k = 5, C4-like rows (~0.34 row units per code, ten entries a key), 9 001 branches, records of 17 words: no kernel
    goes first for uniform and clade-shaped batches, the 1 024-slot table for sparse-hit ones -- place_packed16w_kernel takes only the
    marked tiles of sparse-hit batches and every tile of the other two classes"""
    p = plan_of(plan_grid, 5, 5, 17, 1, 0, 0.34, 10.0, 9001)
    assert (p["for_uniform"], p["for_sparse"], p["for_clade"]) == (F_NONE, F_HASH_SMALL, F_NONE), p
    assert p["hash_small"] == "1,2" and p["hash_behind"] == "1,2" and p["hash_big"].startswith("0,") and p["sorted"].startswith("0,"), p
    assert p["only_marked"] == "1" and p["marked_if"] == "2", p
    # the same reads at one known length beyond the probe batch (120 residues: 116 k-mers > 7 x 16)
    p = plan_of(plan_grid, 5, 5, 19, 0, 120, 0.34, 10.0, 9001)
    assert p["one_batch"] == "0" and p["sorted_fits"] == "0" and p["marked_if"] == "2", p
    # ... and within it (102 residues, 16 words): the sorted-stream kernel for every class, all tiles only when marked
    p = plan_of(plan_grid, 5, 5, 16, 0, 102, 0.34, 10.0, 9001)
    assert p["sorted_fits"] == "1" and p["only_marked"] == "1" and p["marked_if"] == "0", p
    # without the pre-pass's verdict one rule for all: no first kernel, every tile to place_packed16w_kernel
    p = plan_of(plan_grid, 5, 5, 17, 1, 0, 0.34, 10.0, 9001, verdict=0)
    assert p["for_uniform"] == p["for_sparse"] == p["for_clade"] == F_NONE and p["only_marked"] == "0", p


def test_plans_that_serve_every_class_keep_their_launches(plan_grid):
    """C2-like reads (DNA, k = 10, 150 bp in 10 words, ~1 row unit per code): the sorted-stream kernel first on small trees, the
    hash kernel on large ones -- every class has a first kernel, so place_packed16w_kernel takes only marked tiles of all three"""
    for nb, first in ((9001, F_SORTED), (65535, F_HASH_BIG)):
        p = plan_of(plan_grid, 2, 10, 10, 1, 0, 1.0, 9.3, nb)
        assert F_NONE not in (p["for_uniform"], p["for_sparse"], p["for_clade"]) and p["for_uniform"] == first, p
        assert p["only_marked"] == "1" and p["marked_if"] == "0", p
