"""The launch geometry of the placement kernels (rappas_amd/csrc/rk_geometry.h: the LDS a block gets, how it is cut up, the blocks a CU
is asked to hold) compiled for the host and swept over its inputs by tests/geometry_grid.cpp, and compared field by field with
tests/golden/launch_geometry.tsv -- the table the arithmetic gave when it was moved out of rk_engine.hip, before anything in it was
restructured.  Pure host arithmetic: no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++")
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_geometry.tsv")


@pytest.fixture(scope="module")
def geometry_grid(tmp_path_factory):
    if not CXX:
        pytest.skip("no C++ compiler (g++)")
    exe = str(tmp_path_factory.mktemp("geometry") / "geometry_grid")
    subprocess.run([CXX, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "rappas_amd", "csrc"),
                    os.path.join(ROOT, "tests", "geometry_grid.cpp"), "-o", exe], check=True)
    return exe


def case(exe, family, **inputs):
    out = subprocess.run([exe, "case", family, *(f"{k}={v}" for k, v in inputs.items())], check=True, capture_output=True, text=True).stdout
    return dict(kv.split("=", 1) for kv in out.rstrip("\n").split("\t")[2].split())


def test_every_layout_fits_its_allocation_on_the_whole_grid(geometry_grid):
    """every n_branches 1 ... 65 535, a CU of 160 KB and of 64 KB, DNA and amino acids, keep_at_most 1 ... 16, lanes_per_read 0 / 8 / 16 /
    32 / 64, records of 1 ... 40 words, 1 / 2 / 4 forced passes, both hash tables, the ambiguity kernel with and without the row index:
    the rules the kernels rely on (tests/geometry_grid.cpp: check_*) hold everywhere"""
    r = subprocess.run([geometry_grid], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 rules violated" in r.stdout


def test_geometries_are_the_ones_recorded_before_the_move(geometry_grid):
    """every field of every geometry at the tree sizes where a path changes, against the recorded table"""
    got = subprocess.run([geometry_grid, "table", GOLDEN], check=True, capture_output=True, text=True).stdout.splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert len(want) > 1800
    differ = [(w, g) for w, g in zip(want, got) if w != g]
    assert len(got) == len(want) and not differ, differ[:5]
    # the table covers the sizes and families it is meant to (a table cut short would compare equal to itself)
    listed = subprocess.run([geometry_grid, "list"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert [l.split("\t")[:2] for l in listed] == [l.split("\t")[:2] for l in want]


def test_values_the_source_states(geometry_grid):
    """14 592 B per wave for a C4-like dense wave (397 branches, amino acids); 17 920 B and nine waves per CU for the 2 048-slot hash
    kernel; 1 280 words per read for eight windowed waves; two workgroups of 8 waves at 19 999 branches"""
    g = case(geometry_grid, "dense", nb=397, bits=5, keep=7, lanes=0, lds=160 * 1024)
    assert (g["G"], g["lds_per_wave"], g["list_cap"], g["pu"]) == ("16", "14592", "256", "7"), g
    h = case(geometry_grid, "hash", log_slots=11, lds=160 * 1024)
    assert (h["lds_wave"], h["waves_cu"], h["s_stride"]) == ("17920", "9", "2048"), h
    for nb in (1277, 3999, 9001, 39999, 65535):
        p = case(geometry_grid, "plan", nb=nb, bits=2, upc=1.0, upr=1.5)
        assert p["planned"] == "1" and int(p["lds_wave"]) <= 1280 * 16 and int(p["s_stride"]) + int(p["main_cap"]) + int(p["work_cap"]) <= 1280, p
        w = case(geometry_grid, "windowed", nb=nb, bits=2, upc=1.0, upr=1.5, keep=7, wpr=10, lds=160 * 1024)
        assert w["waves_cu"] == "8", w
    assert case(geometry_grid, "plan", nb=1277, bits=2, upc=1.0, upr=1.5)["lds_wave"] == str(1280 * 16)
    wg = case(geometry_grid, "wg", nb=19999, keep=7, passes=1, lds=160 * 1024)
    assert (wg["wgs_per_cu"], wg["nw"], wg["n_pass"]) == ("2", "8", "1"), wg
