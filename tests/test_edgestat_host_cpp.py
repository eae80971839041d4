"""The host twin of the edge statistics (rappas_amd/csrc/rk_edgestat_host.h) compiled on its own by tests/edgestat_host.cpp, without
the library: the raw words and the finished tables it prints equal the numpy restatement word for word -- plain, optimised, and built
with the address and undefined-behaviour sanitizers, run as a program.  No GPU, and nothing loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import edgestat_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++")
SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")


def build(tmp_path_factory, name, *flags):
    if not CXX:
        pytest.skip("no C++ compiler (g++)")
    exe = str(tmp_path_factory.mktemp(name) / "edgestat_host")
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "rappas_amd", "csrc"),
                    os.path.join(ROOT, "tests", "edgestat_host.cpp"), "-o", exe], check=True)
    return exe


def shapes(text):
    """the shapes the program printed"""
    out, cur = [], None
    words = lambda f: np.array([int(v, 16) for v in f[1:]], np.uint64)
    for line in text.splitlines():
        f = line.split(" ")
        if f[0] == "shape":
            cur = {"B": int(f[1]), "S": int(f[2]), "F": int(f[3]), "mass": [], "meta": []}
            out.append(cur)
        elif f[0] == "parent":
            cur["parent"] = np.array(f[1:], np.int32)
        elif f[0] == "mass":
            cur["mass"].append(np.array([int(v) for v in f[1:]], np.uint64))
        elif f[0] == "meta":
            cur["meta"].append(words(f).view(np.float64))
        elif f[0] == "info":
            cur["info"] = [int(f[1]), int(f[2])]
        elif f[0] in ("raw", "table", "features"):
            cur[f[0]] = words(f)
    return out


@pytest.mark.parametrize("flags", [("-O0",), ("-O2",), SANITIZE], ids=["O0", "O2", "sanitizers"])
def test_standalone_twin_equals_the_definition_bit_for_bit(tmp_path_factory, flags):
    r = subprocess.run([build(tmp_path_factory, "edgestat", *flags), "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("done 0 wrong\n"), r.stdout[-2000:] + r.stderr[-4000:]
    got = shapes(r.stdout)
    assert [(g["B"], g["S"], g["F"]) for g in got] == [(1, 1, 0), (40, 5, 3), (9, 64, 1), (25, 65, 8), (6, 200, 2)]
    for g in got:
        B, S, F = g["B"], g["S"], g["F"]
        W = 2 * B + 4
        m = np.zeros(S * W + 1, np.uint64)
        for s in range(S):
            m[s * W:s * W + B] = g["mass"][s]
        meta = np.array(g["meta"], np.float64).reshape(F, S)
        want, info = E.edgestat_ref(g["parent"], m, S, meta)
        assert g["info"] == info.tolist() and (g["raw"] == want).all(), (B, S, F)
        table, ftab = E.finish_ref(B, want, info)
        assert E.same_table(g["table"].view(np.float64).reshape(B, 8 + 4 * F), table) and E.same_table(g["features"].view(np.float64).reshape(F, 2), ftab)
    assert got[1]["info"] == [4, 4] and np.isnan(got[1]["meta"][1][1])  # the NaN of the empty sample leaves column 1 usable; column 2 is not


def test_headers_declare_the_twin_without_hip():
    host = open(os.path.join(ROOT, "rappas_amd", "csrc", "rk_edgestat_host.h")).read()
    math = open(os.path.join(ROOT, "rappas_amd", "csrc", "rk_samplemath.h")).read()
    assert "hip_runtime" not in host and "fma(" not in host and "fma(" not in math
    for name in ("edgestat_share", "edgestat_imbalance", "edgestat_centre", "edgestat_rank_dev"):
        assert name + "(" in math and name + "(" in host + open(os.path.join(ROOT, "rappas_amd", "csrc", "rk_edgestat.h")).read(), name
