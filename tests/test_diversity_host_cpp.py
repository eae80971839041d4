"""The host twin of the per-sample diversity measures (rappas_amd/csrc/rk_samples_host.h, rk_divmath.h) compiled on its own by
tests/diversity_host.cpp, without the library: the rows it prints equal the numpy restatement word for word.  No GPU, and nothing
loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import diversity_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++")


def build(tmp_path_factory, name, *flags):
    if not CXX:
        pytest.skip("no C++ compiler (g++)")
    exe = str(tmp_path_factory.mktemp(name) / "diversity_host")
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "rappas_amd", "csrc"),
                    os.path.join(ROOT, "tests", "diversity_host.cpp"), "-o", exe], check=True)
    return exe


def shapes(text):
    """the shapes the program printed: (parent, branch_len, theta, masses [S, B], rows [S, C] as bit patterns)"""
    out, cur = [], None
    for line in text.splitlines():
        f = line.split(" ")
        if f[0] == "shape":
            cur = {"B": int(f[1]), "S": int(f[2]), "mass": [], "row": []}
            out.append(cur)
        elif f[0] == "parent":
            cur["parent"] = np.array(f[1:], np.int32)
        elif f[0] == "branch_len":
            cur["bl"] = np.array([float.fromhex(v) for v in f[1:]], np.float32)
        elif f[0] == "theta":
            cur["theta"] = [float.fromhex(v) for v in f[1:]]
        elif f[0] == "mass":
            cur["mass"].append(np.array([int(v) for v in f[1:]], np.uint64))
        elif f[0] == "row":
            cur["row"].append(np.array([int(v, 16) for v in f[1:]], np.uint64))
    return out


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_standalone_twin_equals_the_definition_bit_for_bit(tmp_path_factory, opt):
    r = subprocess.run([build(tmp_path_factory, "diversity" + opt, opt), "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.endswith("done 0 wrong\n"), r.stdout[-2000:] + r.stderr
    got = shapes(r.stdout)
    assert [(g["B"], g["S"], len(g["theta"])) for g in got] == [(300, 4, 3), (2100, 3, 0), (2100, 3, 8)]
    for g in got:
        B, S = g["B"], g["S"]
        W = 2 * B + 4
        m = np.zeros(S * W + 1, np.uint64)
        for s in range(S):
            m[s * W:s * W + B] = g["mass"][s]
        want = V.diversity_ref(g["parent"], g["bl"], m, S, g["theta"])
        assert (np.stack(g["row"]) == want.view(np.uint64)).all(), (B, S)
        assert (want.view(np.uint64)[1] == V.NAN_BITS).all() and want[2, 1] == 0.0 and want[2, 0] > 0.0  # the empty sample; all mass on one branch: no PD


def test_headers_declare_the_twin_without_hip_or_libm():
    host = open(os.path.join(ROOT, "rappas_amd", "csrc", "rk_samples_host.h")).read()
    math = open(os.path.join(ROOT, "rappas_amd", "csrc", "rk_divmath.h")).read()
    assert "hip_runtime" not in host and "hip_runtime" not in math and "<cmath>" not in math and "fma(" not in math
    for name in ("rk_log2", "rk_exp2", "rk_pw", "diversity_half", "diversity_node"):
        assert name + "(" in math, name
    assert "diversity_row(" in host and "diversity_sample(" in host
