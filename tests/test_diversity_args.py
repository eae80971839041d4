"""What the diversity calls answer to one bad argument: the return code and the whole text of rk_last_error(), in
the pattern of test_samples_args.py.  Every case starts from a valid call -- that file's five-node tree and buffer of three samples,
two thetas -- and breaks one thing; the expected texts are written out here, from the format strings of the calls.  Here: the host
entry points, and what the device, batch and _work_bytes calls say without a handle.  No GPU; the cases that need a tree handle are
in test_gpu_diversity_args.py, which runs them through run() below."""
import numpy as np
import pytest

from rappas_amd import _lib
from rappas_amd._lib import RK_ERR_INVALID
from tests import test_samples_args as A

B, S, N_THETA = A.B, A.S, 2

CALLS = {
    "rk_diversity_host": "B parent bl S masses n_theta theta out threads",
    "rk_diversity_math_host": "op n x y math_out",
    "rk_diversity_work_bytes": "tree S n_theta",
    "rk_diversity_device": "tree S masses n_theta theta out work work_bytes stream",
    "rk_diversity_batch": "db tree S masses n_theta theta out",
}


def values():
    v = A.values()
    v.update(n_theta=N_THETA, theta=np.array([0.25, 1.0]), out=np.full(S * 9, 7.0), op=2, n=3, x=np.array([0.5, 0.25, 1.0]), y=np.array([1.0, 0.5, 8.0]),
             math_out=np.full(3, 7.0))
    return v


def run(lib, call, change, base=None):
    """(return value, message, the host outputs afterwards) of `call` on valid arguments (`base`: device ones, from the GPU test) with
    `change` laid over them"""
    v = values()
    v.update(base or {})
    v.update(change)
    lib.rk_epca_finish_host(0, 0, 0, None, None, None, None, None, None)  # (leaves a text of its own: no case passes on a stale one)
    keep = []
    rc = getattr(lib, call)(*[A._arg(v[name], keep) for name in CALLS[call].split()])
    return rc, lib.rk_last_error().decode(), v


SAMPLES = A.SAMPLES
N_THETA_RANGE = "n_theta=9 must be in 0..8"
THETA_NAN, THETA_NEG, THETA_BIG = np.array([0.25, np.nan]), np.array([-0.5, 1.0]), np.array([0.25, 8.5])
BAD_THETAS = [
    (dict(n_theta=9, theta=np.zeros(9), out=np.zeros(S * 23)), N_THETA_RANGE),
    (dict(theta=None), "null theta array with n_theta=2"),
    (dict(theta=THETA_NAN), "theta[1]=nan must be in 0..8"),
    (dict(theta=THETA_NEG), "theta[0]=-0.5 must be in 0..8"),
    (dict(theta=THETA_BIG), "theta[1]=8.5 must be in 0..8"),
    (dict(theta=np.array([np.inf, 1.0])), "theta[0]=inf must be in 0..8"),
]

REFUSED = {
    "rk_diversity_host": [
        (dict(B=0), "n_branches=0 must be in 1..65535"),
        (dict(B=65536), "n_branches=65536 must be in 1..65535"),
        (dict(parent=None), "null parent array"),
        (dict(bl=None), "null branch_len array"),
        (dict(parent=A.TWO_ROOTS), "nodes 0 and 1 both have parent -1: one root, not more"),
        (dict(bl=A.BAD_LENGTH), "branch_len[3]=-1 must be finite and not negative"),
        (dict(S=0), SAMPLES % 0),
        (dict(S=65536), SAMPLES % 65536),
        (dict(masses=None), "null mass buffer"),
        (dict(out=None), "null output"),
    ] + BAD_THETAS,
    "rk_diversity_math_host": [
        (dict(op=3), "op=3 must be 0 (log2), 1 (exp2) or 2 (pw)"),
        (dict(x=None), "null input"),
        (dict(math_out=None), "null output"),
        (dict(y=None), "null theta array"),
    ],
    # without a handle (the defaults of A.values() hold no tree and no database): every call says so before anything else
    "rk_diversity_device": [({}, "null tree")],
    "rk_diversity_batch": [({}, "null handle")],
}


def table(cases):
    return [pytest.param(call, change, text, id=f"{call}-{i}") for call, rows in cases.items() for i, (change, text) in enumerate(rows)]


@pytest.mark.parametrize("call,change,text", table(REFUSED))
def test_one_bad_argument_is_refused_with_its_text(call, change, text):
    rc, msg, v = run(_lib.load(), call, change)
    assert (rc, msg) == (RK_ERR_INVALID, f"{call}: {text}")
    for name in ("out", "math_out"):
        assert v[name] is None or (v[name] == (0.0 if name == "out" and "n_theta" in change else 7.0)).all()  # nothing was written


def test_a_size_without_a_tree_is_zero_with_its_text():
    assert run(_lib.load(), "rk_diversity_work_bytes", {})[:2] == (0, "rk_diversity_work_bytes: null tree")


def test_the_valid_calls_the_cases_start_from_are_accepted():
    lib = _lib.load()
    rc, _, v = run(lib, "rk_diversity_host", {})
    assert rc == _lib.RK_OK and not (v["out"] == 7.0).any() and (v["out"].reshape(S, 9)[:, 0] > 0).all()
    rc, _, v = run(lib, "rk_diversity_math_host", {})
    assert rc == _lib.RK_OK and v["math_out"].tolist() == [0.5, 0.5, 1.0]
    assert run(lib, "rk_diversity_math_host", dict(op=0, y=None))[0] == _lib.RK_OK  # y is read by pw only
    assert run(lib, "rk_diversity_host", dict(n_theta=0, theta=None))[0] == _lib.RK_OK  # no thetas: no array
