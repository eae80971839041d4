"""What the sample-level calls answer to one bad argument: the return code and the whole text of
rk_last_error(), call by call.  Every case starts from a valid call -- the five-node tree of test_samples_host.py, a buffer of three
samples, a result set of four reads -- and breaks one thing.  The expected texts are written out here, from the format strings of the
calls.  Here: every host entry point, and what the device, batch and _work_bytes calls say without a handle.  No GPU; the cases that
need a tree handle are in test_gpu_samples_args.py, which runs them through run() below."""
import ctypes as C

import numpy as np
import pytest

from rappas_amd import _lib
from rappas_amd._lib import RK_ERR_INVALID, rk_result

B, S, K, N_READS = 5, 3, 2, 4
W = 2 * B + 4

# the arguments of every call, by the names of values()
CALLS = {
    "rk_tree_validate": "B parent bl",
    "rk_tree_create": "device B parent bl handle_out",
    "rk_clade_masses_host": "B parent S masses clade",
    "rk_kr_distances_host": "B parent bl S masses D threads",
    "rk_squash_host": "B parent bl S masses merges n_merges threads",
    "rk_kmeans_host": "B parent bl S masses k rounds seeds assign dist sizes within info centroids threads",
    "rk_epca_host": "B parent bl S masses k iters raw info threads",
    "rk_epca_finish_host": "B S k raw eigenvalue share residual projection loading",
    "rk_edpl_host": "B parent bl K n_reads res edpl threads",
    "rk_tree_distance_host": "B parent bl n_pairs a b d",
    "rk_clade_masses_device": "tree S masses clade stream",
    "rk_kr_work_bytes": "tree S",
    "rk_squash_work_bytes": "tree S",
    "rk_kmeans_work_bytes": "tree S k",
    "rk_epca_work_bytes": "tree S k",
    "rk_edpl_lds_bytes": "tree",
    "rk_kr_distances_device": "tree S masses D work work_bytes stream",
    "rk_squash_device": "tree S masses merges n_merges work work_bytes stream",
    "rk_kmeans_device": "tree S masses k rounds seeds assign dist sizes within info centroids work work_bytes stream",
    "rk_epca_device": "tree S masses k iters raw info work work_bytes stream",
    "rk_edpl_device": "tree K n_reads res edpl stream",
    "rk_kr_distances_batch": "db tree S masses D",
    "rk_squash_batch": "db tree S masses merges n_merges",
    "rk_kmeans_batch": "db tree S masses k rounds seeds assign dist sizes within info centroids",
    "rk_epca_batch": "db tree S masses k iters raw info",
    "rk_edpl_batch": "db tree K n_reads res edpl",
}


def values():
    """a valid call's arguments on the host: arrays large enough for what the calls write, k = 2 clusters or components"""
    masses = np.zeros(S * W + 1, np.uint64)
    masses[0 * W + 1] = masses[1 * W + 3] = masses[2 * W + 4] = 1 << 30
    return dict(
        B=B, S=S, K=K, n_reads=N_READS, k=2, rounds=10, iters=5, threads=1, n_pairs=2, device=0, stream=None, seeds=None,
        parent=np.array([-1, 0, 0, 2, 2], np.int32), bl=np.array([0, 1, 3, 2, 4], np.float32), masses=masses,
        clade=np.zeros(S * B, np.uint64), D=np.zeros(S * S), merges=np.zeros(24 * (S - 1), np.uint8), n_merges=np.zeros(1, np.uint32),
        assign=np.zeros(S, np.uint32), dist=np.zeros(S), sizes=np.zeros(2, np.uint32), within=np.zeros(2), info=np.zeros(4, np.uint32),
        centroids=np.zeros(2 * 2 * B), raw=np.zeros(1 + 2 * (3 + S + B)), eigenvalue=np.zeros(2), share=np.zeros(2), residual=np.zeros(2),
        projection=np.zeros(S * 2), loading=np.zeros(B * 2), edpl=np.zeros(N_READS), a=np.array([1, 4], np.uint16), b=np.array([3, 0], np.uint16),
        d=np.zeros(2), res=dict(n_rows=np.full(N_READS, K, np.uint8), branch=np.tile(np.array([1, 3], np.uint16), N_READS), lwr=np.full(N_READS * K, 0.5)),
        handle_out=C.c_void_p(), tree=None, db=None, work=None, work_bytes=0)


def _arg(v, keep):
    if isinstance(v, np.ndarray):
        return C.c_void_p(v.ctypes.data)
    if isinstance(v, dict):  # a result set: its three arrays as addresses (numpy arrays or plain integers) or None
        addr = {n: (int(x.ctypes.data) if isinstance(x, np.ndarray) else x) for n, x in v.items()}
        keep.append(rk_result(addr["n_rows"], addr["branch"], None, addr["lwr"], None))
        return C.byref(keep[-1])
    if isinstance(v, C.c_void_p) and v.value is None:  # where a call returns a handle
        return C.byref(v)
    return v


def run(lib, call, change, base=None):
    """(return value, message) of `call` on valid arguments (`base`: device ones, from the GPU test) with `change` laid over them"""
    v = values()
    v.update(base or {})
    v.update(change)
    lib.rk_epca_finish_host(0, 0, 0, None, None, None, None, None, None)  # (leaves a text of its own: no case passes on a stale one)
    keep = []
    rc = getattr(lib, call)(*[_arg(v[name], keep) for name in CALLS[call].split()])
    return rc, lib.rk_last_error().decode()


def no_lwr():
    r = values()["res"]
    r["lwr"] = None
    return r


TWO_ROOTS = np.array([-1, -1, 0, 2, 2], np.int32)
BAD_LENGTH = np.array([0, 1, 3, -1, 4], np.float32)
SAMPLES = "n_samples=%u must be in 1..65535"
SAMPLES_2 = "n_samples=%u must be in 2..4096"

# call -> (what is changed, the text behind "<call>: ")
REFUSED = {
    "rk_tree_validate": [
        (dict(B=0), "n_branches=0 must be in 1..65535"),
        (dict(B=65536), "n_branches=65536 must be in 1..65535"),
        (dict(parent=None), "null parent array"),
        (dict(bl=None), "null branch_len array"),
        (dict(parent=TWO_ROOTS), "nodes 0 and 1 both have parent -1: one root, not more"),
        (dict(parent=np.array([-1, 0, 0, 9, 2], np.int32)), "parent[3]=9 is outside 0..4"),
        (dict(parent=np.array([-1, 0, -2, 2, 2], np.int32)), "parent[2]=-2 is outside 0..4"),
        (dict(parent=np.array([-1, 0, 2, 2, 2], np.int32)), "parent[2] is the node itself"),
        (dict(parent=np.array([1, 0, 0, 2, 2], np.int32)), "no node has parent -1: the tree has no root"),
        (dict(parent=np.array([-1, 0, 3, 2, 2], np.int32)), "node 2 does not reach the root (a cycle among the parents)"),
        (dict(bl=BAD_LENGTH), "branch_len[3]=-1 must be finite and not negative"),
        (dict(bl=np.array([0, 1, np.nan, 2, 4], np.float32)), "branch_len[2]=nan must be finite and not negative"),
        (dict(bl=np.array([0, 1, 3, 2, np.inf], np.float32)), "branch_len[4]=inf must be finite and not negative"),
    ],
    "rk_tree_create": [
        (dict(handle_out=None), "null out"),
        (dict(B=0), "n_branches=0 must be in 1..65535"),
        (dict(parent=None), "null parent array"),
        (dict(bl=None), "null branch_len array"),
        (dict(parent=TWO_ROOTS), "nodes 0 and 1 both have parent -1: one root, not more"),
        (dict(bl=BAD_LENGTH), "branch_len[3]=-1 must be finite and not negative"),
    ],
    "rk_clade_masses_host": [
        (dict(B=0), "n_branches=0 must be in 1..65535"),
        (dict(parent=None), "null parent array"),
        (dict(parent=TWO_ROOTS), "nodes 0 and 1 both have parent -1: one root, not more"),
        (dict(S=0), SAMPLES % 0),
        (dict(S=65536), SAMPLES % 65536),
        (dict(masses=None), "null mass buffer"),
        (dict(clade=None), "null output"),
    ],
    "rk_kr_distances_host": [
        (dict(B=65536), "n_branches=65536 must be in 1..65535"),
        (dict(parent=None), "null parent array"),
        (dict(bl=None), "null branch_len array"),
        (dict(parent=TWO_ROOTS), "nodes 0 and 1 both have parent -1: one root, not more"),
        (dict(bl=BAD_LENGTH), "branch_len[3]=-1 must be finite and not negative"),
        (dict(S=0), SAMPLES % 0),
        (dict(S=65536), SAMPLES % 65536),
        (dict(masses=None), "null mass buffer"),
        (dict(D=None), "null output"),
    ],
    "rk_squash_host": [
        (dict(B=0), "n_branches=0 must be in 1..65535"),
        (dict(parent=None), "null parent array"),
        (dict(bl=None), "null branch_len array"),
        (dict(parent=TWO_ROOTS), "nodes 0 and 1 both have parent -1: one root, not more"),
        (dict(bl=BAD_LENGTH), "branch_len[3]=-1 must be finite and not negative"),
        (dict(S=1), SAMPLES_2 % 1),
        (dict(S=4097), SAMPLES_2 % 4097),
        (dict(masses=None), "null mass buffer"),
        (dict(merges=None), "null output"),
        (dict(n_merges=None), "null output"),
    ],
    "rk_kmeans_host": [
        (dict(B=0), "n_branches=0 must be in 1..65535"),
        (dict(parent=None), "null parent array"),
        (dict(bl=None), "null branch_len array"),
        (dict(parent=TWO_ROOTS), "nodes 0 and 1 both have parent -1: one root, not more"),
        (dict(bl=BAD_LENGTH), "branch_len[3]=-1 must be finite and not negative"),
        (dict(S=0), SAMPLES % 0),
        (dict(S=65536), SAMPLES % 65536),
        (dict(k=0), "k=0 clusters must be in 1..64"),
        (dict(k=65), "k=65 clusters must be in 1..64"),
        (dict(rounds=0), "max_rounds=0 must be in 1..1024"),
        (dict(rounds=1025), "max_rounds=1025 must be in 1..1024"),
        (dict(masses=None), "null mass buffer"),
        (dict(assign=None), "null output"),
        (dict(dist=None), "null output"),
        (dict(sizes=None), "null output"),
        (dict(within=None), "null output"),
        (dict(info=None), "null output"),
        (dict(seeds=np.array([0, 3], np.uint32)), "seeds[1]=3, the buffer has 3 samples"),
        (dict(seeds=np.array([1, 1], np.uint32)), "seeds[0] and seeds[1] are both sample 1"),
    ],
    "rk_epca_host": [
        (dict(B=0), "n_branches=0 must be in 1..65535"),
        (dict(parent=None), "null parent array"),
        (dict(bl=None), "null branch_len array"),
        (dict(parent=TWO_ROOTS), "nodes 0 and 1 both have parent -1: one root, not more"),
        (dict(bl=BAD_LENGTH), "branch_len[3]=-1 must be finite and not negative"),
        (dict(S=1), SAMPLES_2 % 1),
        (dict(S=4097), SAMPLES_2 % 4097),
        (dict(k=0), "k=0 components must be in 1..8"),
        (dict(k=9), "k=9 components must be in 1..8"),
        (dict(iters=0), "iters=0 must be in 1..10000"),
        (dict(iters=10001), "iters=10001 must be in 1..10000"),
        (dict(masses=None), "null mass buffer"),
        (dict(raw=None), "null output"),
        (dict(info=None), "null output"),
    ],
    "rk_epca_finish_host": [
        (dict(B=0), "n_branches=0, n_samples=3, k=2: out of 1..65535, 2..4096, 1..8"),
        (dict(B=65536), "n_branches=65536, n_samples=3, k=2: out of 1..65535, 2..4096, 1..8"),
        (dict(S=1), "n_branches=5, n_samples=1, k=2: out of 1..65535, 2..4096, 1..8"),
        (dict(S=4097), "n_branches=5, n_samples=4097, k=2: out of 1..65535, 2..4096, 1..8"),
        (dict(k=0), "n_branches=5, n_samples=3, k=0: out of 1..65535, 2..4096, 1..8"),
        (dict(k=9), "n_branches=5, n_samples=3, k=9: out of 1..65535, 2..4096, 1..8"),
        (dict(raw=None), "null raw output"),
        (dict(eigenvalue=None), "null output"),
        (dict(share=None), "null output"),
        (dict(residual=None), "null output"),
        (dict(projection=None), "null output"),
        (dict(loading=None), "null output"),
    ],
    "rk_edpl_host": [
        (dict(B=0), "n_branches=0 must be in 1..65535"),
        (dict(parent=None), "null parent array"),
        (dict(bl=None), "null branch_len array"),
        (dict(parent=TWO_ROOTS), "nodes 0 and 1 both have parent -1: one root, not more"),
        (dict(bl=BAD_LENGTH), "branch_len[3]=-1 must be finite and not negative"),
        (dict(K=0), "keep_at_most=0 outside 1..16"),
        (dict(K=17), "keep_at_most=17 outside 1..16"),
        (dict(n_reads=1 << 32), "n_reads=4294967296, at most 2^32 - 1 per call"),
        (dict(res=None), "null result array (n_rows, branch and lwr are read)"),
        (dict(res=no_lwr()), "null result array (n_rows, branch and lwr are read)"),
        (dict(edpl=None), "null output"),
    ],
    "rk_tree_distance_host": [
        (dict(B=0), "n_branches=0 must be in 1..65535"),
        (dict(parent=None), "null parent array"),
        (dict(bl=None), "null branch_len array"),
        (dict(parent=TWO_ROOTS), "nodes 0 and 1 both have parent -1: one root, not more"),
        (dict(bl=BAD_LENGTH), "branch_len[3]=-1 must be finite and not negative"),
        (dict(a=None), "null branch array"),
        (dict(b=None), "null branch array"),
        (dict(d=None), "null output"),
        (dict(a=np.array([1, 5], np.uint16)), "pair 1 is (5, 0), the tree has 5 branches"),
        (dict(b=np.array([7, 0], np.uint16)), "pair 0 is (1, 7), the tree has 5 branches"),
    ],
}
# without a handle (the defaults of values() hold no tree and no database): every call says so before anything else
for _call in ("rk_clade_masses_device", "rk_kr_distances_device", "rk_squash_device", "rk_kmeans_device", "rk_epca_device", "rk_edpl_device"):
    REFUSED[_call] = [({}, "null tree")]
for _call in ("rk_kr_distances_batch", "rk_squash_batch", "rk_kmeans_batch", "rk_epca_batch", "rk_edpl_batch"):
    REFUSED[_call] = [({}, "null handle")]
# the calls that return a size: 0, and the text
NO_SIZE = {call: [({}, "null tree")] for call in ("rk_kr_work_bytes", "rk_squash_work_bytes", "rk_kmeans_work_bytes", "rk_epca_work_bytes", "rk_edpl_lds_bytes")}


def table(cases):
    return [pytest.param(call, change, text, id=f"{call}-{i}") for call, rows in cases.items() for i, (change, text) in enumerate(rows)]


@pytest.mark.parametrize("call,change,text", table(REFUSED))
def test_one_bad_argument_is_refused_with_its_text(call, change, text):
    assert run(_lib.load(), call, change) == (RK_ERR_INVALID, f"{call}: {text}")


@pytest.mark.parametrize("call,change,text", table(NO_SIZE))
def test_a_size_without_a_tree_is_zero_with_its_text(call, change, text):
    assert run(_lib.load(), call, change) == (0, f"{call}: {text}")


@pytest.mark.parametrize("call", [c for c in CALLS if c.endswith("_host") or c == "rk_tree_validate"])
def test_the_valid_call_the_cases_start_from_is_accepted(call):
    assert run(_lib.load(), call, {})[0] == _lib.RK_OK
