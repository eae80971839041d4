"""GPU (-m gpu): the weigh stage every placement kernel ends in (weigh_and_store: the -308 rule, the likelihood weight ratios, the
keep-factor cut, the ns_bound gate) on the line trees of tests/weighplant.py, through the routes of tests/test_gpu_tie_order.py.

The reads sit on -308.0f, on the floats next to it and on either side; their neighbours in a wave are in the other regime; some have
every term of the unshifted sum below the smallest normal binary64, some a term that underflows to +0.0, some their best score on the
ns_bound itself.  Every read goes through every route of its tree for every keep_at_most of planted.K_EDGES with keep_factor 0.0 /
0.01 / 0.5 / 1.0 and, at keep_at_most 7, the three ns_bound values around the most frequent best score, into buffers pre-filled with 0xFF.
Asserted: the parity bar of tests/util.py; rows equal to the plain sort of the oracle's score vector; n_rows and BELOW_NSBOUND equal to
tests/weigh_ref.py (mpmath, 100 digits); LWR within tests/util.py: LWR_RTOL of it, +0.0 where it says +0.0, never NaN; the header's fillers
beyond n_rows; the kernel the route names; the census of the reads (tests/test_weigh_planted_shapes.py asserts it without a GPU); and
the routes of one tree agree bit for bit.  Each route prints its largest relative LWR deviation from weigh_ref: a record, not a bar."""
import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib
from tests import golden_util as GU
from tests import planted as P
from tests import test_gpu_tie_order as TO
from tests import weighplant as W
from tests.util import LWR_RTOL, compare_with_oracle

pytestmark = pytest.mark.gpu

_done = {}  # (tree, route, ambiguity mode): {(keep_at_most, keep_factor, ns_bound): Placements} of a route that passed its checks


def run_route(name, route, monkeypatch, amb=None):
    sdb, odb, seq, off, _ = W.tree(name)
    if amb is not None:
        seq, _ = W.ambiguous(name, amb)
    n = len(off) - 1
    with TO.route_db(name, route, monkeypatch, sdb=sdb) as db:
        pp = ra.PlacementProcess(db)
        packed, lens, flags = pp.pack_reads_host(seq, off)
        if amb is not None:
            assert ((flags & _lib.RK_FLAG_AMBIGUOUS) != 0).all()  # every read is place_ascii_kernel's
        res = {}
        for K, kf, bound in W.calls(name, amb):
            if K in W.Ks_of(route):
                pp.ns_bound = bound
                res[K, kf, bound] = P.place_prefilled(pp, packed, n, 0, K, keep_factor=kf, amb=amb, flags=flags, seq=seq, off=off, lens=lens)
        return res


def check_route(name, route, monkeypatch, amb=None):
    assert route in (W.ROUTES[name] if amb is None else ("ascii",)) and (amb is None or amb in W.ASCII[name])
    sdb, odb, seq, off, vectors = W.tree(name)
    if amb is not None:
        seq, vectors = W.ambiguous(name, amb)
    what = f"{name} {route}" + (f" {amb}" if amb else "")
    # an ambiguity code for the last symbol breaks no census count: see tests/test_weigh_planted_shapes.py
    for K in W.Ks_of(route):
        W.assert_census(vectors, K, what)
    res = run_route(name, route, monkeypatch, amb)
    worst = 0.0
    for (K, kf, bound), got in res.items():
        call = f"{what} keep_at_most={K} keep_factor={kf} ns_bound={bound}"
        compare_with_oracle(got, W.oracle_place(name, K, kf, amb, bound), odb, seq, off, amb_mode=GU.AMB[amb or "mean"])
        if bound == float("-inf"):
            P.check_against_sorted_vectors(got, vectors, K, call)
        n_rows, lwr, below, closest = W.reference(name, amb, K, kf, bound)
        assert closest >= 1e-12, call
        assert np.array_equal(got.n_rows.astype(np.int64), n_rows), (call, np.nonzero(got.n_rows != n_rows)[0][:8])
        assert np.array_equal((got.flags & _lib.RK_FLAG_BELOW_NSBOUND) != 0, below), call
        assert not np.isnan(got.lwr).any(), (call, np.nonzero(np.isnan(got.lwr).any(axis=1))[0][:8])
        on = np.arange(K)[None, :] < n_rows[:, None]
        zero = on & (lwr == 0.0)
        assert (got.lwr.view(np.uint64)[zero] == 0).all(), (call, np.nonzero(zero & (got.lwr.view(np.uint64) != 0))[0][:8])
        some = on & (lwr != 0.0)
        rel = np.abs(got.lwr[some] - lwr[some]) / lwr[some]
        assert (rel <= LWR_RTOL).all(), (call, float(rel.max()), np.nonzero(some & (np.abs(got.lwr - lwr) > LWR_RTOL * lwr))[0][:8])
        worst = max(worst, float(rel.max()) if rel.size else 0.0)
        # beyond n_rows: the header's fillers
        assert (got.branch[~on] == 0xFFFF).all() and (got.score.view(np.uint32)[~on] == np.float32(-np.inf).view(np.uint32)).all(), call
        assert (got.lwr.view(np.uint64)[~on] == 0).all(), call
    _done[name, route, amb] = res
    print(f"{what}: largest relative LWR deviation from weigh_ref {worst:.3g}")


# ---- the dense kernels (place_packed16_kernel: the DPP row sum; place_packed_kernel in 8-, 32- and 64-lane groups: the shuffles) ----
@pytest.mark.parametrize("name,route", [(name, route) for name in ("line999", "lineaa399") for route in W.ROUTES[name]])
def test_dense_kernels(name, route, monkeypatch):
    check_route(name, route, monkeypatch)


# ---- place_ascii_kernel: the weigh stage with G == 64 ----
@pytest.mark.parametrize("amb", W.ASCII["line999"])
def test_ambiguity_kernel(amb, monkeypatch):
    check_route("line999", "ascii", monkeypatch, amb=amb)


# ---- place_packed16w_kernel, place_packed16s_kernel, place_hash64_kernel ----
@pytest.mark.parametrize("name,route", [(name, route) for name in ("line2801", "line9001") for route in W.ROUTES[name]])
def test_windowed_sorted_and_hash_kernels(name, route, monkeypatch, dev_lib):
    check_route(name, route, monkeypatch)


# ---- place_wg_kernel ----
def test_workgroup_kernel_one_pass(monkeypatch):
    check_route("linewg13301", "wg1", monkeypatch)


def test_workgroup_kernel_two_passes(monkeypatch, dev_lib):
    check_route("linewg13301", "wg2", monkeypatch)


# ---- the routes of one tree give the same result, LWR bits included ----
def check_agreement(name, monkeypatch):
    first = None
    for route in W.ROUTES[name]:
        res = _done.get((name, route, None)) or run_route(name, route, monkeypatch)
        if first is None:
            first, first_route = res, route
            continue
        for key, got in res.items():
            TO.assert_same(got, first[key], f"{name}: {route} against {first_route}, (keep_at_most, keep_factor, ns_bound) {key}")


@pytest.mark.parametrize("name", ["line999", "lineaa399"])
def test_dense_kernels_agree(name, monkeypatch):
    check_agreement(name, monkeypatch)


@pytest.mark.parametrize("name", ["line2801", "linewg13301"])
def test_kernels_agree(name, monkeypatch, dev_lib):
    check_agreement(name, monkeypatch)
