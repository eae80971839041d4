"""The host twin of the edge statistics (rk_edgestat_host, rk_edgestat_finish_host) against the numpy restatement word
for word, the hand-derived known answers, scipy's mid-ranks and Spearman, the consequences the header states, the unusable-column
rule, no and one active sample, and the argument errors.  No GPU."""
import json
import os

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, edgestats as ES
from tests import edgestat_ref as E
from tests import kr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def words(raw, B, F):
    """(rows uint64 [B, 6 + 4F], feature rows uint64 [F, 3]) of a raw output"""
    RW = 6 + 4 * F
    return raw[:B * RW].reshape(B, RW), raw[B * RW:].reshape(F, 3)


def i64(w):
    return np.ascontiguousarray(w).view(np.int64)


def golden_case():
    with open(os.path.join(ROOT, "tests", "golden", "edgestat", "edgestat_tree6.json")) as f:
        g = json.load(f)
    B, S = g["n_branches"], len(g["mass"])
    W = 2 * B + 4
    m = np.zeros(S * W + 1, np.uint64)
    for s, mass in enumerate(g["mass"]):
        m[s * W:s * W + B] = mass
    meta = np.array([[np.nan if v is None else v for v in row] for row in g["meta"]], np.float64)
    return g, np.array(g["parent"], np.int32), m, S, meta


def check_golden(g, raw, info):
    """the known answers against a raw output: the integer words exactly, the finished values at relative 1e-12"""
    B, F = g["n_branches"], len(g["feature_names"])
    rows, feat = words(raw, B, F)
    assert int(info[0]) == g["n_active"] and int(info[1]) == g["unusable"]
    assert i64(feat[:, 2]).tolist() == g["grss"]
    for q in range(2):
        assert i64(rows[:, 3 * q + 2]).tolist() == g["rss"][q]
        for f in range(F):
            assert i64(rows[:, 6 + 4 * f + 2 * q + 1]).tolist() == [r[f] for r in g["rcross"][q]]
    r = ES.edgestat_finish(B, len(g["mass"]), raw, info, g["feature_names"])
    assert list(r.columns) == g["columns"] and r.n_active == g["n_active"] and r.unusable == 0
    for got, want in ((r.table, g["table"]), (r.feature_table, g["feature_table"])):
        want = np.array([[np.nan if v is None else v for v in row] for row in want], np.float64)
        assert (np.isnan(got) == np.isnan(want)).all()
        ok = ~np.isnan(want)
        assert (np.abs(got[ok] - want[ok]) <= 1e-12 * np.abs(want[ok])).all(), np.abs(got[ok] - want[ok]).max()
    node5 = r.table[5]
    assert node5[r.columns.index("mass_spearman_pH")] == 1.0 and node5[r.columns.index("imb_spearman_pH")] == 1.0


@pytest.mark.parametrize("B,S,F", E.shapes(ES.COUNT_MAX_SAMPLES))
def test_host_twin_equals_the_restatement_word_for_word(B, S, F):
    parent, _ = R.random_tree(B, 40 + B)
    m, meta = R.sample_buffer(B, S, 50 + S), E.metadata(S, F, 60 + S)
    raw, info = ES.edgestat_host(parent, m, S, meta)
    want, want_info = E.edgestat_ref(parent, m, S, meta)
    assert raw.shape[0] == E.out_words(B, F) == _lib.load().rk_edgestat_out_words(B, F)
    assert (info == want_info).all() and (raw == want).all(), (B, S, F, np.flatnonzero(raw != want)[:8])
    r = ES.edgestat_finish(B, S, raw, info)
    table, ftab = E.finish_ref(B, raw, info)
    assert E.same_table(r.table, table) and E.same_table(r.feature_table, ftab)
    assert r.columns == ES.edgestat_columns([str(f) for f in range(F)]) and len(r.columns) == 8 + 4 * F


def test_tie_heavy_buffers_equal_the_restatement():
    """empty, identical and huge samples; a buffer that is mostly zeros"""
    for B, S, m in ((300, 70, R.special_buffer(300, 70, 14)), (300, 140, E.sparse_buffer(300, 140, 15))):
        parent, _ = R.random_tree(B, 13)
        meta = E.metadata(S, 4, 16)
        raw, info = ES.edgestat_host(parent, m, S, meta)
        want, want_info = E.edgestat_ref(parent, m, S, meta)
        assert (info == want_info).all() and (raw == want).all()


def test_header_and_binding_share_the_constants():
    src = open(os.path.join(ROOT, "include", "rappas_place.h")).read()
    for name, value in (("MAX_SAMPLES", ES.MAX_SAMPLES), ("MAX_FEATURES", ES.MAX_FEATURES), ("COUNT_MAX_SAMPLES", ES.COUNT_MAX_SAMPLES)):
        assert f"#define RK_EDGESTAT_{name} {value}u\n" in src, name


def test_known_answers():
    g, parent, m, S, meta = golden_case()
    raw, info = ES.edgestat_host(parent, m, S, meta)
    check_golden(g, raw, info)
    want, want_info = E.edgestat_ref(parent, m, S, meta)
    assert (raw == want).all() and (info == want_info).all()


def test_rank_words_equal_scipys_mid_ranks_exactly():
    """rank2 is twice scipy's average rank: every integer word of the raw output from rankdata over the active samples"""
    stats = pytest.importorskip("scipy.stats")
    B, S, F = 60, 97, 4
    parent, _ = R.random_tree(B, 3)
    m, meta = R.special_buffer(B, S, 4), E.metadata(S, F, 5)
    raw, info = ES.edgestat_host(parent, m, S, meta)
    rows, feat = words(raw, B, F)
    P0, P1, active = E.profiles(parent, m, S)
    n = int(active.sum())
    assert n == S - 1 == info[0]
    dev = lambda v: np.rint(2 * stats.rankdata(v, method="average")).astype(np.int64) - (n + 1)
    assert (E.rank_devs(P0, active)[:, active] == np.array([dev(r) for r in P0[:, active]])).all()
    gd = [dev(meta[f][active]) for f in range(F)]
    assert i64(feat[:, 2]).tolist() == [int((d * d).sum()) for d in gd]
    for q, P in enumerate((P0, P1)):
        d = np.array([dev(r) for r in P[:, active]])
        assert (i64(rows[:, 3 * q + 2]) == (d * d).sum(axis=1)).all()
        for f in range(F):
            assert (i64(rows[:, 6 + 4 * f + 2 * q + 1]) == (d * gd[f]).sum(axis=1)).all()


@pytest.mark.parametrize("S", [9, 64, 130])
def test_spearman_equals_scipys(S):
    """ours is exact integers and four roundings, scipy's a Pearson of the ranks in floating point, O(S * 2^-53): absolute 1e-12, on the
    rows with at least three distinct values"""
    stats = pytest.importorskip("scipy.stats")
    B, F = 40, 3
    parent, _ = R.random_tree(B, 7)
    m, meta = R.sample_buffer(B, S, 8), E.metadata(S, F, 9)
    r = ES.edgestat_finish(B, S, *ES.edgestat_host(parent, m, S, meta))
    P0, P1, _ = E.profiles(parent, m, S)
    checked = 0
    for q, P in enumerate((P0, P1)):
        for x in range(B):
            if len(np.unique(P[x])) < 3:
                continue
            for f in range(F):
                want = stats.spearmanr(P[x], meta[f])[0]
                assert abs(r.table[x, 8 + 4 * f + 2 * q + 1] - want) <= 1e-12, (q, x, f)
                checked += 1
    assert checked > B


def test_the_stated_consequences_hold_exactly():
    B, S, F = 50, 33, 2
    parent, _ = R.random_tree(B, 21)
    m = R.sample_buffer(B, S, 22, fill=1.0)
    rng = np.random.default_rng(23)
    meta = np.stack([rng.permutation(S) / 7.0 - 2.0, rng.integers(0, 5, S) - 2.0])
    raw, info = ES.edgestat_host(parent, m, S, meta)
    rows, feat = words(raw, B, F)
    ints = lambda rows, feat: (i64(rows[:, 2::3][:, :2]).copy(), i64(rows[:, 7::2]).copy(), i64(feat[:, 2]).copy())
    base = ints(rows, feat)
    # a strictly increasing transform of the columns: cubed, exponentiated
    for g in (meta ** 3, np.exp(meta)):
        r2, f2 = words(ES.edgestat_host(parent, m, S, g)[0], B, F)
        assert all((a == b).all() for a, b in zip(base, ints(r2, f2)))
    # one permutation of the samples of buffer and metadata
    perm = rng.permutation(S)
    W = 2 * B + 4
    mp = m.copy()
    for s in range(S):
        mp[s * W:(s + 1) * W] = m[perm[s] * W:(perm[s] + 1) * W]
    r2, f2 = words(ES.edgestat_host(parent, mp, S, meta[:, perm])[0], B, F)
    assert all((a == b).all() for a, b in zip(base, ints(r2, f2)))
    # a row strictly increasing / decreasing with a column: Spearman is exactly +-1.0; the root's row is all ties: NaN
    P0, _, _ = E.profiles(parent, m, S)
    root = int(np.flatnonzero(np.asarray(parent) < 0)[0])
    x = next(x for x in range(B) if x != root and len(np.unique(P0[x])) == S)
    planted = np.stack([P0[x] * 3.0 + 1.0, -P0[x]])
    raw, info = ES.edgestat_host(parent, m, S, planted)
    rows, feat = words(raw, B, 2)
    assert i64(rows[x, 7]) == i64(rows[x, 2]) == i64(feat[0, 2]) and i64(rows[x, 11]) == -i64(rows[x, 2])
    r = ES.edgestat_finish(B, S, raw, info, ("up", "down"))
    assert r.table[x, r.columns.index("mass_spearman_up")] == 1.0 and r.table[x, r.columns.index("mass_spearman_down")] == -1.0
    assert np.isnan(r.table[root, 8:]).all() and (R.bits(r.table[root, [0, 1, 2, 5, 6, 7]]) == 0).all()


def test_unusable_columns_write_fillers_and_set_the_mask():
    B, S = 30, 12
    parent, _ = R.random_tree(B, 31)
    m = R.special_buffer(B, S, 32)  # sample 1 is empty
    meta = E.metadata(S, 3, 33)
    good = ES.edgestat_host(parent, m, S, meta)
    for bad_value in (np.nan, np.inf, -np.inf):
        quiet = meta.copy()
        quiet[1, 1] = bad_value  # not finite in the inactive sample only: the column stays usable, the value is never read
        raw, info = ES.edgestat_host(parent, m, S, quiet)
        assert info[1] == 0 and (raw == good[0]).all()
        loud = meta.copy()
        loud[1, 4] = bad_value
        raw, info = ES.edgestat_host(parent, m, S, loud)
        want, want_info = E.edgestat_ref(parent, m, S, loud)
        assert info[1] == 2 and (info == want_info).all() and (raw == want).all()
        rows, feat = words(raw, B, 3)
        assert feat[1].tolist() == [E.NAN_BITS, E.NAN_BITS, 0]
        assert (rows[:, [10, 12]] == E.NAN_BITS).all() and (rows[:, [11, 13]] == 0).all()
        keep = [c for c in range(rows.shape[1]) if c not in (10, 11, 12, 13)]
        assert (rows[:, keep] == words(good[0], B, 3)[0][:, keep]).all() and (feat[[0, 2]] == words(good[0], B, 3)[1][[0, 2]]).all()
        r = ES.edgestat_finish(B, S, raw, info)
        assert r.unusable == 2 and np.isnan(r.table[:, 12:16]).all() and np.isnan(r.feature_table[1]).all() and not np.isnan(r.feature_table[[0, 2]]).any()


def test_no_and_one_active_sample():
    B = 9
    parent, _ = R.random_tree(B, 41)
    W = 2 * B + 4
    for S in (1, 3):
        m = np.zeros(S * W + 1, np.uint64)
        meta = E.metadata(S, 2, 42)
        raw, info = ES.edgestat_host(parent, m, S, meta)
        assert info.tolist() == [0, 0] and not raw.any()
        r = ES.edgestat_finish(B, S, raw, info)
        assert np.isnan(r.table).all() and np.isnan(r.feature_table).all() and r.n_active == 0
        m[(S - 1) * W + 2] = 5  # one sample with mass: every row is constant
        m[(S - 1) * W + 4] = 7
        raw, info = ES.edgestat_host(parent, m, S, meta)
        want, _ = E.edgestat_ref(parent, m, S, meta)
        assert info.tolist() == [1, 0] and (raw == want).all()
        rows, feat = words(raw, B, 2)
        assert not rows[:, [1, 2, 4, 5]].any() and not rows[:, 6:].any() and not feat[:, 1:].any()
        r = ES.edgestat_finish(B, S, raw, info)
        assert np.isnan(r.table[:, 8:]).all() and (r.table[:, [1, 2, 6, 7]] == 0).all() and (r.feature_table[:, 0] == meta[:, S - 1]).all()


def test_argument_errors_without_a_device():
    lib = _lib.load()
    B, S = 9, 4
    parent, _ = R.random_tree(B, 51)
    m, meta = R.sample_buffer(B, S, 52), E.metadata(S, 2, 53)
    raw, info = np.full(E.out_words(B, 2), 0x6B6B, np.uint64), np.full(2, 0x6B6B, np.uint32)
    p = lambda a: a.ctypes.data

    def call(B=B, parent=p(parent), S=S, masses=p(m), F=2, meta=p(meta), raw=p(raw), info=p(info)):
        return lib.rk_edgestat_host(B, parent, S, masses, F, meta, raw, info, 1)

    for kw in (dict(S=0), dict(S=4097), dict(F=9), dict(meta=None), dict(raw=None), dict(info=None), dict(masses=None), dict(parent=None), dict(B=0)):
        assert call(**kw) == _lib.RK_ERR_INVALID, kw
        assert b"rk_edgestat_host" in lib.rk_last_error()
    assert (raw == 0x6B6B).all() and (info == 0x6B6B).all()
    assert call(F=0, meta=None) == _lib.RK_OK
    assert lib.rk_edgestat_out_words(0, 0) == 0 and lib.rk_edgestat_out_words(65536, 0) == 0 and lib.rk_edgestat_out_words(5, 9) == 0
    assert lib.rk_edgestat_out_words(65535, 8) == 65535 * 38 + 24
    assert lib.rk_edgestat_work_bytes(None, 4, 0) == 0 and b"null tree" in lib.rk_last_error()
    table, ftab = np.zeros((B, 16)), np.zeros((2, 2))
    good = ES.edgestat_host(parent, m, S, meta)
    fin = lambda B=B, S=S, F=2, raw=p(good[0]), info=p(good[1]), table=p(table), ftab=p(ftab): lib.rk_edgestat_finish_host(B, S, F, raw, info, table, ftab)
    for kw in (dict(B=0), dict(S=0), dict(S=4097), dict(F=9), dict(raw=None), dict(info=None), dict(table=None), dict(ftab=None)):
        assert fin(**kw) == _lib.RK_ERR_INVALID, kw
    assert fin() == _lib.RK_OK
    with pytest.raises(ValueError):
        ES.edgestat_host(parent, m, S, meta[:, :3])
    with pytest.raises(ValueError):
        ES.edgestat_finish(B, S, good[0][:-1], good[1])
    with pytest.raises(ra.RkError):
        ES.edgestat_host(parent, m, S, np.zeros((9, S)))
