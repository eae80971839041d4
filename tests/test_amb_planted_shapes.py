"""No GPU: the planted ambiguity reads of tests/ambplant.py hold every shape place_ascii_kernel's accumulate paths branch on -- the census
of CLASSES, at least four sites (or reads) a class --, every entry of every alternative row length is among the rows the oracle reports
for some read, no read has a tie and no score is infinite, and the two references (tests/pyref.py, the C oracle) agree bit for bit on
every read's whole score vector in every ambiguity mode.  tests/test_gpu_amb_planted.py runs the same reads on the device."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import ambplant as A
from tests import golden_util as GU
from tests import pyref
from tests.util import LWR_RTOL

NAMES = sorted(A.FAMILIES)
FLAGS = {"placed": O.RO_FLAG_PLACED, "bad_char": O.RO_FLAG_BAD_CHAR, "too_short": O.RO_FLAG_TOO_SHORT, "ambiguous": O.RO_FLAG_AMBIGUOUS,
         "below_nsbound": O.RO_FLAG_BELOW_NSBOUND}


def test_the_families_are_the_ones_with_classes():
    assert set(A.FAMILIES) == set(A.CLASSES)


@pytest.mark.parametrize("name", NAMES)
def test_every_class_holds_four_sites(name):
    f = A.family(name)
    seen = dict(f.census)
    if len(f.borders) and f.s_win < f.nb:
        seen.update(A.window_census(f, {K: A.oracle_place(name, K, "mean") for K in A.KS}))
    few = {c: seen.get(c, 0) for c in A.CLASSES[name] if seen.get(c, 0) < 4}
    assert not few, f"{name}: classes with fewer than four sites {few}"


def test_the_geometry_the_census_counts_with():
    """dna99, aa399, dna16 and dna20 in one chunk; dna_chunks and dna_indexed in two chunk passes; dna_windows in windows, one chunk each"""
    for name in ("dna99", "aa399", "dna16", "dna20"):
        f = A.family(name)
        assert f.chunk >= f.nb and f.s_win >= f.nb and not f.borders
    for name in ("dna_chunks", "dna_indexed"):
        f = A.family(name)
        assert f.s_win >= f.nb and f.chunk < f.nb <= 2 * f.chunk and f.borders == [f.chunk]
    f = A.family("dna_chunks")
    assert f.nb <= 8192 and A.amb_geometry(f.nb - 1)[0] > f.nb - 1 - 64  # (a branch fewer leaves the second pass fewer than 64)
    f = A.family("dna_windows")
    assert f.s_win < f.nb and f.chunk >= f.s_win and len(f.borders) >= 3


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("name", NAMES)
def test_every_entry_of_every_row_length_is_reported_somewhere(name, mode):
    f = A.family(name)
    needed, seen = A.entries_seen(f, A.oracle_place(name, 16, mode))
    lengths = {c for c, _, _ in needed}
    assert lengths >= set(A.LENGTHS), lengths
    lost = sorted(needed - seen)
    assert not lost, f"{name} {mode}: {len(lost)} of {len(needed)} (length, alternative, entry) never reported: {lost[:20]}"


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("name", NAMES)
def test_no_ties_and_no_infinities(name, mode):
    f = A.family(name)
    odb = A.oracle_db(name)
    for K in A.KS:
        assert int(((A.oracle_place(name, K, mode)["flags"] & O.RO_FLAG_TIE) != 0).sum()) == 0, (name, mode, K)
    bad = 0
    for r in range(len(f.reads)):
        S, touched, _ = odb.score_vector(f.reads[r].encode(), GU.AMB[mode])
        bad += int((~np.isfinite(S[touched])).sum())
    assert bad == 0


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("name", NAMES)
def test_the_two_references_agree(name, mode):
    """pyref.place_read and the C oracle: the whole score vector bit for bit, the touched set, the flags, and the reported rows"""
    f = A.family(name)
    odb = A.oracle_db(name)
    ref = {K: A.oracle_place(name, K, mode) for K in A.KS}
    n_code = 0
    for r, read in enumerate(f.reads):
        S, touched, _ = odb.score_vector(read.encode(), GU.AMB[mode])
        for K in A.KS:
            py = pyref.place_read(f.pydb, read, keep_at_most=K, keep_factor=A.keep_factor(K), amb_mode=mode)
            if K == A.KS[0]:
                n_code += "ambiguous" in py["flags"]
                assert set(py["L"]) == set(touched.tolist()), (name, mode, r)
                got = np.array([py["S"][b] for b in sorted(py["L"])], np.float32)
                assert np.array_equal(got.view(np.uint32), S[sorted(py["L"])].view(np.uint32)), (name, mode, r)
            o = ref[K]
            assert sum(FLAGS[x] for x in py["flags"]) == int(o["flags"][r]) & ~O.RO_FLAG_TIE, (name, mode, r, K, py["flags"], o["flags"][r])
            n = int(o["n_rows"][r])
            assert n == len(py["rows"]), (name, mode, r, K)
            assert [b for b, _, _ in py["rows"]] == o["branch"][r, :n].tolist(), (name, mode, r, K)
            assert np.array_equal(np.array([s for _, s, _ in py["rows"]], np.float32).view(np.uint32), o["score"][r, :n].view(np.uint32)), (name, mode, r, K)
            assert np.allclose([w for _, _, w in py["rows"]], o["lwr"][r, :n], rtol=LWR_RTOL, atol=0.0), (name, mode, r, K)
    assert n_code == f.n_with_code == int(((ref[1]["flags"] & O.RO_FLAG_AMBIGUOUS) != 0).sum())
