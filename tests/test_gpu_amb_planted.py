"""GPU (-m gpu): place_ascii_kernel's accumulate paths on the planted alternative rows of tests/ambplant.py -- the 16-lane and the 64-lane
form of amb_position, the general form with its chunk passes, two codes in one k-mer, tree windows with the final merge, the flush of
the pending list at its cap and at a code, pending rows of more than 64 entries, codes at the ends of the 64-position blocks.  The
census of those shapes, the two references' agreement and the absence of ties are asserted without a GPU in
tests/test_amb_planted_shapes.py; here every family runs in mean, max and skip with keep_at_most 1, 7 and 16 (16 with keep factor 0)
through result tensors pre-filled with 0xFF, against the oracle at the bar of tests/util.py (flags, n_rows and branches equal, scores
bit-equal, LWR within LWR_RTOL).  Also: the host path and its `ambiguous` counter, and that a read's rows do not depend on the batch it
comes in (the wave serves the flagged reads of 64 in turn): the same reads in reversed order, and one-to-one between code-free reads."""
import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib
from tests import ambplant as A
from tests import golden_util as GU
from tests import planted as P
from tests.util import compare_with_oracle

pytestmark = pytest.mark.gpu

TABLE = {"auto": ra.RK_TABLE_AUTO, "direct8": ra.RK_TABLE_DIRECT8, "hash": ra.RK_TABLE_HASH}
CASES = [("dna99", t) for t in A.TABLES_OF_DNA99] + [(name, spec["table"]) for name, spec in sorted(A.FAMILIES.items()) if name != "dna99"]
KNOBS = ["RK_NO_WSTREAM", "RK_NO_HASH", "RK_WSTREAM_ALWAYS", "RK_HASH_ALWAYS", "RK_HASH_SMALL_TABLE", "RK_HASH_KEY_SLACK", "RK_WG_PASSES",
         "RK_RETILE_MIN_READS", "RK_WINDOW_ALWAYS", "RK_NO_WINDOW", "RK_HASH_BIG_TABLE"]  # developer knobs: none holds here
_OPEN = {}


@pytest.fixture(scope="module", autouse=True)
def _databases():
    yield
    for db, _ in _OPEN.values():
        db.close()
    _OPEN.clear()


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)


def opened(name, table):
    """(database, placement process) of a family in a table mode, made once for the module"""
    if (name, table) not in _OPEN:
        f = A.family(name)
        db = ra.PhyloKmerDB.from_synth(f.sdb, table_mode=TABLE[table], device=0)
        kn = db.kernel_name()
        # the image the census counted with: place_wg_kernel serves the indexed (large-tree) image alone
        assert kn.startswith("place_wg_kernel<") == f.indexed or name == "dna_windows", (name, table, kn)
        if table != "auto":
            assert {"direct8": ",DIRECT8,", "hash": ",HASH,"}[table] in kn or not kn.startswith("place_packed_kernel<"), (name, table, kn)
        _OPEN[name, table] = (db, ra.PlacementProcess(db))
    return _OPEN[name, table]


def place(name, table, mode, K, seq=None, off=None):
    f = A.family(name)
    seq, off = (f.seq, f.off) if seq is None else (seq, off)
    _, pp = opened(name, table)
    packed, lens, flags = pp.pack_reads_host(seq, off)
    return P.place_prefilled(pp, packed, len(off) - 1, 0, K, keep_factor=A.keep_factor(K), amb=mode, flags=flags, seq=seq, off=off, lens=lens)


def rows_of(got, r):
    n = int(got.n_rows[r])
    return (n, int(got.flags[r]), got.branch[r, :n].tolist(), got.score[r, :n].view(np.uint32).tolist(), got.lwr[r, :n].view(np.uint64).tolist())


@pytest.mark.parametrize("K", A.KS)
@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("name,table", CASES)
def test_planted_alternative_rows(name, table, mode, K):
    f = A.family(name)
    got = place(name, table, mode, K)
    st = compare_with_oracle(got, A.oracle_place(name, K, mode), A.oracle_db(name), f.seq, f.off, amb_mode=GU.AMB[mode])
    assert st["ties"] == 0
    assert int(((got.flags & _lib.RK_FLAG_AMBIGUOUS) != 0).sum()) == f.n_with_code == len(f.reads)


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("name,table", [c for c in CASES if c[1] == A.FAMILIES[c[0]]["table"]])
def test_host_path_and_its_counter(name, table, mode):
    f = A.family(name)
    _, pp = opened(name, table)
    got = pp.processQueries(f.seq, f.off, keepAtMost=7, keepFactor=A.keep_factor(7), treatAmbiguities=mode != "skip", treatAmbiguitiesWithMax=mode == "max")
    compare_with_oracle(got, A.oracle_place(name, 7, mode), A.oracle_db(name), f.seq, f.off, amb_mode=GU.AMB[mode])
    assert got.counters["ambiguous"] == f.n_with_code


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("name,table", CASES)
def test_rows_do_not_depend_on_the_batch(name, table, mode):
    """the planted reads in reversed order, and one-to-one between code-free reads (which the packed kernel places): every planted read's
    rows are those of the plain batch, bit for bit; the mixed batch as a whole meets the oracle's"""
    f = A.family(name)
    n, K = len(f.reads), 16
    first = place(name, table, mode, K)
    back = place(name, table, mode, K, *A.reads_array(f.reads[::-1]))
    differ = [r for r in range(n) if rows_of(first, r) != rows_of(back, n - 1 - r)]
    assert not differ, (name, table, mode, "reversed", differ[:8])
    mixed = [x for pair in zip(f.reads, A.code_free(f, n)) for x in pair]
    seq, off = A.reads_array(mixed)
    got = place(name, table, mode, K, seq, off)
    differ = [r for r in range(n) if rows_of(first, r) != rows_of(got, 2 * r)]
    assert not differ, (name, table, mode, "one-to-one", differ[:8])
    assert int(((got.flags & _lib.RK_FLAG_AMBIGUOUS) != 0).sum()) == n
    odb = A.oracle_db(name)
    ref = odb.place(seq, off, keep_at_most=K, keep_factor=A.keep_factor(K), amb_mode=GU.AMB[mode])
    compare_with_oracle(got, ref, odb, seq, off, amb_mode=GU.AMB[mode])
