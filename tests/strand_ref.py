"""Expected values for the strand tests, none of them taken from the engine: the reverse complement of the characters in numpy
(written out here, not imported from the package), the oracle run on those characters, and the merge rule of
include/rappas_place.h (rk_merge_strands_device) restated over the oracle's result dicts.

Bit 32 means two things: RO_FLAG_TIE in the oracle's flags (exact float tie inside the top K + 1, tests/util.py), RK_FLAG_REVERSE in
the engine's.  The expected dicts therefore keep the oracle's meaning and carry the strand next to it as a boolean array `reverse`;
compare() checks the engine's bit 32 against that array, then hands the engine's result without the bit to the existing comparer."""
import numpy as np

from oracle import oracle as O
from rappas_amd import Placements
from tests.util import compare_with_oracle

REVERSE = 32

_COMP = np.arange(256, dtype=np.uint8)
for _pair in (b"AT", b"TA", b"UA", b"CG", b"GC", b"RY", b"YR", b"KM", b"MK", b"BV", b"VB", b"DH", b"HD"):
    _COMP[_pair[0]] = _pair[1]
    _COMP[_pair[0] + 32] = _pair[1] + 32


def revcomp_reads(seq, off):
    """every read reversed and complemented, same offsets (A<->T, U->A, C<->G, R<->Y, K<->M, B<->V, D<->H, case kept, the rest as is)"""
    out = np.empty_like(seq)
    o = off.astype(np.int64)
    for r in range(len(o) - 1):
        out[o[r]:o[r + 1]] = _COMP[seq[o[r]:o[r + 1]][::-1]]
    return out


def oracle_reverse(odb, seq, off, **kw):
    ref = odb.place(revcomp_reads(seq, off), off, **kw)
    ref["reverse"] = np.ones(len(off) - 1, bool)
    return ref


def merge(fwd, rev):
    """per read: the reverse result iff it has rows and forward has none or a smaller best score (float32); a tie keeps forward"""
    take = (rev["n_rows"] > 0) & ((fwd["n_rows"] == 0) | (rev["score"][:, 0] > fwd["score"][:, 0]))
    out = {}
    for key in ("n_rows", "flags"):
        out[key] = np.where(take, rev[key], fwd[key])
    for key in ("branch", "score", "lwr"):
        out[key] = np.where(take[:, None], rev[key], fwd[key])
    out["reverse"] = take
    return out


def oracle_both(odb, seq, off, **kw):
    fwd = odb.place(seq, off, **kw)
    rev = odb.place(revcomp_reads(seq, off), off, **kw)
    return merge(fwd, rev), fwd, rev


def compare(got, want, odb, seq, off, amb_mode=O.AMB_MEAN):
    """got: Placements of the engine; want: an expected dict with `reverse`.  The characters a tie is re-scored on are those of the
    strand the expected result comes from."""
    got_rev = (got.flags & REVERSE) != 0
    bad = np.nonzero(got_rev != want["reverse"])[0]
    assert not len(bad), f"RK_FLAG_REVERSE differs on {len(bad)} reads, first {bad[:5]}: got {got_rev[bad[:5]]}"
    chars = np.where(np.repeat(want["reverse"], np.diff(off.astype(np.int64))), revcomp_reads(seq, off), seq)
    plain = Placements(got.n_rows, got.branch, got.score, got.lwr, got.flags & ~np.uint32(REVERSE), {})
    return compare_with_oracle(plain, want, odb, chars, off, amb_mode=amb_mode)
