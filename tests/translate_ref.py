"""Expected values for the translated-placement tests, none of them taken from the engine or from rappas_amd.hostio: the standard
genetic code written out letter by letter, the six reading frames of a DNA read, the longest stop-free run of a frame, the 5-bit
packing of its residues, the oracle run on every frame's residues, and the merge rule of include/rappas_place.h
(rk_merge_frames_device) restated over the oracle's result dicts.  Plain Python, one read at a time.

Bit 32 means two things: RO_FLAG_TIE in the oracle's flags (tests/util.py), RK_FLAG_REVERSE in the engine's.  Expected dicts keep
the oracle's meaning and carry the frame next to it as the array `frame`; compare() checks the engine's frame bytes and its bit 32
against that array, then hands the engine's result without the bit to the existing comparer."""
import numpy as np

from oracle import oracle as O
from rappas_amd import Placements
from tests.util import compare_with_oracle

REVERSE = 32
BAD_CHAR, TOO_SHORT, AMBIGUOUS = 2, 4, 8
NONE = 0xFF

# NCBI translation table 1, codon -> one-letter residue ('*' = stop), written out by hand
CODE = {
    "TTT": "F", "TTC": "F", "TTA": "L", "TTG": "L", "TCT": "S", "TCC": "S", "TCA": "S", "TCG": "S",
    "TAT": "Y", "TAC": "Y", "TAA": "*", "TAG": "*", "TGT": "C", "TGC": "C", "TGA": "*", "TGG": "W",
    "CTT": "L", "CTC": "L", "CTA": "L", "CTG": "L", "CCT": "P", "CCC": "P", "CCA": "P", "CCG": "P",
    "CAT": "H", "CAC": "H", "CAA": "Q", "CAG": "Q", "CGT": "R", "CGC": "R", "CGA": "R", "CGG": "R",
    "ATT": "I", "ATC": "I", "ATA": "I", "ATG": "M", "ACT": "T", "ACC": "T", "ACA": "T", "ACG": "T",
    "AAT": "N", "AAC": "N", "AAA": "K", "AAG": "K", "AGT": "S", "AGC": "S", "AGA": "R", "AGG": "R",
    "GTT": "V", "GTC": "V", "GTA": "V", "GTG": "V", "GCT": "A", "GCC": "A", "GCA": "A", "GCG": "A",
    "GAT": "D", "GAC": "D", "GAA": "E", "GAG": "E", "GGT": "G", "GGC": "G", "GGA": "G", "GGG": "G",
}
AA_ORDER = "RHKDESTNQCGPAILMFWYV"  # residue states 0..19 (src/core/AAStates.java:48-197)
DNA_STATE = {"A": 0, "T": 1, "U": 1, "C": 2, "G": 3}  # src/core/DNAStatesShifted.java:182-209
STATE_DNA = "ATCG"
AMBIGUITY = set("RYSWKMBDHVN.-")
CODONS_OF = {}
for _c, _a in CODE.items():
    CODONS_OF.setdefault(_a, []).append(_c)


def dna_states(read):
    """characters (str) -> (states as the packer writes them, DNA-level flags): ambiguity codes and unsupported characters pack as
    state 0 and raise RK_FLAG_AMBIGUOUS / RK_FLAG_BAD_CHAR"""
    states, flags = [], 0
    for ch in read.upper():
        if ch in DNA_STATE:
            states.append(DNA_STATE[ch])
        elif ch in AMBIGUITY:
            states.append(0)
            flags |= AMBIGUOUS
        else:
            states.append(0)
            flags |= BAD_CHAR
    return states, flags


def frame_residues(states, f):
    """residue letters ('*' included) of reading frame f of a read given as DNA states"""
    s = states if f < 3 else [b ^ 1 for b in reversed(states)]
    o = f % 3
    return "".join(CODE["".join(STATE_DNA[b] for b in s[i:i + 3])] for i in range(o, len(s) - 2, 3))


def longest_run(residues):
    """the longest stop-free run of a residue string, the first of equal ones"""
    best = ""
    for run in residues.split("*"):
        if len(run) > len(best):
            best = run
    return best


def frames_of(read):
    """read (str of DNA characters) -> ([the six frames' records as residue strings], DNA-level flags)"""
    states, flags = dna_states(read)
    return [longest_run(frame_residues(states, f)) for f in range(6)], flags


def pack_residues(run, words):
    """5 bits a residue from bit 0 of a little-endian bit string -> `words` u32"""
    v = 0
    for i, a in enumerate(run):
        v |= AA_ORDER.index(a) << (5 * i)
    return [(v >> (32 * w)) & 0xFFFFFFFF for w in range(words)]


def pack_dna(reads, words=None):
    """list of str (plain ACGT) -> (u32 [n, words], lens u32 [n]): base i at bits [2i, 2i+2)"""
    if words is None:
        words = max(1, (max((len(r) for r in reads), default=0) * 2 + 31) // 32)
    out = np.zeros((len(reads), words), np.uint32)
    for r, read in enumerate(reads):
        v = 0
        for i, ch in enumerate(read):
            v |= DNA_STATE[ch] << (2 * i)
        for w in range(words):
            out[r, w] = (v >> (32 * w)) & 0xFFFFFFFF
    return out, np.array([len(r) for r in reads], np.uint32)


def expected_records(reads, f, aa_words):
    """frame f of every read -> (u32 [n, aa_words], lens u32 [n])"""
    runs = [frames_of(r)[0][f] for r in reads]
    return np.array([pack_residues(run, aa_words) for run in runs], np.uint32).reshape(len(reads), aa_words), np.array([len(x) for x in runs], np.uint32)


def back_translate(residues, rng):
    """a DNA string that translates to `residues` ('*' allowed), synonymous codons drawn at random"""
    return "".join(CODONS_OF[a][int(rng.integers(0, len(CODONS_OF[a])))] for a in residues)


def revcomp(dna):
    return "".join({"A": "T", "T": "A", "C": "G", "G": "C"}.get(c, c) for c in reversed(dna))


def batch(strings):
    off = np.zeros(len(strings) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings])
    return np.frombuffer("".join(strings).encode(), np.uint8).copy(), off


def merge(best, cand, f):
    """rk_merge_frames_device: the candidate (frame f) replaces the best so far iff it has rows and the best has none or a smaller
    best score as float32; a tie keeps the earlier frame"""
    take = (cand["n_rows"] > 0) & ((best["n_rows"] == 0) | (cand["score"][:, 0] > best["score"][:, 0]))
    out = {}
    for key in ("n_rows", "flags"):
        out[key] = np.where(take, cand[key], best[key])
    for key in ("branch", "score", "lwr"):
        out[key] = np.where(take[:, None], cand[key], best[key])
    out["frame"] = np.where(take, np.uint8(f), best["frame"]).astype(np.uint8)
    out["chars"] = [c if t else b for t, c, b in zip(take, cand["chars"], best["chars"])]
    return out


def oracle_translated(odb, k, reads, keep_at_most=7, keep_factor=0.01, ns_bound=float("-inf")):
    """reads: list of str.  -> (expected dict with `frame` and `chars`, [the six per-frame dicts]).  Every frame's residues go
    through the oracle as an amino-acid read of their own; a read whose DNA carries an ambiguity code or an unsupported character
    is not placed in any frame and keeps the flag (rk_place_packed_device without characters), TOO_SHORT said per frame."""
    per_read = [frames_of(r) for r in reads]
    dflags = np.array([fl for _, fl in per_read], np.uint32)
    rejected = dflags != 0
    frames = []
    for f in range(6):
        runs = [fr[f] for fr, _ in per_read]
        seq, off = batch(runs)
        ref = odb.place(seq, off, keep_at_most=keep_at_most, keep_factor=keep_factor, ns_bound=ns_bound)
        short = np.array([len(x) < k for x in runs])
        ref["n_rows"] = np.where(rejected, 0, ref["n_rows"]).astype(np.uint8)
        ref["flags"] = np.where(rejected, dflags | np.where(short, TOO_SHORT, 0).astype(np.uint32), ref["flags"]).astype(np.uint32)
        ref["branch"] = np.where(rejected[:, None], 0xFFFF, ref["branch"]).astype(np.uint16)
        ref["score"] = np.where(rejected[:, None], -np.inf, ref["score"]).astype(np.float32)
        ref["lwr"] = np.where(rejected[:, None], 0.0, ref["lwr"])
        ref["chars"] = runs
        frames.append(ref)
    best = dict(frames[0])
    best["frame"] = np.where(best["n_rows"] > 0, 0, NONE).astype(np.uint8)
    for f in range(1, 6):
        best = merge(best, frames[f], f)
    return best, frames


def compare(got, got_frame, want, odb):
    """got: Placements of the engine, got_frame: its frame bytes; want: an expected dict of oracle_translated.  The characters a tie
    is re-scored on are the residues of the frame the expected result comes from."""
    got_frame = np.asarray(got_frame, np.uint8)
    bad = np.nonzero(got_frame != want["frame"])[0]
    assert not len(bad), f"frame differs on {len(bad)} reads, first {bad[:5]}: got {got_frame[bad[:5]]} want {want['frame'][bad[:5]]}"
    assert np.array_equal(got_frame == NONE, got.n_rows == 0)
    got_rev = (got.flags & REVERSE) != 0
    want_rev = (want["frame"] >= 3) & (want["frame"] <= 5)
    bad = np.nonzero(got_rev != want_rev)[0]
    assert not len(bad), f"RK_FLAG_REVERSE differs on {len(bad)} reads, first {bad[:5]}"
    seq, off = batch(want["chars"])
    plain = Placements(got.n_rows, got.branch, got.score, got.lwr, got.flags & ~np.uint32(REVERSE), {})
    return compare_with_oracle(plain, want, odb, seq, off)
