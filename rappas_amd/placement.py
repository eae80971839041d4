"""Host-side mirror of the reference's placement interface, over the C ABI (include/rappas_place.h).

Names follow the reference: `PhyloKmerDB` stands where `session.hash` (CustomHash_v4_FastUtil81) plus the session
scalars stand (src/main_v2/SessionNext_v2.java:43-66); `PlacementProcess.processQueries` takes the arguments of
src/core/algos/PlacementProcess.java:471-483 that reach the hot path (keepAtMost, keepFactor, treatAmbiguities,
treatAmbiguitiesWithMax) and returns, per read, what :974-1025 turns into jplace rows.
No compute happens in Python and nothing here falls back to a CPU implementation.

Every public call is a written-out def over a few shared steps: the handle base (_Handle), the output allocator with its one
numpy -> torch dtype map (_alloc), the rows of a result set (_rows), the reads of a packed call (_packed_reads), and, for the five
sample-level analyses, one description a call (_SAMPLE_CALLS) run by one runner a form (_sample_host, EdgeTree._sample_device,
EdgeTree._sample_batch).
"""
import collections
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import (RK_ALPHABET_AA, RK_ALPHABET_DNA, RK_AMB_MAX, RK_AMB_MEAN, RK_AMB_SKIP, RK_TABLE_AUTO,
                   RK_TABLE_DIRECT, RK_TABLE_DIRECT8, RK_TABLE_HASH, rk_counters, rk_db_desc, rk_db_info, rk_params, rk_result)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dp(t):
    return None if t is None else t.data_ptr()


def _torch():
    """torch, imported when a device form first needs it: the package and its host forms work without"""
    import torch
    return torch


def _stream(dev, stream):
    """the stream argument of a device call: `stream` (a raw handle), or the current stream of `dev`"""
    return C.c_void_p(stream if stream is not None else _torch().cuda.current_stream(dev).cuda_stream)


# numpy -> torch, by the dtype's kind and size: torch tensors carry unsigned words as the signed type of the same width
_TORCH_DTYPE = {"u1": "uint8", "u2": "int16", "u4": "int32", "u8": "int64", "f4": "float32", "f8": "float64"}


def _alloc(shape, dtype, dev=None):
    """an output array of a call: zeroed numpy on the host, or (dev: a torch device) an uninitialised tensor of the matching torch
    dtype there; a structured dtype becomes uint8 [..., itemsize] on the device"""
    if dev is None:
        return np.zeros(shape, dtype)
    torch, dtype = _torch(), np.dtype(dtype)
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    if dtype.names:
        return torch.empty(shape + (dtype.itemsize,), dtype=torch.uint8, device=dev)
    return torch.empty(shape, dtype=getattr(torch, _TORCH_DTYPE[dtype.str[1:]]), device=dev)


def _grow(owner, attr, dev, need):
    """the device workspace owner.<attr>, grow-only (the old block goes back to its stream's allocator in stream order)"""
    work = getattr(owner, attr, None)
    if work is None or work.device != dev or work.numel() < need:
        work = _alloc(max(need, 256), np.uint8, dev)
        setattr(owner, attr, work)
    return work


def _or_error(lib, need, code=_lib.RK_ERR_INVALID):
    """the answer of a _work_bytes call -- or, when it is 0, the call's error: an RkError of `code` with the text the call left"""
    if not need:
        raise _lib.RkError(code, lib.rk_last_error().decode("utf-8", "replace"))
    return int(need)


def _strand(strand):
    """"forward" | "reverse" | "both" (or the drivers' fwd / rev, or an RK_STRAND_* value) -> RK_STRAND_*"""
    if isinstance(strand, str):
        if strand not in _lib.STRANDS:
            raise ValueError(f"strand must be 'forward', 'reverse' or 'both', not {strand!r}")
        return _lib.STRANDS[strand]
    return int(strand)


def _reads(seq, seq_off):
    """(characters u8, offsets u64 [n + 1], n): the contiguous arrays the C ABI reads"""
    seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    return np.ascontiguousarray(seq, dtype=np.uint8), seq_off, seq_off.shape[0] - 1


def _packed_reads(packed, lens, fixed_len, flags, seq, seq_off):
    """the reads of a *Packed* call: (n, the arguments n .. seq_off as the C ABI takes them, the contiguous arrays those point into)"""
    keep = [np.ascontiguousarray(packed, dtype=np.uint32)] + [None if a is None else np.ascontiguousarray(a, dtype=dt) for a, dt in (
        (lens, np.uint32), (flags, np.uint32), (seq, np.uint8), (seq_off, np.uint64))]
    n, wpr = keep[0].shape
    at = [_ptr(a) for a in keep]
    return n, (n, at[0], wpr, at[1], fixed_len, at[2], at[3], at[4]), keep


def _packed_out(n, wpr, dev=None):
    """(packed u32 [n, wpr], lens u32 [n], flags u32 [n]): what a read packer writes"""
    return _alloc((n, wpr), np.uint32, dev), _alloc(n, np.uint32, dev), _alloc(n, np.uint32, dev)


def _db_desc(alphabet, k, n_branches, thr_log10, thr, key_codes, row_offsets, branch_ids, scores, table_mode, convert_uo, device=0):
    """(rk_db_desc, the contiguous CSR arrays it points into)"""
    csr = [np.ascontiguousarray(a, dtype=dt) for a, dt in ((key_codes, np.uint64), (row_offsets, np.uint64), (branch_ids, np.uint16), (scores, np.float32))]
    return rk_db_desc(alphabet, int(bool(convert_uo)), k, n_branches, float(thr_log10), float(thr), csr[0].shape[0], *map(_ptr, csr), device, table_mode), csr


# the arrays of a result set, in the order of rk_result: (name, per read K entries or one, dtype)
_RESULT = (("n_rows", False, np.uint8), ("branch", True, np.uint16), ("score", True, np.float32), ("lwr", True, np.float64), ("flags", False, np.uint32))


def _host_out(n, K, out):
    """`out`, or new host arrays for n reads of K rows"""
    return out if out is not None else Placements(*(_alloc((n, K) if rows else n, dt) for _, rows, dt in _RESULT), {})


def _device_out(n, K, dev, out, frame=False):
    """`out`, or a new dict of device tensors for n reads of K rows; frame: with the "frame" bytes of place_translated"""
    if out is None:
        out = {f: _alloc((n, K) if rows else n, dt, dev) for f, rows, dt in _RESULT}
    if frame and "frame" not in out:
        out["frame"] = _alloc(n, np.uint8, dev)
    return out


def _result(out):
    """rk_result over a Placements (host arrays) or over a dict of device tensors"""
    if isinstance(out, dict):
        return rk_result(*(out[f].data_ptr() for f, _, _ in _RESULT))
    return rk_result(*(_ptr(getattr(out, f)) for f, _, _ in _RESULT))


def _rows(rows, K=None):
    """the three arrays of a result set that a sum reads -> (rk_result with score and flags null, n, K, device or None).  `rows`: a
    dict of device tensors, or anything with n_rows u8 [n], branch u16 [n, K] and lwr f64 [n, K] on the host, which are made contiguous
    and checked against each other.  K None: from the shape of branch."""
    if isinstance(rows, dict):
        n_rows, branch, lwr = rows["n_rows"], rows["branch"], rows["lwr"]
        n, K = (n_rows.numel(), K) if K is not None else branch.shape
        return rk_result(n_rows.data_ptr(), branch.data_ptr(), None, lwr.data_ptr(), None), n, K, branch.device
    n_rows, branch, lwr = (np.ascontiguousarray(getattr(rows, f), dtype=dt) for f, dt in (("n_rows", np.uint8), ("branch", np.uint16), ("lwr", np.float64)))
    if K is not None:
        n, what = n_rows.size, f" = {n_rows.size} x {K}"
    else:
        n, what = n_rows.shape[0], ""
        K = branch.shape[1] if branch.ndim == 2 else (branch.size // n if n else 1)
    if branch.size != n * K or lwr.size != n * K:
        raise ValueError(f"branch and lwr must hold n_reads x K{what} rows")
    res = rk_result(_ptr(n_rows), _ptr(branch), None, _ptr(lwr), None)
    res.keep = (n_rows, branch, lwr)  # the arrays live as long as the addresses
    return res, n, K, None


def _counters(ct):
    return {f: getattr(ct, f) for f, _ in rk_counters._fields_}


@dataclass
class Placements:
    """Rows best -> worse per read; unused rows are branch 0xFFFF / score -inf / lwr 0."""
    n_rows: np.ndarray   # u8  [n]
    branch: np.ndarray   # u16 [n, K]
    score: np.ndarray    # f32 [n, K]
    lwr: np.ndarray      # f64 [n, K]
    flags: np.ndarray    # u32 [n]
    counters: dict
    frame: np.ndarray = None  # u8 [n], processQueriesTranslated only: the reading frame of the result (0..5, 0xFF = none)


def pack_reads(alphabet, k, seq, seq_off, words_per_read=None, convert_uo=False, threads=0):
    """rk_pack_reads: the host-side read packer without a database handle (no GPU): ASCII reads -> (packed u32 [n, wpr], lens u32 [n],
    flags u32 [n]), the records the device packer produces (AmbigSequenceKnife.java:103-130 char -> state)."""
    lib = _lib.load()
    seq, seq_off, n = _reads(seq, seq_off)
    bits = 2 if alphabet == _lib.RK_ALPHABET_DNA else 5
    if words_per_read is None:
        max_len = int((seq_off[1:] - seq_off[:-1]).max()) if n else 0
        words_per_read = max(1, (max_len * bits + 31) // 32)
    packed, lens, flags = _packed_out(n, words_per_read)
    _lib.check(lib.rk_pack_reads(alphabet, int(bool(convert_uo)), k, n, _ptr(seq), _ptr(seq_off), words_per_read, _ptr(packed), _ptr(lens), _ptr(flags), threads))
    return packed, lens, flags


def translated_words(dna_len):
    """32-bit words of the amino-acid record of one reading frame of a DNA read of dna_len bases (5 bits a residue)"""
    return max(1, (dna_len // 3 * 5 + 31) // 32)


def translate_packed_host(dna, frame, lens=None, fixed_len=0, aa_words=None):
    """rk_translate_packed_host (no GPU): reading frame `frame` (0..2 the read as given from base 0, 1, 2; 3..5 its reverse complement)
    of 2-bit DNA records u32 [n, dna_words] -> (aa u32 [n, aa_words], aa_lens u32 [n]): per read the longest stop-free run of
    residues under the standard genetic code, 5 bits a residue -- the records the device kernel writes."""
    lib = _lib.load()
    dna = np.ascontiguousarray(dna, dtype=np.uint32)
    n, dna_words = dna.shape
    if lens is not None:
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
    if aa_words is None:
        aa_words = translated_words(dna_words * 16 if lens is not None else fixed_len)
    aa, aa_lens = _alloc((n, aa_words), np.uint32), _alloc(n, np.uint32)
    _lib.check(lib.rk_translate_packed_host(frame, n, _ptr(dna), dna_words, _ptr(lens), fixed_len, _ptr(aa), aa_words, _ptr(aa_lens)))
    return aa, aa_lens


def masses_words(n_branches):
    """rk_masses_words: 64-bit words of a mass buffer of a tree of n_branches (2 * B + 4; 0 for 0 or more than 65535 branches)"""
    return int(_lib.load().rk_masses_words(n_branches))


def _host_masses(words, masses):
    """the mass buffer of a host call: made and zeroed when None, else checked -- a contiguous uint64 array of `words` words"""
    if masses is None:
        return np.zeros(words, np.uint64)
    if masses.dtype != np.uint64 or masses.shape != (words,) or not masses.flags.c_contiguous:
        raise ValueError(f"masses must be a contiguous uint64 array of {words} words")
    return masses


def _device_masses(words, masses, dev, stream):
    """the mass buffer of a device call: an int64 tensor of `words` words on `dev`, made and zeroed on the call's stream when None"""
    torch = _torch()
    if masses is None:
        masses = _alloc(words, np.uint64, dev)
        if stream is not None:
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)):
                masses.zero_()
        else:
            masses.zero_()
    elif masses.dtype != torch.int64 or masses.numel() != words or not masses.is_contiguous() or masses.device != dev:
        raise ValueError(f"masses must be a contiguous int64 tensor of {words} words on {dev}")
    return masses


def _i32_tensor(t, n, dev, what):
    """None, or `t` checked: a contiguous int32 tensor of n words on `dev`"""
    if t is not None and (t.dtype != _torch().int32 or t.numel() != n or not t.is_contiguous() or t.device != dev):
        raise ValueError(f"{what} must be a contiguous int32 tensor of {n} words on {dev}")
    return t


def accumulate_masses_host(n_branches, placements, weights=None, masses=None, threads=0):
    """rk_masses_accumulate_host (no GPU): the per-branch LWR sums of a result set (`placements`: a Placements, or anything with
    n_rows u8 [n], branch u16 [n, K] and lwr f64 [n, K]) ADDED into `masses`, a uint64 array of masses_words(n_branches) -- mass_q30[B] |
    best[B] | four totals (include/rappas_place.h) -- made and zeroed when None.  weights: uint32 [n], one per read (None = 1 each)."""
    lib = _lib.load()
    words = masses_words(n_branches)
    if not words:
        raise ValueError(f"n_branches={n_branches} must be in 1..65535")
    res, n, K, _ = _rows(placements)
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.uint32)
        if weights.shape != (n,):
            raise ValueError("weights must hold one uint32 per read")
    masses = _host_masses(words, masses)
    _lib.check(lib.rk_masses_accumulate_host(n_branches, K, n, C.byref(res), _ptr(weights), _ptr(masses), threads))
    return masses


def masses_samples_words(n_branches, n_samples):
    """rk_masses_samples_words: 64-bit words of a sample mass buffer, n_samples * masses_words(n_branches) + 1 (0 on a bad argument:
    n_branches or n_samples outside 1..65535, or more than 2^29 words)"""
    return int(_lib.load().rk_masses_samples_words(n_branches, n_samples))


def _u32_list(a, n, what):
    """None, or `a` as a contiguous uint32 array of n words"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if a.shape != (n,):
        raise ValueError(f"{what} must hold {n} uint32 words")
    return a


def _samples_buffer(n_branches, n_samples, masses):
    words = masses_samples_words(n_branches, n_samples)
    if not words:
        raise ValueError(f"n_samples={n_samples} on {n_branches} branches: both in 1..65535 and at most 2^29 words")
    return _host_masses(words, masses)


def accumulate_masses_samples_host(n_branches, placements, n_samples, member_sample, member_read=None, member_weight=None, masses=None, threads=0):
    """rk_masses_accumulate_samples_host (no GPU): one mass buffer per sample from the membership entries (member_read[i],
    member_sample[i], member_weight[i]) over a result set, ADDED into `masses`, a uint64 array of masses_samples_words(n_branches,
    n_samples) -- n_samples buffers of masses_words(n_branches) words and the count of entries skipped for a sample or read out of
    range -- made and zeroed when None.  member_read None: entry i is read i; member_weight None: 1."""
    lib = _lib.load()
    masses = _samples_buffer(n_branches, n_samples, masses)
    res, n, K, _ = _rows(placements)
    member_sample = np.ascontiguousarray(member_sample, dtype=np.uint32)
    m = member_sample.shape[0]
    member_read, member_weight = _u32_list(member_read, m, "member_read"), _u32_list(member_weight, m, "member_weight")
    _lib.check(lib.rk_masses_accumulate_samples_host(n_branches, K, n, C.byref(res), n_samples, m, _ptr(member_read), _ptr(member_sample),
                                                     _ptr(member_weight), _ptr(masses), threads))
    return masses


def host_alloc(shape, dtype):
    """numpy array in page-locked host memory (rk_host_alloc): buffers the DMA reads / writes directly, no staging copies in
    rk_place_batch / rk_place_batch_packed.  The memory lives until the process ends (tests and the bench allocate a handful)."""
    lib = _lib.load()
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    nbytes = max(1, int(np.prod(shape)) * np.dtype(dtype).itemsize)
    p = _or_error(lib, lib.rk_host_alloc(nbytes), _lib.RK_ERR_NOMEM)
    return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p)).view(dtype)[:int(np.prod(shape))].reshape(shape)


def validate_db(alphabet, k, n_branches, thr_log10, thr, key_codes, row_offsets, branch_ids, scores,
                table_mode=RK_TABLE_AUTO, convert_uo=False):
    """rk_db_validate: argument checks + host-side image construction, no device needed. Returns rk_db_info."""
    lib = _lib.load()
    d, _keep = _db_desc(alphabet, k, n_branches, thr_log10, thr, key_codes, row_offsets, branch_ids, scores, table_mode, convert_uo)
    info = rk_db_info()
    _lib.check(lib.rk_db_validate(C.byref(d), C.byref(info)))
    return info


def save_db_image(path, alphabet, k, n_branches, thr_log10, thr, key_codes, row_offsets, branch_ids, scores, table_mode=RK_TABLE_AUTO,
                  convert_uo=False, user=b""):
    """rk_db_save_desc: the image file of a database given as CSR arrays, built on the host (no GPU needed)."""
    lib = _lib.load()
    d, _keep = _db_desc(alphabet, k, n_branches, thr_log10, thr, key_codes, row_offsets, branch_ids, scores, table_mode, convert_uo)
    user = bytes(user)
    _lib.check(lib.rk_db_save_desc(C.byref(d), str(path).encode(), user, len(user)))


def db_image_info(path):
    """rk_db_image_info + rk_db_image_user: (rk_db_info, user blob) of an image file after its size / checksum tests; no GPU needed."""
    lib = _lib.load()
    info, n = rk_db_info(), C.c_uint64(0)
    _lib.check(lib.rk_db_image_info(str(path).encode(), C.byref(info), C.byref(n)))
    buf = C.create_string_buffer(max(1, n.value))
    _lib.check(lib.rk_db_image_user(str(path).encode(), buf, n.value, C.byref(n)))
    return info, buf.raw[:n.value]


class _Handle:
    """A handle of the C ABI and its life: made by a create call of the library current at that moment, read through `handle` while it
    is open, freed by close() or with the object.  A class names its destroy call and the text of its closed-handle error."""
    _destroy = _closed = None

    @classmethod
    def _adopt(cls, lib, create, *args):
        """a new object around the handle that lib.<create>(*args, &handle) makes, without the class's __init__"""
        self = cls.__new__(cls)
        self._open(lib, create, *args)
        return self

    def _open(self, lib, create, *args):
        self._lib = lib
        self._h = C.c_void_p()
        _lib.check(getattr(lib, create)(*args, C.byref(self._h)))

    @property
    def handle(self):
        if not self._h:
            raise RuntimeError(self._closed)
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PhyloKmerDB(_Handle):
    """Phylo-kmer DB resident in one GPU's HBM (open-addressed / direct table + CSR rows)."""
    _destroy, _closed = "rk_db_destroy", "PhyloKmerDB is closed"

    def __init__(self, alphabet, k, n_branches, thr_log10, thr, key_codes, row_offsets, branch_ids, scores,
                 device=0, table_mode=RK_TABLE_AUTO, convert_uo=False):
        d, (key_codes, row_offsets, branch_ids, scores) = _db_desc(alphabet, k, n_branches, thr_log10, thr, key_codes, row_offsets, branch_ids,
                                                                   scores, table_mode, convert_uo, device)
        if row_offsets.shape[0] != key_codes.shape[0] + 1:
            raise ValueError("row_offsets must have n_keys+1 entries")
        if key_codes.shape[0] and int(row_offsets[-1]) != branch_ids.shape[0]:
            raise ValueError("row_offsets[-1] must equal len(branch_ids)")
        if branch_ids.shape[0] != scores.shape[0]:
            raise ValueError("branch_ids and scores differ in length")
        self._open(_lib.load(), "rk_db_create", C.byref(d))

    def _open(self, lib, create, *args):
        super()._open(lib, create, *args)
        self.info = rk_db_info()
        _lib.check(self._lib.rk_db_get_info(self._h, C.byref(self.info)))

    @classmethod
    def synthetic(cls, spec, device=0, table_mode=RK_TABLE_AUTO, convert_uo=False):
        """The seeded synthetic database of SURVEY 8(d) generated on the device straight into the HBM image
        (rk_db_create_synth); `spec` is a rappas_amd.synth.SynthSpec, whose numpy twin regenerates any row on the host."""
        d = _lib.rk_synth_desc(spec.alphabet, int(bool(convert_uo)), spec.k, spec.n_branches, float(spec.thr_log10), float(spec.thr),
                               int(spec.seed) & 0xFFFFFFFFFFFFFFFF, float(spec.key_fraction), float(spec.mean_row_len), device, table_mode)
        return cls._adopt(_lib.load(), "rk_db_create_synth", C.byref(d))

    def save(self, path, user=b""):
        """rk_db_save: this handle's HBM image as a file (the reference's SessionNext_v2.storeHash, SessionNext_v2.java:110-154);
        `user` = bytes the caller wants next to it (the tools keep the reference tree there)."""
        user = bytes(user)
        _lib.check(self._lib.rk_db_save(self.handle, str(path).encode(), user, len(user)))

    @classmethod
    def load(cls, path, device=0):
        """rk_db_load: a handle from an image file -- mmap + one upload per section, no rebuild (SessionNext_v2.load, :158-207)."""
        return cls._adopt(_lib.load(), "rk_db_load", str(path).encode(), device)

    def clone(self, device=0):
        """rk_db_clone: another handle of this database on `device`, copied device to device (no rebuild, no host round trip)."""
        return type(self)._adopt(self._lib, "rk_db_clone", self.handle, device)

    def fetch_row(self, code):
        """(branch_ids u16[len], scores f32[len]) of one k-mer code as stored in the HBM image; empty arrays if absent
        (CustomHash_v4_FastUtil81.getPairsOfTopPosition2, src/core/hash/CustomHash_v4_FastUtil81.java:146-153)."""
        n = C.c_uint32(0)
        cap = int(self.info.max_row_len)
        br = np.zeros(max(cap, 1), np.uint16)
        sc = np.zeros(max(cap, 1), np.float32)
        _lib.check(self._lib.rk_db_fetch_row(self.handle, int(code), cap, C.byref(n), _ptr(br), _ptr(sc)))
        return br[:n.value].copy(), sc[:n.value].copy()

    @classmethod
    def from_synth(cls, db, **kw):
        return cls(db.alphabet, db.k, db.n_branches, db.thr_log10, db.thr, db.key_codes, db.row_offsets,
                   db.branch_ids, db.scores, **kw)

    def set_lanes_per_read(self, lanes):
        _lib.check(self._lib.rk_set_lanes_per_read(self.handle, lanes))

    def kernel_name(self):
        return self._lib.rk_kernel_name(self.handle).decode()

    def packed_words(self, max_len):
        return int(self._lib.rk_packed_words(self.handle, max_len))


class PlacementProcess:
    """Mirror of core.algos.PlacementProcess for the hot path."""

    def __init__(self, db, ns_bound=float("-inf")):
        self.db = db
        self.ns_bound = ns_bound  # PlacementProcess(session, nsBound, queryLimit) (Main_PLACEMENT_v07.java:248-253)
        self._lib = _lib.load()

    def _params(self, keepAtMost, keepFactor, treatAmbiguities, treatAmbiguitiesWithMax):
        amb = RK_AMB_SKIP if not treatAmbiguities else (RK_AMB_MAX if treatAmbiguitiesWithMax else RK_AMB_MEAN)
        return rk_params(keepAtMost, keepFactor, amb, self.ns_bound)

    def _place_into(self, fn, head, reads, n, rule, out, translated=False):
        """one host placement call with a result set: fn(*head, &params, *reads, &result, [frame,] &counters) into `out` (made when
        None), the counters left in out.counters.  rule: (keepAtMost, keepFactor, treatAmbiguities, treatAmbiguitiesWithMax)"""
        out = _host_out(n, rule[0], out)
        if translated and (getattr(out, "frame", None) is None or out.frame.shape != (n,)):
            out.frame = np.full(n, _lib.RK_FRAME_NONE, np.uint8)
        res, p, ct = _result(out), self._params(*rule), rk_counters()
        _lib.check(fn(*head, C.byref(p), *reads, C.byref(res), *((_ptr(out.frame),) if translated else ()), C.byref(ct)))
        out.counters = _counters(ct)
        return out

    def _place_masses(self, fn, reads, rule, sums):
        """one profile-only call: fn(handle, &params, *reads, *sums, &counters), where `sums` are host arrays, None or numbers and end
        with the mass buffer and the flags -> (masses, flags, counters)"""
        p, ct = self._params(*rule), rk_counters()
        _lib.check(fn(self.db.handle, C.byref(p), *reads, *(_ptr(a) if isinstance(a, np.ndarray) else a for a in sums), C.byref(ct)))
        return sums[-2], sums[-1], _counters(ct)

    def processQueries(self, seq, seq_off, keepAtMost=7, keepFactor=0.01, treatAmbiguities=True,
                       treatAmbiguitiesWithMax=False, out=None, strand="forward"):
        """seq: uint8 ASCII of all reads concatenated (no gap stripping, as FASTAPointer(q,false) delivers them);
        seq_off: uint64 [n+1].  Defaults = src/main_v2/ArgumentsParser_v2.java:87-91.  `out`: a Placements to reuse.
        strand (DNA databases): "forward" = the reads as given (rk_place_batch, the reference's behaviour), "reverse" = their reverse
        complements, "both" = per read the strand with the better best score (rk_place_batch_strands; RK_FLAG_REVERSE marks the
        results that come from the reverse complement)."""
        seq, seq_off, n = _reads(seq, seq_off)
        rule, st = (keepAtMost, keepFactor, treatAmbiguities, treatAmbiguitiesWithMax), _strand(strand)
        if st == _lib.RK_STRAND_FORWARD:
            return self._place_into(self._lib.rk_place_batch, (self.db.handle,), (n, _ptr(seq), _ptr(seq_off)), n, rule, out)
        return self._place_into(self._lib.rk_place_batch_strands, (self.db.handle,), (st, n, _ptr(seq), _ptr(seq_off)), n, rule, out)

    def processQueriesTranslated(self, seq, seq_off, keepAtMost=7, keepFactor=0.01, out=None):
        """rk_place_batch_translated (amino-acid databases): DNA reads as characters, every read translated in its six reading frames
        on the device and placed on the database; per read the frame with the best score is reported.  Returns a Placements with one
        more array, `frame` (u8 [n]: 0..2 forward from base 0, 1, 2; 3..5 the reverse complement; 0xFF = no result).  Reads with an
        ambiguity code or an unsupported character come back unplaced with their flag."""
        seq, seq_off, n = _reads(seq, seq_off)
        return self._place_into(self._lib.rk_place_batch_translated, (self.db.handle,), (n, _ptr(seq), _ptr(seq_off)), n,
                                (keepAtMost, keepFactor, True, False), out, translated=True)

    def pack_reads_host(self, seq, seq_off, max_len=None, threads=0, out=None):
        """rk_pack_reads_host: ASCII reads -> (packed u32 [n, wpr], lens u32 [n], flags u32 [n]) on the host, the records the
        device packer would produce (AmbigSequenceKnife.java:103-130 char -> state).  `out` = (packed, lens, flags) to reuse."""
        seq, seq_off, n = _reads(seq, seq_off)
        if max_len is None:
            max_len = int((seq_off[1:] - seq_off[:-1]).max()) if n else 0
        wpr = self.db.packed_words(max_len)
        if out is not None:
            packed, lens, flags = out
            assert packed.shape == (n, wpr) and packed.dtype == np.uint32 and lens.shape == (n,) and flags.shape == (n,)
        else:
            packed, lens, flags = _packed_out(n, wpr)
        _lib.check(self._lib.rk_pack_reads_host(self.db.handle, n, _ptr(seq), _ptr(seq_off), wpr, _ptr(packed), _ptr(lens), _ptr(flags), threads))
        return packed, lens, flags

    def processQueriesPacked(self, packed, lens=None, fixed_len=0, flags=None, seq=None, seq_off=None, keepAtMost=7, keepFactor=0.01,
                             treatAmbiguities=True, treatAmbiguitiesWithMax=False, out=None):
        """rk_place_batch_packed: processQueries for reads already packed on the host (38 instead of 150 bytes per 150-bp read over
        PCIe); seq / seq_off are only needed for reads flagged AMBIGUOUS.  `out`: a Placements whose arrays are reused."""
        n, reads, _keep = _packed_reads(packed, lens, fixed_len, flags, seq, seq_off)
        return self._place_into(self._lib.rk_place_batch_packed, (self.db.handle,), reads, n,
                                (keepAtMost, keepFactor, treatAmbiguities, treatAmbiguitiesWithMax), out)

    def _flags_out(self, n, flags_out):
        """the flags of a profile-only call: made when None, else checked"""
        if flags_out is None:
            return np.zeros(n, np.uint32)
        if flags_out.dtype != np.uint32 or flags_out.shape != (n,) or not flags_out.flags.c_contiguous:
            raise ValueError("flags_out must be a contiguous uint32 array with one word per read")
        return flags_out

    def _masses_args(self, n, weights, masses, flags_out):
        """(weights u32 [n] or None, masses u64 [2B + 4], flags u32 [n]) of a profile-only call, checked / made"""
        words = masses_words(self.db.info.n_branches)
        if weights is not None and not isinstance(weights, np.ndarray):
            weights = np.asarray(weights, dtype=np.uint32)
        if weights is not None and (weights.dtype != np.uint32 or weights.shape != (n,) or not weights.flags.c_contiguous):
            raise ValueError("weights must be a contiguous uint32 array with one word per read")
        return weights, _host_masses(words, masses), self._flags_out(n, flags_out)

    def processQueriesMasses(self, seq, seq_off, weights=None, masses=None, strand="forward", translate=False, keepAtMost=7, keepFactor=0.01,
                             treatAmbiguities=True, treatAmbiguitiesWithMax=False, flags_out=None):
        """rk_place_batch_masses: profile-only placement.  The reads are placed as processQueries(strand=...) -- or, with translate=True,
        processQueriesTranslated -- would place them, but every chunk is summed on the device (accumulate_masses) and only the flags
        come back: no Placements.  Returns (masses uint64 [2B + 4], flags uint32 [n], counters): `masses` (made and zeroed when None)
        has received exactly what accumulate_masses_host would add for that call's result set and `weights` (uint32 [n], None = 1 a
        read); flags and counters are that call's.  The frame bytes of the translated step do not come back."""
        seq, seq_off, n = _reads(seq, seq_off)
        sums = self._masses_args(n, weights, masses, flags_out)
        step = _lib.RK_STEP_TRANSLATED if translate else _strand(strand)
        return self._place_masses(self._lib.rk_place_batch_masses, (step, n, _ptr(seq), _ptr(seq_off)),
                            (keepAtMost, keepFactor, treatAmbiguities, treatAmbiguitiesWithMax), sums)

    def processQueriesPackedMasses(self, packed, lens=None, fixed_len=0, flags=None, seq=None, seq_off=None, weights=None, masses=None,
                                   keepAtMost=7, keepFactor=0.01, treatAmbiguities=True, treatAmbiguitiesWithMax=False, flags_out=None):
        """rk_place_batch_packed_masses: processQueriesMasses for reads already packed on the host (the arguments of
        processQueriesPacked); the same (masses, flags, counters)."""
        n, reads, _keep = _packed_reads(packed, lens, fixed_len, flags, seq, seq_off)
        sums = self._masses_args(n, weights, masses, flags_out)
        return self._place_masses(self._lib.rk_place_batch_packed_masses, reads, (keepAtMost, keepFactor, treatAmbiguities, treatAmbiguitiesWithMax), sums)

    def _members_args(self, n, n_samples, member_off, member_sample, member_weight, masses, flags_out):
        """(n_samples, member_off u64 [n + 1] or None, member_sample u32, member_weight u32 or None, masses, flags) of a per-sample call"""
        masses = _samples_buffer(self.db.info.n_branches, n_samples, masses)
        if member_off is not None:
            member_off = np.ascontiguousarray(member_off, dtype=np.uint64)
            if member_off.shape != (n + 1,):
                raise ValueError("member_off must hold n_reads + 1 uint64 words")
        m = int(member_off[-1]) if member_off is not None else n
        member_sample, member_weight = _u32_list(member_sample, m, "member_sample"), _u32_list(member_weight, m, "member_weight")
        return n_samples, member_off, member_sample, member_weight, masses, self._flags_out(n, flags_out)

    def processQueriesMassesSamples(self, seq, seq_off, n_samples, member_sample, member_off=None, member_weight=None, masses=None, strand="forward",
                                    translate=False, keepAtMost=7, keepFactor=0.01, treatAmbiguities=True, treatAmbiguitiesWithMax=False, flags_out=None):
        """rk_place_batch_masses_samples: processQueriesMasses with one mass buffer per sample.  Read r owns the entries member_off[r] ..
        member_off[r + 1] of member_sample / member_weight (member_off None: one entry per read; member_weight None: 1).  Returns
        (masses uint64 [masses_samples_words(B, n_samples)], flags uint32 [n], counters): `masses` (made and zeroed when None) has
        received what accumulate_masses_samples_host would add for that call's result set with the entries expanded."""
        seq, seq_off, n = _reads(seq, seq_off)
        sums = self._members_args(n, n_samples, member_off, member_sample, member_weight, masses, flags_out)
        step = _lib.RK_STEP_TRANSLATED if translate else _strand(strand)
        return self._place_masses(self._lib.rk_place_batch_masses_samples, (step, n, _ptr(seq), _ptr(seq_off)),
                            (keepAtMost, keepFactor, treatAmbiguities, treatAmbiguitiesWithMax), sums)

    def processQueriesPackedMassesSamples(self, packed, n_samples, member_sample, member_off=None, member_weight=None, lens=None, fixed_len=0, flags=None,
                                          seq=None, seq_off=None, masses=None, keepAtMost=7, keepFactor=0.01, treatAmbiguities=True,
                                          treatAmbiguitiesWithMax=False, flags_out=None):
        """rk_place_batch_packed_masses_samples: processQueriesMassesSamples for reads already packed on the host (the arguments of
        processQueriesPacked); the same (masses, flags, counters)."""
        n, reads, _keep = _packed_reads(packed, lens, fixed_len, flags, seq, seq_off)
        sums = self._members_args(n, n_samples, member_off, member_sample, member_weight, masses, flags_out)
        return self._place_masses(self._lib.rk_place_batch_packed_masses_samples, reads, (keepAtMost, keepFactor, treatAmbiguities, treatAmbiguitiesWithMax), sums)

    def processQueriesMulti(self, dbs, seq, seq_off, keepAtMost=7, keepFactor=0.01, treatAmbiguities=True,
                            treatAmbiguitiesWithMax=False, out=None):
        """processQueries over several device handles of the same database from this one process
        (rk_place_batch_multi: contiguous shards, one host thread per handle, no collective)."""
        seq, seq_off, n = _reads(seq, seq_off)
        handles = (C.c_void_p * len(dbs))(*[d.handle for d in dbs])
        return self._place_into(self._lib.rk_place_batch_multi, (handles, len(dbs)), (n, _ptr(seq), _ptr(seq_off)), n,
                                (keepAtMost, keepFactor, treatAmbiguities, treatAmbiguitiesWithMax), out)

    # ---- device-resident variant (torch tensors only carry the memory and the stream) ----
    def place_packed(self, packed, fixed_len=0, lens=None, flags_in=None, seq_ascii=None, seq_off=None, out=None,
                     keepAtMost=7, keepFactor=0.01, treatAmbiguities=True, treatAmbiguitiesWithMax=False,
                     stream=None, strand="forward"):
        """rk_place_packed_device; with strand "reverse" / "both" rk_place_packed_device_strands, whose device workspace (the
        reverse records, a second result set, the reversed characters) is a tensor this object owns and grows as batches ask."""
        n, wpr = packed.shape
        dev = packed.device
        K = keepAtMost
        out = _device_out(n, K, dev, out)
        res = _result(out)
        p = self._params(keepAtMost, keepFactor, treatAmbiguities, treatAmbiguitiesWithMax)
        st = _stream(dev, stream)
        sd = _strand(strand)
        if sd == _lib.RK_STRAND_FORWARD:
            _lib.check(self._lib.rk_place_packed_device(self.db.handle, C.byref(p), n, packed.data_ptr(), wpr, _dp(lens),
                                                        fixed_len, _dp(flags_in), _dp(seq_ascii), _dp(seq_off), C.byref(res), st))
            return out
        chars = seq_ascii is not None and seq_off is not None and flags_in is not None
        need = int(self._lib.rk_strands_work_bytes(self.db.handle, n, wpr, K, max(1, seq_ascii.numel()) if chars else 0))
        if n:
            _or_error(self._lib, need, _lib.RK_ERR_INVALID if self.db.info.alphabet == RK_ALPHABET_DNA else _lib.RK_ERR_UNSUPPORTED)
        work = _grow(self, "_strand_work", dev, need)
        _lib.check(self._lib.rk_place_packed_device_strands(self.db.handle, C.byref(p), sd, n, packed.data_ptr(), wpr, _dp(lens),
                                                            fixed_len, _dp(flags_in), _dp(seq_ascii), _dp(seq_off),
                                                            C.byref(res), work.data_ptr(), work.numel(), st))
        return out

    def place_translated(self, dna, fixed_len=0, lens=None, flags_in=None, out=None, keepAtMost=7, keepFactor=0.01, stream=None):
        """rk_place_packed_device_translated (amino-acid databases): 2-bit DNA records [n, dna_words] (int32 tensor on the database's
        device, as rk_pack_reads(RK_ALPHABET_DNA) writes them) placed in their six reading frames; `out` gains "frame" (uint8 [n]).
        The device workspace (one frame's amino-acid records and lengths, a second result set) is a tensor this object owns and
        grows as batches ask."""
        n, wpr = dna.shape
        dev = dna.device
        K = keepAtMost
        out = _device_out(n, K, dev, out, frame=True)
        res = _result(out)
        p = self._params(keepAtMost, keepFactor, True, False)
        st = _stream(dev, stream)
        need = int(self._lib.rk_translated_work_bytes(self.db.handle, n, wpr, K))
        if n:
            _or_error(self._lib, need, _lib.RK_ERR_INVALID if self.db.info.alphabet == RK_ALPHABET_AA else _lib.RK_ERR_UNSUPPORTED)
        work = _grow(self, "_translated_work", dev, need)
        _lib.check(self._lib.rk_place_packed_device_translated(self.db.handle, C.byref(p), n, dna.data_ptr(), wpr, _dp(lens), fixed_len,
                                                               _dp(flags_in), C.byref(res), out["frame"].data_ptr(), work.data_ptr(),
                                                               work.numel(), st))
        return out

    def accumulate_masses(self, out, weights=None, masses=None, stream=None):
        """rk_masses_accumulate_device: the per-branch LWR sums of `out` -- the dict of device tensors place_packed / place_translated
        return -- ADDED into `masses`, an int64 tensor of masses_words(n_branches) words on the same device (the bits are unsigned:
        .cpu().numpy().view(numpy.uint64)), allocated and zeroed when None.  weights: int32 tensor [n] read as uint32 (None = 1 a
        read).  Asynchronous on the stream; the results are read, never written."""
        res, n, K, dev = _rows(out)
        masses = _device_masses(masses_words(self.db.info.n_branches), masses, dev, stream)
        _i32_tensor(weights, n, dev, "weights")
        _lib.check(self._lib.rk_masses_accumulate_device(self.db.handle, K, n, C.byref(res), _dp(weights), masses.data_ptr(), _stream(dev, stream)))
        return masses

    def accumulate_masses_samples(self, out, n_samples, member_sample, member_read=None, member_weight=None, masses=None, stream=None):
        """rk_masses_accumulate_samples_device: one mass buffer per sample from the membership entries (int32 tensors read as uint32, on
        the device of `out`) over `out` -- the dict of device tensors place_packed / place_translated return -- ADDED into `masses`, an
        int64 tensor of masses_samples_words(n_branches, n_samples) words on the same device, allocated and zeroed when None.
        member_read None: entry i is read i; member_weight None: 1.  Asynchronous on the stream."""
        res, n, K, dev = _rows(out)
        words = masses_samples_words(self.db.info.n_branches, n_samples)
        if not words:
            raise ValueError(f"n_samples={n_samples} on {self.db.info.n_branches} branches: 1..65535 and at most 2^29 words")
        masses = _device_masses(words, masses, dev, stream)
        m = member_sample.numel()
        for t, what in ((member_sample, "member_sample"), (member_read, "member_read"), (member_weight, "member_weight")):
            _i32_tensor(t, m, dev, what)
        _lib.check(self._lib.rk_masses_accumulate_samples_device(self.db.handle, K, n, C.byref(res), n_samples, m, _dp(member_read), member_sample.data_ptr(),
                                                                 _dp(member_weight), masses.data_ptr(), _stream(dev, stream)))
        return masses

    def translate_packed(self, dna, frame, fixed_len=0, lens=None, aa_words=None, stream=None):
        """rk_translate_packed_device: one reading frame of 2-bit DNA records [n, dna_words] -> (amino-acid records [n, aa_words],
        their lengths [n]) as new int32 tensors (translate_packed_host is the host twin)."""
        n, wpr = dna.shape
        if aa_words is None:
            aa_words = translated_words(wpr * 16 if lens is not None else fixed_len)
        aa, aa_lens = _alloc((n, aa_words), np.uint32, dna.device), _alloc(n, np.uint32, dna.device)
        _lib.check(self._lib.rk_translate_packed_device(self.db.handle, frame, n, dna.data_ptr(), wpr, _dp(lens),
                                                        fixed_len, aa.data_ptr(), aa_words, aa_lens.data_ptr(), _stream(dna.device, stream)))
        return aa, aa_lens

    def revcomp_packed(self, packed, fixed_len=0, lens=None, stream=None):
        """rk_revcomp_packed_device: the reverse complement of 2-bit records [n, wpr] (int32 tensor on the database's device) ->
        a new tensor of the same shape; lengths and flags are the same for both strands."""
        n, wpr = packed.shape
        out = _torch().empty_like(packed)
        _lib.check(self._lib.rk_revcomp_packed_device(self.db.handle, n, packed.data_ptr(), wpr, _dp(lens),
                                                      fixed_len, out.data_ptr(), _stream(packed.device, stream)))
        return out

    def revcomp_ascii(self, seq_ascii, seq_off, stream=None):
        """rk_revcomp_ascii_device: every read's characters reversed and complemented (hostio.revcomp is the numpy twin), same offsets."""
        out = _torch().empty_like(seq_ascii)
        _lib.check(self._lib.rk_revcomp_ascii_device(self.db.handle, seq_off.shape[0] - 1, seq_ascii.data_ptr(), seq_off.data_ptr(),
                                                     out.data_ptr(), _stream(seq_ascii.device, stream)))
        return out

    def count_work(self, packed, fixed_len=0, lens=None, flags_in=None, stream=None):
        """k-mers probed / k-mers with a row / row entries walked for a batch of packed reads (rk_count_work_device: a kernel of its own,
        the placement kernels carry no counters) -> dict"""
        n, wpr = packed.shape
        dev = packed.device
        out = _alloc(3, np.uint64, dev)
        _lib.check(self._lib.rk_count_work_device(self.db.handle, n, packed.data_ptr(), wpr, _dp(lens), fixed_len, _dp(flags_in), out.data_ptr(),
                                                  _stream(dev, stream)))
        if stream is not None:
            _torch().cuda.synchronize(dev)
        probed, hit, entries = (int(x) for x in out.tolist())
        return {"kmers_probed": probed, "kmers_hit": hit, "entries": entries}

    def pack_reads(self, seq_ascii, seq_off, max_len, stream=None):
        n = seq_off.shape[0] - 1
        dev = seq_ascii.device
        wpr = self.db.packed_words(max_len)
        packed, lens, flags = _packed_out(n, wpr, dev)
        _lib.check(self._lib.rk_pack_reads_device(self.db.handle, n, seq_ascii.data_ptr(), seq_off.data_ptr(), wpr,
                                                  packed.data_ptr(), lens.data_ptr(), flags.data_ptr(), _stream(dev, stream)))
        return packed, lens, flags


# ------------------------------------------------------------------------------------------------
# Sample-level output: clade masses and pairwise KR distances of a sample mass buffer (include/rappas_place.h)
# ------------------------------------------------------------------------------------------------
def _tree_arrays(parent, branch_len=None):
    parent = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1)
    if branch_len is not None:
        branch_len = np.ascontiguousarray(branch_len, dtype=np.float32).reshape(-1)
        if branch_len.shape != parent.shape:
            raise ValueError(f"branch_len holds {branch_len.shape[0]} lengths, parent {parent.shape[0]} nodes")
    return parent, branch_len


def _samples_in(n_branches, n_samples, masses):
    """a host sample mass buffer as the sample-level calls read it: n_samples * (2B + 4) words, the skipped-entries word optional"""
    masses = np.ascontiguousarray(masses, dtype=np.uint64).reshape(-1)
    W = 2 * n_branches + 4
    if masses.shape[0] not in (n_samples * W, n_samples * W + 1):
        raise ValueError(f"masses holds {masses.shape[0]} words, {n_samples} samples on {n_branches} branches have {n_samples * W} (+ 1)")
    return masses


def _host_samples(parent, branch_len, masses, n_samples):
    """what the sample-level host calls take in: (parent, branch_len, B, masses) as the C ABI reads them"""
    parent, branch_len = _tree_arrays(parent, branch_len)
    B = parent.shape[0]
    return parent, branch_len, B, _samples_in(B, n_samples, masses)


def tree_validate(parent, branch_len):
    """rk_tree_validate (no GPU): the checks of EdgeTree on a parent array (-1 = the root) and the lengths of the edges above the nodes;
    raises RkError (RK_ERR_INVALID and the message) for a tree the sample-level calls refuse"""
    parent, branch_len = _tree_arrays(parent, branch_len)
    _lib.check(_lib.load().rk_tree_validate(parent.shape[0], _ptr(parent), _ptr(branch_len)))


def clade_masses_host(parent, masses, n_samples):
    """rk_clade_masses_host (no GPU): uint64 [n_samples, B], the sum of mass_q30 over every node's subtree for each sample of a sample
    mass buffer (with n_samples = 1 an ordinary mass buffer) -- the clade_mass_q30 column of hostio.masses_table"""
    parent, _, B, masses = _host_samples(parent, None, masses, n_samples)
    clade = np.zeros((n_samples, B), np.uint64)
    _lib.check(_lib.load().rk_clade_masses_host(B, _ptr(parent), n_samples, _ptr(masses), _ptr(clade)))
    return clade


# rk_squash_merge: a row of the squash clustering (a and b the smallest sample indices of the two clusters, size after the merge)
SQUASH_MERGE = np.dtype([("a", "<u4"), ("b", "<u4"), ("size", "<u4"), ("reserved", "<u4"), ("distance", "<f8")])
assert SQUASH_MERGE.itemsize == 24

# a k-means run: assign uint32 [S] (KMEANS_NONE for a sample without mass), dist float64 [S], sizes uint32 [k], within float64 [k],
# info uint32 [4] = k_eff, n_active, rounds, converged | status << 1, centroids float64 [k, 2, B] or None
KMeans = collections.namedtuple("KMeans", "assign dist sizes within info centroids")
KMEANS_NONE = 0xFFFFFFFF

# the diversity measures of the samples: values float64 [S, 5 + 2 n_theta] (a NaN row for a sample without mass), columns their names
Diversity = collections.namedtuple("Diversity", "values columns")
DIVERSITY_FIXED = ("rooted_pd", "pd", "bwpd", "quadratic", "phylo_entropy")

# what epca_finish makes of a raw edge-PCA output: eigenvalue, share, residual [k]; projection [S, k]; loading [B, k]; the two info words
EdgePCA = collections.namedtuple("EdgePCA", "eigenvalue share residual projection loading n_active k_eff")


def _kmeans_seeds(seeds, k):
    if seeds is None:
        return None
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
    if seeds.shape[0] != k:
        raise ValueError(f"seeds must hold k = {k} sample indices")
    return seeds


def _diversity_theta(theta):
    """the thetas of a diversity call as the C ABI reads them: float64 [n_theta], None for none"""
    return np.ascontiguousarray(() if theta is None else theta, dtype=np.float64).reshape(-1)


def diversity_columns(theta):
    """the column names of a diversity table: the five fixed ones, then rooted_pd_<theta> and bwpd_<theta> per theta (%.17g)"""
    names = list(DIVERSITY_FIXED)
    for t in np.asarray(() if theta is None else theta, dtype=np.float64).reshape(-1):
        names += ["rooted_pd_%.17g" % t, "bwpd_%.17g" % t]
    return tuple(names)


def _epca_out(n_branches, n_samples, k):
    n = int(_lib.load().rk_epca_out_doubles(n_branches, n_samples, k))
    if not n:
        raise _lib.RkError(_lib.RK_ERR_INVALID, f"edge PCA: n_branches={n_branches}, n_samples={n_samples}, k={k}: out of 1..65535, 2..4096, 1..8")
    return n


# One description per sample-level analysis, for its three forms rk_<name>_host, rk_<name>_device and rk_<name>_batch.  `p` holds the
# call's own parameters, those behind n_samples in the public signatures.
#   work     rk_<work>_work_bytes(tree, n_samples, *args[:1]) sizes the device form's workspace: it depends on the first parameter
#   args     p -> the parameters as C takes them, in order; a host array among them (seeds, theta) is read during the call
#   outputs  (B, S, p) -> (name, shape or None for an output that is not asked for, numpy dtype), in the order C takes them
#   wrap     (outputs by name, p, host) -> the return value; host: host arrays (the _host and _batch forms), else device tensors
_SampleCall = collections.namedtuple("_SampleCall", "name work args outputs wrap")
_SAMPLE_CALLS = {c.name: c for c in (
    _SampleCall("kr_distances", "kr", lambda p: (),
                lambda B, S, p: (("out", (S, S), np.float64),),
                lambda o, p, host: o["out"]),
    # (n_merges: a word the host and batch forms hand back as a number, the device form as the tensor it is)
    _SampleCall("squash", "squash", lambda p: (),
                lambda B, S, p: (("merges", (max(S - 1, 0),), SQUASH_MERGE), ("n_merges", (1,), np.uint32)),
                lambda o, p, host: (o["merges"], int(o["n_merges"][0]) if host else o["n_merges"])),
    _SampleCall("kmeans", "kmeans", lambda p: (p["k"], p["max_rounds"], _kmeans_seeds(p["seeds"], p["k"])),
                lambda B, S, p: (("assign", (S,), np.uint32), ("dist", (S,), np.float64), ("sizes", (max(p["k"], 0),), np.uint32),
                                 ("within", (max(p["k"], 0),), np.float64), ("info", (4,), np.uint32),
                                 ("centroids", (max(p["k"], 0), 2, B) if p["centroids"] else None, np.float64)),
                lambda o, p, host: KMeans(**o)),
    _SampleCall("diversity", "diversity", lambda p: (p["theta"].shape[0], p["theta"] if p["theta"].shape[0] else None),
                lambda B, S, p: (("values", (S, len(DIVERSITY_FIXED) + 2 * p["theta"].shape[0]), np.float64),),
                lambda o, p, host: Diversity(o["values"], diversity_columns(p["theta"]))),
    # (sized with max(.., 0) and max(.., 1) above and here: a k or S out of range reaches the C side, which says so)
    _SampleCall("epca", "epca", lambda p: (p["k"], p["iters"]),
                lambda B, S, p: (("raw", (max(int(_lib.load().rk_epca_out_doubles(B, S, p["k"])), 1),), np.float64), ("info", (2,), np.uint32)),
                lambda o, p, host: (o["raw"], o["info"])),
)}


def _sample_outputs(call, B, S, p, dev=None):
    """the outputs of a sample-level call by name: zeroed host arrays, or tensors on `dev`; None where one is not asked for"""
    return {name: None if shape is None else _alloc(shape, dt, dev) for name, shape, dt in call.outputs(B, S, p)}


def _address(x):
    """a parameter or an output as C takes it: the address of a host array or a device tensor, anything else as it is"""
    return _ptr(x) if isinstance(x, np.ndarray) else x.data_ptr() if hasattr(x, "data_ptr") else x


def _sample_host(name, parent, branch_len, masses, n_samples, threads, **p):
    """the host form of a sample-level call: rk_<name>_host(B, parent, branch_len, n_samples, masses, parameters, outputs, threads)"""
    call = _SAMPLE_CALLS[name]
    parent, branch_len, B, masses = _host_samples(parent, branch_len, masses, n_samples)
    args = call.args(p)
    out = _sample_outputs(call, B, n_samples, p)
    _lib.check(getattr(_lib.load(), f"rk_{name}_host")(B, _ptr(parent), _ptr(branch_len), n_samples, _ptr(masses), *map(_address, args),
                                                       *map(_address, out.values()), threads))
    return call.wrap(out, p, True)


def kr_distances_host(parent, branch_len, masses, n_samples, threads=0):
    """rk_kr_distances_host (no GPU): float64 [n_samples, n_samples], the pairwise Kantorovich-Rubinstein distances between the samples
    of a sample mass buffer on the tree (parent, branch_len) -- the bits EdgeTree.kr_distances gives on the device.  A sample without
    mass has a NaN row and column."""
    return _sample_host("kr_distances", parent, branch_len, masses, n_samples, threads)


def squash_host(parent, branch_len, masses, n_samples, threads=0):
    """rk_squash_host (no GPU): (merges, n_merges) -- the squash clustering of the samples of a sample mass buffer on the tree (parent,
    branch_len): a SQUASH_MERGE array of n_samples - 1 rows, of which the first n_merges are merges and the rest fillers -- the bits
    EdgeTree.squash gives on the device.  A sample without mass takes no part."""
    return _sample_host("squash", parent, branch_len, masses, n_samples, threads)


def kmeans_host(parent, branch_len, masses, n_samples, k, max_rounds=100, seeds=None, centroids=True, threads=0):
    """rk_kmeans_host (no GPU): a KMeans of host arrays -- the phylogenetic k-means of the samples of a sample mass buffer on the tree
    (parent, branch_len), farthest-first seeds unless `seeds` gives k sample indices -- the bits EdgeTree.kmeans gives on the device."""
    return _sample_host("kmeans", parent, branch_len, masses, n_samples, threads, k=k, max_rounds=max_rounds, seeds=seeds, centroids=centroids)


def diversity_host(parent, branch_len, masses, n_samples, theta=(), threads=0):
    """rk_diversity_host (no GPU): a Diversity of host arrays -- rooted and unrooted phylogenetic diversity, balance-weighted PD,
    quadratic entropy and phylogenetic entropy of every sample of a sample mass buffer on the tree (parent, branch_len), and
    rooted_pd_theta / bwpd_theta for every theta in [0, 8] (at most 8) -- the bits EdgeTree.diversity gives on the device."""
    return _sample_host("diversity", parent, branch_len, masses, n_samples, threads, theta=_diversity_theta(theta))


def diversity_math_host(op, x, y=None):
    """rk_diversity_math_host (no GPU): the diversity measures' own rk_log2 (op 0), rk_exp2 (op 1) or pw(x, y) = x ** y (op 2),
    elementwise on float64 arrays"""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    y = None if y is None else np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if y is not None and y.shape != x.shape:
        raise ValueError("x and y must hold one value each per element")
    out = np.zeros(x.shape[0], np.float64)
    _lib.check(_lib.load().rk_diversity_math_host(op, x.shape[0], _ptr(x), _ptr(y), _ptr(out)))
    return out


def epca_host(parent, branch_len, masses, n_samples, k, iters, threads=0):
    """rk_epca_host (no GPU): (raw, info) -- the raw edge-PCA output of the samples of a sample mass buffer on the tree (parent, branch_len),
    float64 [1 + k * (3 + S + B)]: trace | lambda[k] | nn[k] | rr[k] | q[k][S] | w[k][B], and uint32 [2]: n_active, k_eff -- the bits
    EdgeTree.epca gives on the device.  epca_finish turns them into eigenvalues, projections and loadings."""
    return _sample_host("epca", parent, branch_len, masses, n_samples, threads, k=k, iters=iters)


def epca_finish(n_branches, n_samples, k, raw, info=None):
    """rk_epca_finish_host: an EdgePCA from a raw output (a host array, or a device tensor, which is downloaded) -- the eigenvalues of the
    Gram matrix of the centred edge imbalances, their shares of its trace, the residuals |G q - lambda q| of the unit vectors, the
    projections of the samples [S, k] and the unit-norm loadings of the edges [B, k].  The only square roots of the edge PCA are here."""
    if hasattr(raw, "cpu"):
        raw = raw.cpu().numpy()
    if info is not None and hasattr(info, "cpu"):
        info = info.cpu().numpy()
    raw = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1)
    if raw.shape[0] != _epca_out(n_branches, n_samples, k):
        raise ValueError(f"raw holds {raw.shape[0]} doubles, an edge PCA of {k} components of {n_samples} samples on {n_branches} branches has {_epca_out(n_branches, n_samples, k)}")
    ev, share, res = np.zeros(k), np.zeros(k), np.zeros(k)
    proj, load = np.zeros((n_samples, k)), np.zeros((n_branches, k))
    _lib.check(_lib.load().rk_epca_finish_host(n_branches, n_samples, k, _ptr(raw), _ptr(ev), _ptr(share), _ptr(res), _ptr(proj), _ptr(load)))
    n_active, k_eff = (None, None) if info is None else (int(np.asarray(info).view(np.uint32)[0]), int(np.asarray(info).view(np.uint32)[1]))
    return EdgePCA(ev, share, res, proj, load, n_active, k_eff)


def edpl_host(parent, branch_len, keep_at_most, n_rows, branch, lwr, threads=0):
    """rk_edpl_host (no GPU): float64 [n_reads], the expected distance between the placement locations of every read of a result set
    (n_rows u8 [n], branch u16 [n, K], lwr f64 [n, K]) on the tree (parent, branch_len): 2 * the sum over the pairs of its usable rows of
    lwr_i * lwr_j * the path between the midpoints of the two edges -- the bits EdgeTree.edpl gives on the device."""
    parent, branch_len = _tree_arrays(parent, branch_len)
    res, n, _, _ = _rows(Placements(n_rows, branch, None, lwr, None, None), keep_at_most)
    out = np.zeros(n, np.float64)
    _lib.check(_lib.load().rk_edpl_host(parent.shape[0], _ptr(parent), _ptr(branch_len), keep_at_most, n, C.byref(res), _ptr(out), threads))
    return out


def tree_distance_host(parent, branch_len, a, b):
    """rk_tree_distance_host (no GPU): float64 [n], the path between the midpoints of the edges above a[i] and b[i] on the tree (parent,
    branch_len), the d(a, b) of the EDPL; the midpoint of the root's edge is the root"""
    parent, branch_len = _tree_arrays(parent, branch_len)
    a = np.ascontiguousarray(a, dtype=np.uint16).reshape(-1)
    b = np.ascontiguousarray(b, dtype=np.uint16).reshape(-1)
    if a.shape != b.shape:
        raise ValueError("a and b must hold one branch each per pair")
    d = np.zeros(a.shape[0], np.float64)
    _lib.check(_lib.load().rk_tree_distance_host(parent.shape[0], _ptr(parent), _ptr(branch_len), a.shape[0], _ptr(a), _ptr(b), _ptr(d)))
    return d


class EdgeTree(_Handle):
    """rk_tree: the shape of a reference tree on the device -- parent[x] the node id of x's parent (-1 for the root), branch_len[x] the
    length of the edge above x -- for the sample-level calls over device mass buffers.  Takes and returns torch device tensors and owns
    its workspace (grow-only, one a tree: calls on different streams that overlap in time need a tree each)."""
    _destroy, _closed = "rk_tree_destroy", "EdgeTree is closed"

    def __init__(self, parent, branch_len, device=0):
        parent, branch_len = _tree_arrays(parent, branch_len)
        self.n_branches = parent.shape[0]
        self.device = device
        self._work_buf = None
        self._open(_lib.load(), "rk_tree_create", device, self.n_branches, _ptr(parent), _ptr(branch_len))

    def _masses(self, masses, n_samples):
        W = 2 * self.n_branches + 4
        if (masses.dtype != _torch().int64 or not masses.is_contiguous() or not masses.is_cuda or masses.device.index != self.device
                or masses.numel() not in (n_samples * W, n_samples * W + 1)):
            raise ValueError(f"masses must be a contiguous int64 tensor of {n_samples * W} (+ 1) words on cuda:{self.device}")
        return masses.device

    def clade_masses(self, masses, n_samples, stream=None):
        """rk_clade_masses_device: int64 tensor [n_samples, B] (the bits are unsigned), written; asynchronous on the stream"""
        dev = self._masses(masses, n_samples)
        clade = _alloc((n_samples, self.n_branches), np.uint64, dev)
        _lib.check(self._lib.rk_clade_masses_device(self.handle, n_samples, masses.data_ptr(), clade.data_ptr(), _stream(dev, stream)))
        return clade

    def _need(self, fn, *args):
        """the answer of a _work_bytes call, or the RkError of the shape it refuses"""
        return _or_error(self._lib, fn(self.handle, *args))

    def _batch_masses(self, n_samples, masses):
        """the host buffer of a _batch call as the C ABI reads it -- whole, the skipped-entries word with it -- or None: the one in the handle"""
        if masses is None:
            return None
        masses = _samples_in(self.n_branches, n_samples, masses)
        if masses.shape[0] != masses_samples_words(self.n_branches, n_samples):
            raise ValueError("masses must be a whole sample mass buffer (masses_samples_words)")
        return masses

    def _sample_device(self, name, masses, n_samples, stream, **p):
        """the device form of a sample-level call: rk_<name>_device(tree, n_samples, masses, parameters, outputs, work, work_bytes, stream)"""
        call = _SAMPLE_CALLS[name]
        dev = self._masses(masses, n_samples)
        args = call.args(p)
        work = _grow(self, "_work_buf", dev, self._need(getattr(self._lib, f"rk_{call.work}_work_bytes"), n_samples, *args[:1]))
        out = _sample_outputs(call, self.n_branches, n_samples, p, dev)
        _lib.check(getattr(self._lib, f"rk_{name}_device")(self.handle, n_samples, masses.data_ptr(), *map(_address, args), *map(_address, out.values()),
                                                           work.data_ptr(), work.numel(), _stream(dev, stream)))
        return call.wrap(out, p, False)

    def _sample_batch(self, name, db, n_samples, masses, **p):
        """the drivers' form of a sample-level call: rk_<name>_batch(db, tree, n_samples, masses or NULL, parameters, outputs)"""
        call = _SAMPLE_CALLS[name]
        masses = self._batch_masses(n_samples, masses)
        args = call.args(p)
        out = _sample_outputs(call, self.n_branches, n_samples, p)
        _lib.check(getattr(self._lib, f"rk_{name}_batch")(db.handle, self.handle, n_samples, _ptr(masses), *map(_address, args), *map(_address, out.values())))
        return call.wrap(out, p, True)

    def kr_work_bytes(self, n_samples):
        return self._need(self._lib.rk_kr_work_bytes, n_samples)

    def kr_distances(self, masses, n_samples, stream=None):
        """rk_kr_distances_device: float64 tensor [n_samples, n_samples], written; asynchronous on the stream"""
        return self._sample_device("kr_distances", masses, n_samples, stream)

    def kr_distances_batch(self, db, n_samples, masses=None):
        """rk_kr_distances_batch, the drivers' call: float64 array [n_samples, n_samples] on the host from a host sample mass buffer --
        or, masses None, from the buffer the last processQueriesMassesSamples call on `db` left on the device -- through
        rk_kr_distances_device on db's device; returns when the matrix is there"""
        return self._sample_batch("kr_distances", db, n_samples, masses)

    def squash_work_bytes(self, n_samples):
        return self._need(self._lib.rk_squash_work_bytes, n_samples)

    def squash(self, masses, n_samples, stream=None):
        """rk_squash_device: (merges, n_merges) as device tensors, written -- uint8 [n_samples - 1, 24], the rows of SQUASH_MERGE
        (merges.cpu().numpy().view(SQUASH_MERGE)), and int32 [1]; asynchronous on the stream"""
        return self._sample_device("squash", masses, n_samples, stream)

    def squash_batch(self, db, n_samples, masses=None):
        """rk_squash_batch, the drivers' call: (merges, n_merges) on the host, as squash_host gives them, from a host sample mass buffer --
        or, masses None, from the buffer the last processQueriesMassesSamples call on `db` left on the device -- through rk_squash_device
        on db's device; returns when the rows are there"""
        return self._sample_batch("squash", db, n_samples, masses)

    def kmeans_work_bytes(self, n_samples, k):
        return self._need(self._lib.rk_kmeans_work_bytes, n_samples, k)

    def kmeans(self, masses, n_samples, k, max_rounds=100, seeds=None, centroids=False, stream=None):
        """rk_kmeans_device: a KMeans of device tensors, written -- assign int32 [S] (the bits are unsigned: -1 is KMEANS_NONE), dist
        float64 [S], sizes int32 [k], within float64 [k], info int32 [4] and, when asked for, centroids float64 [k, 2, B] --, as
        kmeans_host gives them; asynchronous on the stream.  `seeds`: k sample indices on the host, read during the call."""
        return self._sample_device("kmeans", masses, n_samples, stream, k=k, max_rounds=max_rounds, seeds=seeds, centroids=centroids)

    def kmeans_batch(self, db, n_samples, k, max_rounds=100, masses=None, seeds=None, centroids=False):
        """rk_kmeans_batch, the drivers' call: a KMeans of host arrays, as kmeans_host gives them, from a host sample mass buffer -- or,
        masses None, from the buffer the last processQueriesMassesSamples call on `db` left on the device -- through rk_kmeans_device on
        db's device; returns when they are there"""
        return self._sample_batch("kmeans", db, n_samples, masses, k=k, max_rounds=max_rounds, seeds=seeds, centroids=centroids)

    def diversity_work_bytes(self, n_samples, n_theta=0):
        return self._need(self._lib.rk_diversity_work_bytes, n_samples, n_theta)

    def diversity(self, masses, n_samples, theta=(), stream=None):
        """rk_diversity_device: a Diversity whose values are a device tensor float64 [S, 5 + 2 n_theta], written, as diversity_host
        gives them; asynchronous on the stream.  `theta`: at most 8 values in [0, 8] on the host, read during the call."""
        return self._sample_device("diversity", masses, n_samples, stream, theta=_diversity_theta(theta))

    def diversity_batch(self, db, n_samples, theta=(), masses=None):
        """rk_diversity_batch, the drivers' call: a Diversity of host arrays, as diversity_host gives them, from a host sample mass
        buffer -- or, masses None, from the buffer the last processQueriesMassesSamples call on `db` left on the device -- through
        rk_diversity_device on db's device; returns when the table is there"""
        return self._sample_batch("diversity", db, n_samples, masses, theta=_diversity_theta(theta))

    def epca_work_bytes(self, n_samples, k):
        return self._need(self._lib.rk_epca_work_bytes, n_samples, k)

    def epca(self, masses, n_samples, k, iters, stream=None):
        """rk_epca_device: (raw, info) as device tensors, written -- float64 [1 + k * (3 + S + B)] and int32 [2] (n_active, k_eff), as
        epca_host gives them; asynchronous on the stream.  epca_finish(B, S, k, raw, info) downloads and finishes them."""
        return self._sample_device("epca", masses, n_samples, stream, k=k, iters=iters)

    def epca_batch(self, db, n_samples, k, iters, masses=None):
        """rk_epca_batch, the drivers' call: (raw, info) on the host, as epca_host gives them, from a host sample mass buffer -- or, masses
        None, from the buffer the last processQueriesMassesSamples call on `db` left on the device -- through rk_epca_device on db's
        device; returns when they are there"""
        return self._sample_batch("epca", db, n_samples, masses, k=k, iters=iters)

    def edpl_lds_bytes(self):
        """rk_edpl_lds_bytes: the bytes of the distance tables when edpl copies them into the LDS of every block, 0 when it reads them
        from global memory"""
        return int(self._lib.rk_edpl_lds_bytes(self.handle))

    def edpl(self, out, keep_at_most, stream=None):
        """rk_edpl_device: float64 tensor [n_reads], written -- the EDPL of every read of a device result set (`out`: the dict of device
        tensors a placement call returns; n_rows, branch [n, keep_at_most] and lwr [n, keep_at_most] are read); asynchronous on the stream"""
        torch = _torch()
        res, n, K, dev = _rows(out, keep_at_most)
        for what, dt, size in (("n_rows", torch.uint8, n), ("branch", torch.int16, n * K), ("lwr", torch.float64, n * K)):
            t = out[what]
            if t.dtype != dt or t.numel() != size or not t.is_contiguous() or not t.is_cuda or t.device.index != self.device:
                raise ValueError(f"{what} must be a contiguous {dt} tensor of {size} elements on cuda:{self.device}")
        edpl = _alloc(n, np.float64, out["n_rows"].device)
        _lib.check(self._lib.rk_edpl_device(self.handle, K, n, C.byref(res), edpl.data_ptr(), _stream(out["n_rows"].device, stream)))
        return edpl

    def edpl_batch(self, db, keep_at_most, n_rows, branch, lwr):
        """rk_edpl_batch, the drivers' call: float64 array [n_reads] on the host, as edpl_host gives it, from a host result set, in chunks
        through rk_edpl_device on db's device; returns when the values are there"""
        res, n, _, _ = _rows(Placements(n_rows, branch, None, lwr, None, None), keep_at_most)
        edpl = np.zeros(n, np.float64)
        _lib.check(self._lib.rk_edpl_batch(db.handle, self.handle, keep_at_most, n, C.byref(res), _ptr(edpl)))
        return edpl

    def close(self):
        super().close()
        self._work_buf = None
