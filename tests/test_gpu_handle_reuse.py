"""GPU (-m gpu): ONE rk_db handle over many batches, sizes, entry points and streams -- what the JNI stub and rk_place do.

The handle keeps state between calls: the four host-path workspaces (grow-only device and page-locked buffers, sized by each call's
reads, keep_at_most, record width and characters), one grow-only launch-scratch block per stream a caller has launched on (at most
sixteen; its layout -- histogram, counters, tile marks, permutation, keys, list of marked tiles -- is laid out anew from every
call's n_reads), and the lane-group width.  Every call made on the long-lived handle is compared with the same call on a handle
that was opened for it alone and closed afterwards: n_rows / branch / flags equal, score bit-equal, lwr exactly equal, every read
(same code, same inputs: no tolerance).  A slice of at most 600 reads of every call also goes to the CPU oracle (tests/util.py:
its tie rule, LWR_RTOL).  All result arrays are filled with the byte 0xA5 before a call, so that a row the call did not write is
garbage and not the right answer of an earlier call, and every result is held to the header's contract for unused rows."""
import ctypes as C
import threading

import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, synth
from oracle import oracle as O
from tests import golden_util as GU
from tests import strand_ref as SR
from tests.util import compare_with_oracle

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
ORACLE_READS = 600  # the largest slice the oracle is asked for; on 19 999 branches it takes ~4 ms a read: 150 there
ORACLE_READS_OF = {"large": 150, "wg": 150}
FIELDS = ("n_rows", "branch", "score", "lwr", "flags")
AMBIGUOUS = _lib.RK_FLAG_AMBIGUOUS

# dense: 999 branches, the dense 16-lane kernel; windowed: 7 999 branches; large: 19 999 branches with rows of ~300 entries (below the
# 320 at which an image takes the workgroup-per-read kernel: windowed too, with long rows); wg: the same tree with rows of ~400, the
# workgroup-per-read kernel (no launch scratch: there the sequences check that nothing else is carried over); protein: 5-bit records
MAKE_DB = {
    "dense": lambda: synth.make_config_db("C2", scale=0.2),
    "windowed": lambda: synth.make_db(4, 8, 7999, 40000, 520000, seed=7999),
    "large": lambda: synth.make_db(4, 6, 19999, 3000, 900_000, seed=5),
    "wg": lambda: synth.make_db(4, 6, 19999, 3000, 1_200_000, seed=5),
    "protein": lambda: synth.make_config_db("C4", scale=0.2),
}
FAMILY = {"dense": "place_packed16_kernel<G=16,BITS=2", "windowed": "place_packed16w_kernel", "wg": "place_wg_kernel", "protein": "BITS=5"}
ALL_DBS = ["dense", "windowed", "large", "wg", "protein"]

_DBS = {}


@pytest.fixture(scope="module")
def dbs():
    """name -> (SynthDB, OracleDB), each built once for the module"""
    def get(name):
        if name not in _DBS:
            sdb = MAKE_DB[name]()
            _DBS[name] = (sdb, O.OracleDB.from_synth(sdb))
        return _DBS[name]
    yield get
    for _, odb in _DBS.values():
        odb.close()
    _DBS.clear()
    _ORACLE.clear()
    _BATCHES.clear()


def _open(sdb, lanes=0):
    db = ra.PhyloKmerDB.from_synth(sdb)
    if lanes:
        db.set_lanes_per_read(lanes)
    return db


def _fresh(sdb, fn, lanes=0):
    """fn(handle) on a handle opened for this one call and closed after it"""
    db = _open(sdb, lanes)
    try:
        return fn(db)
    finally:
        db.close()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _gather(seq, off, idx):
    """the reads idx (in that order) of a batch -> (seq, off)"""
    lens = np.diff(off.astype(np.int64))[idx]
    new_off = np.zeros(len(idx) + 1, np.uint64)
    new_off[1:] = np.cumsum(lens)
    src = np.repeat(off[:-1].astype(np.int64)[idx] - new_off[:-1].astype(np.int64), lens) + np.arange(int(new_off[-1]))
    return np.ascontiguousarray(seq[src]), new_off


class Batch:
    """reads + the parameters of one call; the packed records and the oracle's slices are made once and kept"""

    def __init__(self, key, seq, off, K, amb="mean", chars=True):
        self.key, self.seq, self.off, self.K, self.amb, self.chars = key, np.ascontiguousarray(seq), np.ascontiguousarray(off), K, amb, chars
        self.n = len(off) - 1
        self._packed = None

    def packed(self, db):
        if self._packed is None:  # (the packer needs a handle for the alphabet only: the records do not depend on it)
            self._packed = ra.PlacementProcess(db).pack_reads_host(self.seq, self.off)
        return self._packed

    def oracle_idx(self, db, bare, limit=ORACLE_READS):
        """at most 600 reads, evenly spread over the batch; `bare` (no characters handed over): among the reads without an ambiguity code"""
        idx = np.arange(self.n)
        if bare:
            idx = idx[(self.packed(db)[2] & AMBIGUOUS) == 0]
        if len(idx) > limit:
            idx = idx[np.linspace(0, len(idx) - 1, limit).astype(np.int64)]
        return idx


def _take(p, idx):
    return ra.Placements(p.n_rows[idx], p.branch[idx], p.score[idx], p.lwr[idx], p.flags[idx], {})


_ORACLE = {}  # (database, batch key, reads, K, ambiguity mode, strand, bare) -> the oracle's result on that slice: computed once, never changed


def _oracle_check(name, odb, db, got, b, both=False, bare=False):
    if b.n == 0:
        return
    idx = b.oracle_idx(db, bare, ORACLE_READS_OF.get(name, ORACLE_READS))
    assert 0 < len(idx) <= ORACLE_READS, "no read for the oracle"
    seq, off = _gather(b.seq, b.off, idx)
    key = (name, b.key, b.n, b.K, b.amb, both, bare)
    kw = dict(keep_at_most=b.K, amb_mode=GU.AMB[b.amb])
    if key not in _ORACLE:
        _ORACLE[key] = SR.oracle_both(odb, seq, off, **kw)[0] if both else odb.place(seq, off, **kw)
    part = _take(got, idx)
    if both:
        SR.compare(part, _ORACLE[key], odb, seq, off, amb_mode=GU.AMB[b.amb])
    else:
        compare_with_oracle(part, _ORACLE[key], odb, seq, off, amb_mode=GU.AMB[b.amb])
    if bare:  # include/rappas_place.h: without their characters, reads with an ambiguity code come back unplaced with the flag set
        amb = (b.packed(db)[2] & AMBIGUOUS) != 0
        assert (got.n_rows[amb] == 0).all() and ((got.flags[amb] & AMBIGUOUS) != 0).all() and ((got.flags[amb] & _lib.RK_FLAG_PLACED) == 0).all()


def _same(got, want, what):
    """exact equality of two results of the same call, every read"""
    assert got.n_rows.shape == want.n_rows.shape and got.branch.shape == want.branch.shape, what
    n = len(want.n_rows)
    diff = (got.n_rows != want.n_rows) | (got.flags != want.flags)
    if n:
        diff |= (got.branch != want.branch).any(axis=1) | (got.score.view(np.uint32) != want.score.view(np.uint32)).any(axis=1)
        diff |= ~(got.lwr == want.lwr).all(axis=1)
    bad = np.nonzero(diff)[0]
    if len(bad):
        r = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {n} reads differ from the fresh handle's, reads {bad[:12].tolist()} ... {bad[-3:].tolist()}\n"
                             f"read {r}: n_rows {got.n_rows[r]} / {want.n_rows[r]} flags {got.flags[r]:#x} / {want.flags[r]:#x}\n"
                             f"branch {got.branch[r]} / {want.branch[r]}\nscore {got.score[r]} / {want.score[r]}\nlwr {got.lwr[r]} / {want.lwr[r]}")
    if got.counters or want.counters:
        assert got.counters == want.counters, (what, got.counters, want.counters)


def _check_rows(got, b, n_branches, what):
    """include/rappas_place.h: unused rows are branch 0xFFFF, score -inf, lwr 0; used ones name a branch of the tree"""
    K = b.K
    assert got.branch.shape == (b.n, K) and got.n_rows.shape == (b.n,), what
    nr = got.n_rows.astype(np.int64)
    assert (nr <= K).all(), what
    used = np.arange(K)[None, :] < nr[:, None]
    assert (got.branch[~used] == 0xFFFF).all() and np.isneginf(got.score[~used]).all() and (got.lwr[~used] == 0).all(), what
    assert (got.branch[used] < n_branches).all() and np.isfinite(got.score[used]).all(), what
    assert ((got.flags & ~np.uint32(0x7F)) == 0).all(), what


# ---- host entry points through ctypes, result arrays pre-filled with 0xA5 ----
class _Mem:
    """caller memory of one host call: pageable numpy arrays (the staged path) or rk_host_alloc buffers (the direct-DMA path)"""

    def __init__(self, lib, pinned):
        self.lib, self.pinned, self.ptrs = lib, pinned, []

    def empty(self, shape, dtype):
        shape = tuple(shape)
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if self.pinned:
            p = self.lib.rk_host_alloc(max(1, nbytes))
            assert p, "rk_host_alloc failed"
            self.ptrs.append(p)
            raw = np.ctypeslib.as_array((C.c_uint8 * max(1, nbytes)).from_address(p))
        else:
            raw = np.empty(max(1, nbytes), np.uint8)
        return raw[:nbytes].view(dtype).reshape(shape)

    def copy(self, a):
        if not self.pinned:
            return a
        out = self.empty(a.shape, a.dtype)
        out[...] = a
        return out

    def outputs(self, n, K):
        out = dict(n_rows=self.empty((n,), np.uint8), branch=self.empty((n, K), np.uint16), score=self.empty((n, K), np.float32),
                   lwr=self.empty((n, K), np.float64), flags=self.empty((n,), np.uint32))
        for a in out.values():
            a.view(np.uint8)[...] = SENTINEL
        return out

    def free(self):
        for p in self.ptrs:
            self.lib.rk_host_free(p)
        self.ptrs = []


def _host_call(db, entry, b, pinned=False):
    """entry: "ascii" rk_place_batch | "packed" / "packed_bare" rk_place_batch_packed with / without the characters |
    "both" rk_place_batch_strands(RK_STRAND_BOTH) -> Placements with the call's counters"""
    lib = _lib.load()
    mem = _Mem(lib, pinned)
    try:
        out = mem.outputs(b.n, b.K)
        res = _lib.rk_result(*[_ptr(out[f]) for f in FIELDS])
        p = _lib.rk_params(b.K, 0.01, GU.AMB[b.amb], float("-inf"))
        ct = _lib.rk_counters()
        C.memset(C.byref(ct), SENTINEL, C.sizeof(ct))
        seq, off = mem.copy(b.seq), mem.copy(b.off)
        if entry == "ascii":
            rc = lib.rk_place_batch(db.handle, C.byref(p), b.n, _ptr(seq), _ptr(off), C.byref(res), C.byref(ct))
        elif entry == "both":
            rc = lib.rk_place_batch_strands(db.handle, C.byref(p), _lib.RK_STRAND_BOTH, b.n, _ptr(seq), _ptr(off), C.byref(res), C.byref(ct))
        else:
            packed, lens, flags = (mem.copy(a) for a in b.packed(db))
            chars = entry == "packed"
            rc = lib.rk_place_batch_packed(db.handle, C.byref(p), b.n, _ptr(packed), packed.shape[1], _ptr(lens), 0, _ptr(flags),
                                           _ptr(seq) if chars else None, _ptr(off) if chars else None, C.byref(res), C.byref(ct))
        _lib.check(rc)
        return ra.Placements(*[out[f].copy() for f in FIELDS], {f: getattr(ct, f) for f, _ in _lib.rk_counters._fields_})
    finally:
        mem.free()


_BATCHES = {}


def _sym_len(sdb):
    return 100 if sdb.alphabet == 20 else 150


def _host_steps(name, sdb):
    """the sequence of test 1: every buffer of a workspace grows, then is used by a smaller call"""
    if name not in _BATCHES:
        a, L = sdb.alphabet, _sym_len(sdb)
        b1 = Batch("h1", *synth.make_reads(a, 300, 40, seed=11), K=1)
        b2 = Batch("h2", *synth.make_reads(a, 5000, 400, seed=12, amb_rate=0.01, bad_rate=0.01, var_len=400), K=16)  # lengths 0 ... 400
        b3 = Batch("h3", *synth.make_reads(a, 7, L, seed=13), K=7)
        b4 = Batch("h4", np.zeros(0, np.uint8), np.zeros(1, np.uint64), K=7)
        b5 = Batch("h5", *synth.make_reads(a, 1, 3000, seed=15), K=7)
        # (ragged, so that a few dozen short reads carry no ambiguity code: what the call without characters still places)
        b6 = Batch("h6", *synth.make_reads(a, 2000, L, seed=16, amb_rate=0.08, var_len=L - 10), K=7)
        steps = [("ascii", b1), ("ascii", b2), ("ascii", b3), ("ascii", b4), ("ascii", b5), ("ascii", b6), ("packed", b6), ("packed_bare", b6)]
        if a == 4:
            steps.append(("both", b6))
        steps.append(("ascii", b1))
        _BATCHES[name] = steps
    return _BATCHES[name]


def _run_host_steps(name, sdb, odb, db, pinned, compare=True):
    steps = _host_steps(name, sdb)
    results = []
    for i, (entry, b) in enumerate(steps):
        what = f"{name} step {i + 1} ({entry}, {b.n} reads, K={b.K}, {'page-locked' if pinned else 'pageable'})"
        got = _host_call(db, entry, b, pinned)
        results.append(got)
        if not compare:
            continue
        want = _fresh(sdb, lambda f: _host_call(f, entry, b, pinned))
        _same(got, want, what)
        assert got.counters["reads"] == b.n and got.counters["placed"] == int((got.flags & 1).sum()), what
        _check_rows(got, b, sdb.n_branches, what)
        _oracle_check(name, odb, db, got, b, both=entry == "both", bare=entry == "packed_bare")
        if entry == "packed_bare":
            assert ((b.packed(db)[2] & AMBIGUOUS) == 0).sum() >= 20  # (some reads the call still places)
    _same(results[-1], results[0], f"{name}: the first call made again")
    return results


def _assert_family(name, db):
    if name in FAMILY:
        assert FAMILY[name] in db.kernel_name(), db.kernel_name()


# ---- 1. host path ----
@pytest.mark.parametrize("memory", ["pageable", "page_locked"])
@pytest.mark.parametrize("name", ALL_DBS)
def test_host_path_buffers_grow_and_are_reused_by_smaller_calls(name, memory, dbs):
    """300 reads K=1 | 5 000 ragged reads K=16 with ambiguity codes and unsupported characters | 7 reads | the empty batch | one read
    of 3 000 symbols | 2 000 reads full of ambiguity codes (the character buffers grow) | the same through rk_place_batch_packed with
    and without the characters | DNA: on both strands (the strands workspace grows) | the first call again, bit-equal to itself"""
    sdb, odb = dbs(name)
    db = _open(sdb)
    try:
        _assert_family(name, db)
        _run_host_steps(name, sdb, odb, db, memory == "page_locked")
    finally:
        db.close()


@pytest.mark.parametrize("name", ALL_DBS)
def test_host_path_in_chunks_of_1024_reads_alternates_the_workspaces(name, dbs, monkeypatch, dev_lib):
    """RK_CHUNK_READS=1024 (the knob's minimum): the 5 000-read call takes five chunks over the four workspaces, and the calls behind
    it land in workspaces that last held a full chunk"""
    monkeypatch.setenv("RK_CHUNK_READS", "1024")
    sdb, odb = dbs(name)
    db = _open(sdb)
    try:
        _run_host_steps(name, sdb, odb, db, False)
    finally:
        db.close()


# ---- 2. rk_reserve_host_path ----
@pytest.mark.parametrize("name", ["dense", "protein"])
def test_reserve_host_path_between_batches(name, dbs):
    """rk_reserve_host_path pre-sizes the four workspaces and the launch scratch and runs a batch of 32 768 short reads of its own
    through the handle: whatever it is asked for, and whenever, the batches placed afterwards are the fresh handle's"""
    sdb, odb = dbs(name)
    lib = _lib.load()
    a, L = sdb.alphabet, _sym_len(sdb)
    small = Batch("r1", *synth.make_reads(a, 3000, L, seed=21, amb_rate=0.001, var_len=40), K=7)
    wide = Batch("r2", *synth.make_reads(a, 2500, 400, seed=22, amb_rate=0.002, bad_rate=0.01, var_len=300), K=16)
    # Beyond what (K=1, 20 symbols) reserves for a chunk of 2^18 reads (+ 25 %): 2.6 MB of lwr = 20 480 reads at K = 16, 2.6 MB (DNA) /
    # 5.2 MB (amino acids) of records = 26 000 / 20 800 reads of 400 symbols
    big = Batch("r3", *synth.make_reads(a, 30000, 400, seed=23, amb_rate=0.0005, var_len=200), K=16)
    want = {b.key: _fresh(sdb, lambda f, b=b: _host_call(f, "ascii", b)) for b in (small, wide, big)}

    def place(db, b, what):
        got = _host_call(db, "ascii", b)
        _same(got, want[b.key], f"{name}: {what}")
        _check_rows(got, b, sdb.n_branches, what)
        _oracle_check(name, odb, db, got, b)

    db = _open(sdb)
    try:
        _lib.check(lib.rk_reserve_host_path(db.handle, 7, 150))
        place(db, small, "after reserve(7, 150) on a new handle")
        _lib.check(lib.rk_reserve_host_path(db.handle, 3, 60))
        place(db, wide, "after a smaller reserve(3, 60)")
        place(db, small, "the small batch behind it")
        _lib.check(lib.rk_reserve_host_path(db.handle, 16, 400))
        place(db, wide, "after a larger reserve(16, 400)")
        place(db, small, "the small batch behind it")
        # errors leave the handle as it was
        for h, K in ((None, 7), (db.handle, 0), (db.handle, 17)):
            assert lib.rk_reserve_host_path(h, K, 150) == _lib.RK_ERR_INVALID
            assert lib.rk_last_error().decode() != ""
        place(db, small, "after three refused reserves")
    finally:
        db.close()
    db = _open(sdb)
    try:
        _lib.check(lib.rk_reserve_host_path(db.handle, 1, 20))
        place(db, big, "30 000 reads of up to 400 symbols at K=16 after reserve(1, 20): every buffer has to grow")
        place(db, small, "the small batch behind it")
    finally:
        db.close()


# ---- device path ----
def _clade_reads(sdb, n, length, seed):
    """reads that sit in one neighbourhood of THIS database's tree, as the reads of tests/test_gpu_parity.py's _clade_db /
    make_motif_reads sit in theirs: uniform reads with a k-mer of the database at each of the seven places the tile-order pre-pass
    looks at (rk_kernels.hip: retile_read_key), all seven from rows that start within a few branches of each other"""
    rng = np.random.default_rng(seed)
    seq, off = synth.make_reads(sdb.alphabet, n, length, seed=seed)
    seq = seq.reshape(n, length).copy()
    letters = synth.DNA_LETTERS if sdb.alphabet == 4 else synth.AA_LETTERS
    bits = np.uint64(sdb.bits)
    by_place = np.argsort(sdb.branch_ids[sdb.row_offsets[:-1].astype(np.int64)], kind="stable")
    span = max(8, sdb.n_keys // 400)
    centre = rng.integers(0, sdb.n_keys - span, size=n)
    Q = length - sdb.k + 1
    for i in range(7):
        p = (Q - 1) * i // 6
        codes = sdb.key_codes[by_place[centre + rng.integers(0, span, size=n)]]
        for j in range(sdb.k):
            seq[:, p + j] = letters[((codes >> (bits * np.uint64(j))) & np.uint64((1 << sdb.bits) - 1)).astype(np.int64)]
    return seq.reshape(-1), off


def _device_batch(sdb, key, n, K, chars, seed, mixed):
    """mixed: seven clade-shaped reads in ten, interleaved with ragged uniform ones (ambiguity codes, unsupported characters): the
    pre-pass re-tiles the batch and the permutation is not the identity"""
    a, L = sdb.alphabet, _sym_len(sdb)
    if mixed:
        n1 = n * 7 // 10
        s1, o1 = _clade_reads(sdb, n1, L, seed)
        s2, o2 = synth.make_reads(a, n - n1, L, seed=seed + 1, amb_rate=0.001, bad_rate=0.003, var_len=L // 2)
        seq, off = _gather(np.concatenate([s1, s2]), np.concatenate([o1, o2[1:] + o1[-1]]), np.random.default_rng(seed).permutation(n))
    else:
        seq, off = synth.make_reads(a, n, L, seed=seed, amb_rate=0.002, bad_rate=0.01, var_len=L // 2)
    return Batch(key, seq, off, K, "mean" if chars else "skip", chars)


def _device_queue(name, sdb, sizes, tag, mixed_from=33000):
    """K alternates 7 / 16 from call to call; mean with the characters / skip without them alternates every second call, so that the
    large batches (every second call) see both"""
    key = (name, tag)
    if key not in _BATCHES:
        _BATCHES[key] = [_device_batch(sdb, f"{tag}{i}", n, (7, 16)[i % 2], (i // 2) % 2 == 0, 100 + i, n >= mixed_from) for i, n in enumerate(sizes)]
    return _BATCHES[key]


def _prepare(db, b):
    """inputs and 0xA5-filled outputs of one device call, on torch's current stream"""
    import torch
    packed, lens, flags = b.packed(db)
    kw = dict(packed=torch.from_numpy(packed.view(np.int32)).cuda(), lens=torch.from_numpy(lens.view(np.int32)).cuda(),
              flags_in=torch.from_numpy(flags.view(np.int32)).cuda())
    if b.chars:
        kw["seq_ascii"] = torch.from_numpy(b.seq).cuda()
        kw["seq_off"] = torch.from_numpy(b.off.view(np.int64)).cuda()
    raw = lambda nbytes: torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    n, K = b.n, b.K
    kw["out"] = dict(n_rows=raw(n), branch=raw(n * K * 2).view(torch.int16).view(n, K), score=raw(n * K * 4).view(torch.float32).view(n, K),
                     lwr=raw(n * K * 8).view(torch.float64).view(n, K), flags=raw(n * 4).view(torch.int32))
    return kw


def _launch(pp, b, kw, stream):
    """stream: a hipStream_t as an integer (0 = the null stream), or None = torch's current stream"""
    pp.place_packed(keepAtMost=b.K, treatAmbiguities=b.amb != "skip", stream=stream, **kw)


def _to_host(out):
    return ra.Placements(out["n_rows"].cpu().numpy(), out["branch"].cpu().numpy().view(np.uint16), out["score"].cpu().numpy(),
                         out["lwr"].cpu().numpy(), out["flags"].cpu().numpy().view(np.uint32), {})


def _device_once(db, b):
    import torch
    kw = _prepare(db, b)
    _launch(ra.PlacementProcess(db), b, kw, None)
    torch.cuda.synchronize()
    return _to_host(kw["out"])


class _FreshCache:
    """the fresh handle's result of a device call, computed once per batch"""

    def __init__(self, sdb):
        self.sdb, self.known = sdb, {}

    def get(self, b):
        if b.key not in self.known:
            self.known[b.key] = _fresh(self.sdb, lambda f: _device_once(f, b))
        return self.known[b.key]


def _check_device(name, sdb, odb, db, b, got, fresh, what):
    what = f"{name}: {what} ({b.n} reads, K={b.K}, {'mean with' if b.chars else 'skip without'} characters)"
    _same(got, fresh.get(b), what)
    _check_rows(got, b, sdb.n_branches, what)
    _oracle_check(name, odb, db, got, b, bare=not b.chars)


def _queue_on_one_stream(name, sdb, odb, sizes, tag, mixed_from):
    import torch
    queue = _device_queue(name, sdb, sizes, tag, mixed_from)
    fresh = _FreshCache(sdb)
    db = _open(sdb)
    try:
        pp = ra.PlacementProcess(db)
        preps = [_prepare(db, b) for b in queue]           # on the default stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        for b, kw in zip(queue, preps):                    # back to back, no synchronisation in between
            _launch(pp, b, kw, side.cuda_stream)
        side.synchronize()
        for i, (b, kw) in enumerate(zip(queue, preps)):
            _check_device(name, sdb, odb, db, b, _to_host(kw["out"]), fresh, f"call {i + 1} of the queue")
    finally:
        db.close()


# ---- 3. one stream, calls queued back to back ----
@pytest.mark.parametrize("name", ALL_DBS)
def test_device_calls_queued_on_one_side_stream(name, dbs):
    """100, 40 000, 5, 33 000, 32 767, 32 768 and 3 reads on one non-default stream without a synchronisation in between: across the
    32 768-read threshold of the tile order in both directions, and the scratch block grows (hipStreamSynchronize + hipFree inside
    launch_scratch) while earlier calls are still queued.  The two largest batches are re-tiled (clade-shaped reads among uniform ones)"""
    sdb, odb = dbs(name)
    _queue_on_one_stream(name, sdb, odb, [100, 40000, 5, 33000, 32767, 32768, 3], "q", 33000)


def test_device_calls_queued_with_the_tile_order_for_every_batch(dbs, monkeypatch, dev_lib):
    """RK_RETILE_MIN_READS=0 on the windowed tree: marks, list and permutation all exist for 4 001, 13, 2 500 and 4 001 reads, and
    their offsets inside the block move with n_reads"""
    monkeypatch.setenv("RK_RETILE_MIN_READS", "0")
    sdb, odb = dbs("windowed")
    _queue_on_one_stream("windowed", sdb, odb, [4001, 13, 2500, 4001], "t", 2500)


# ---- 4. several streams on one handle ----
@pytest.mark.parametrize("name", ["dense", "windowed"])
def test_interleaved_streams_with_host_calls_in_between(name, dbs):
    """three side streams, torch's default stream and the null stream, calls of different sizes dealt out in turn without a
    synchronisation, rk_place_batch calls (the handle's own four streams) made in between; the device is synchronised once"""
    import torch
    sdb, odb = dbs(name)
    sizes = [3000, 17, 40000, 700, 33000, 5, 1200, 2500, 64, 36000]
    queue = _device_queue(name, sdb, sizes, "i", 33000)
    host_b = Batch("ih", *synth.make_reads(sdb.alphabet, 1500, 150, seed=31, amb_rate=0.002, var_len=60), K=7)
    host_want = _fresh(sdb, lambda f: _host_call(f, "ascii", host_b))
    fresh = _FreshCache(sdb)
    db = _open(sdb)
    try:
        pp = ra.PlacementProcess(db)
        preps = [_prepare(db, b) for b in queue]
        side = [torch.cuda.Stream() for _ in range(3)]
        for s in side:
            s.wait_stream(torch.cuda.current_stream())
        streams = [s.cuda_stream for s in side] + [torch.cuda.current_stream().cuda_stream, 0]
        host_got = []
        for i, (b, kw) in enumerate(zip(queue, preps)):
            _launch(pp, b, kw, streams[i % len(streams)])
            if i % 3 == 2:
                host_got.append(_host_call(db, "ascii", host_b))
        torch.cuda.synchronize()
        for i, (b, kw) in enumerate(zip(queue, preps)):
            _check_device(name, sdb, odb, db, b, _to_host(kw["out"]), fresh, f"call {i + 1}, stream {i % len(streams) + 1} of 5")
        for i, got in enumerate(host_got):
            _same(got, host_want, f"{name}: host call {i + 1} between the device calls")
            _check_rows(got, host_b, sdb.n_branches, "host call")
        _oracle_check(name, odb, db, host_got[0], host_b)
    finally:
        db.close()


@pytest.mark.parametrize("name,sizes", [("dense", [32768, 33001, 34000]), ("windowed", [900, 33001, 2100])])
def test_more_streams_than_scratch_blocks(name, sizes, dbs):
    """eighteen streams, one call on each in turn: past the sixteen blocks a handle keeps, so the two least recently used ones are
    freed (behind a hipDeviceSynchronize); then the first stream again, whose block is gone and is made anew.  (The dense kernels
    ask for scratch from 32 768 reads on, the windowed ones for every batch.)"""
    import torch
    sdb, odb = dbs(name)
    batches = _device_queue(name, sdb, sizes, "e", 32768)
    fresh = _FreshCache(sdb)
    db = _open(sdb)
    try:
        pp = ra.PlacementProcess(db)
        calls = [batches[i % len(batches)] for i in range(19)]
        preps = [_prepare(db, b) for b in calls]
        streams = [torch.cuda.Stream() for _ in range(18)]  # all alive until the end
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
        for i, (b, kw) in enumerate(zip(calls, preps)):
            _launch(pp, b, kw, streams[i % 18].cuda_stream)
        torch.cuda.synchronize()
        for i, (b, kw) in enumerate(zip(calls, preps)):
            got = _to_host(kw["out"])
            _same(got, fresh.get(b), f"{name}: call {i + 1} on stream {i % 18 + 1} of 18")
            _check_rows(got, b, sdb.n_branches, f"call {i + 1}")
            if i in (0, 1, 2, 17, 18):
                _oracle_check(name, odb, db, got, b, bare=not b.chars)
    finally:
        db.close()


@pytest.mark.parametrize("name", ["dense", "windowed"])
def test_two_host_threads_each_on_its_own_stream(name, dbs):
    """the header forbids only overlapping calls on ONE stream: two threads, each with a stream, inputs and outputs of its own,
    make ten calls of different sizes each on one handle"""
    import torch
    sdb, odb = dbs(name)
    sizes = ([10, 33000, 500, 40000, 3, 32768, 2000, 64, 35000, 700], [36000, 7, 32767, 1000, 34000, 129, 5, 33500, 250, 38000])
    queues = [_device_queue(name, sdb, sz, f"w{t}", 32768) for t, sz in enumerate(sizes)]
    fresh = _FreshCache(sdb)
    db = _open(sdb)
    try:
        preps = [[_prepare(db, b) for b in q] for q in queues]
        streams = [torch.cuda.Stream() for _ in queues]
        torch.cuda.synchronize()  # the inputs are there before a thread starts
        errors = []

        def work(t):
            try:
                pp = ra.PlacementProcess(db)
                for b, kw in zip(queues[t], preps[t]):
                    _launch(pp, b, kw, streams[t].cuda_stream)
                streams[t].synchronize()
            except BaseException as e:  # noqa: B036 -- handed to the main thread
                errors.append((t, e))

        threads = [threading.Thread(target=work, args=(t,)) for t in range(len(queues))]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=120)
        assert not any(th.is_alive() for th in threads), "a thread did not come back"
        if errors:
            raise errors[0][1]
        torch.cuda.synchronize()
        for t, q in enumerate(queues):
            for i, (b, kw) in enumerate(zip(q, preps[t])):
                _check_device(name, sdb, odb, db, b, _to_host(kw["out"]), fresh, f"thread {t + 1}, call {i + 1}")
    finally:
        db.close()


# ---- 5. rk_set_lanes_per_read between batches ----
@pytest.mark.parametrize("name", ["dense", "windowed"])
def test_lane_group_width_changed_between_batches(name, dbs):
    """0 -> 32 -> 64 -> 0: rk_kernel_name tells the family of the next launch, each batch is the one of a fresh handle set to the same
    width, and back at 0 the very first result comes out again; a width the engine refuses leaves the handle usable"""
    sdb, odb = dbs(name)
    b = Batch("l1", *synth.make_reads(sdb.alphabet, 3000, 150, seed=41, amb_rate=0.001, bad_rate=0.002, var_len=50), K=7)
    b16 = Batch("l2", b.seq, b.off, K=16)
    db = _open(sdb)
    try:
        name0 = db.kernel_name()
        _assert_family(name, db)
        results = []
        for lanes in (0, 32, 64, 0):
            db.set_lanes_per_read(lanes)
            kn = db.kernel_name()
            assert kn == name0 if lanes == 0 else f"place_packed_kernel<G={lanes}," in kn, (lanes, kn)
            got = _host_call(db, "ascii", b)
            _same(got, _fresh(sdb, lambda f: _host_call(f, "ascii", b), lanes), f"{name}: lanes_per_read={lanes}")
            _check_rows(got, b, sdb.n_branches, f"lanes {lanes}")
            _oracle_check(name, odb, db, got, b)
            results.append(got)
        _same(results[3], results[0], f"{name}: back at width 0")
        with pytest.raises(ra.RkError):   # no such width: refused when it is set
            db.set_lanes_per_read(5)
        assert db.kernel_name() == name0
        db.set_lanes_per_read(8)          # a legal width that cannot serve this call (16 winners from 8 lanes; on the larger tree
        with pytest.raises(ra.RkError):   # eight score vectors do not fit a CU either): refused when the batch is placed
            _host_call(db, "ascii", b16)
        db.set_lanes_per_read(0)
        assert db.kernel_name() == name0
        _same(_host_call(db, "ascii", b), results[0], f"{name}: width 0 after two refusals")
        got16 = _host_call(db, "ascii", b16)
        _same(got16, _fresh(sdb, lambda f: _host_call(f, "ascii", b16)), f"{name}: K=16 at width 0 after the refusals")
        _oracle_check(name, odb, db, got16, b16)
    finally:
        db.close()


# ---- 6. lifetime ----
@pytest.mark.parametrize("name", ["dense", "windowed"])
def test_clone_outlives_a_much_used_source(name, dbs):
    """a handle that has been through the host sequence is cloned and destroyed; the clone (its own workspaces and scratch, none of
    the source's) places like a fresh handle on the host and the device path"""
    sdb, odb = dbs(name)
    hb = Batch("clone_host", *synth.make_reads(sdb.alphabet, 2500, 150, seed=51, amb_rate=0.002, bad_rate=0.004, var_len=70), K=7)
    dq = _device_queue(name, sdb, [33000, 900], "c", 33000)
    fresh = _FreshCache(sdb)
    src = _open(sdb)
    clone = None
    try:
        _run_host_steps(name, sdb, odb, src, False, compare=False)
        clone = src.clone(0)
        src.close()
        assert clone.kernel_name() != ""
        _assert_family(name, clone)
        got = _host_call(clone, "ascii", hb)
        _same(got, _fresh(sdb, lambda f: _host_call(f, "ascii", hb)), f"{name}: host call on the clone")
        _check_rows(got, hb, sdb.n_branches, "clone")
        _oracle_check(name, odb, clone, got, hb)
        for i, b in enumerate(dq):
            _check_device(name, sdb, odb, clone, b, _device_once(clone, b), fresh, f"device call {i + 1} on the clone")
    finally:
        src.close()
        if clone is not None:
            clone.close()


def test_new_handle_after_one_used_on_several_streams_is_destroyed(dbs):
    """destroy a handle whose device-path calls (three streams) have been synchronised, then open another in the same process -- the
    allocator is likely to hand out the same addresses -- and use it"""
    import torch
    name = "dense"
    sdb, odb = dbs(name)
    queue = _device_queue(name, sdb, [33000, 1200, 34000], "n", 33000)
    hb = Batch("new_host", *synth.make_reads(sdb.alphabet, 2500, 150, seed=61, amb_rate=0.002, var_len=70), K=16)
    fresh = _FreshCache(sdb)
    host_want = _fresh(sdb, lambda f: _host_call(f, "ascii", hb))
    for b in queue:
        fresh.get(b)
    db = _open(sdb)
    try:
        pp = ra.PlacementProcess(db)
        preps = [_prepare(db, b) for b in queue]
        streams = [torch.cuda.Stream() for _ in queue]
        for s, b, kw in zip(streams, queue, preps):
            s.wait_stream(torch.cuda.current_stream())
            _launch(pp, b, kw, s.cuda_stream)
        _host_call(db, "ascii", hb)
        torch.cuda.synchronize()
    finally:
        db.close()
    for i, (b, kw) in enumerate(zip(queue, preps)):
        _same(_to_host(kw["out"]), fresh.get(b), f"call {i + 1} of the handle that was destroyed")
    db = _open(sdb)
    try:
        got = _host_call(db, "ascii", hb)
        _same(got, host_want, "host call on the new handle")
        _check_rows(got, hb, sdb.n_branches, "new handle")
        _oracle_check(name, odb, db, got, hb)
        for i, b in enumerate(queue):
            _check_device(name, sdb, odb, db, b, _device_once(db, b), fresh, f"device call {i + 1} on the new handle")
    finally:
        db.close()
