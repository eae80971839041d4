"""No GPU: the argument tests of the profile-only entry points (rk_place_batch_masses, rk_place_batch_packed_masses) that need no
handle.  A null handle and step = 4 are RK_ERR_INVALID with a message, and neither the mass buffer nor flags_out is written.  The
calls themselves are tested on the GPU (tests/test_gpu_masses_only.py)."""
import ctypes as C

import numpy as np

import rappas_amd as ra
from rappas_amd import _lib

POISON = np.uint64(0xA5A5A5A5DEADBEEF)
FLAG_POISON = np.uint32(0xDEADBEEF)


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_null_handle_and_step_4_are_invalid_and_touch_nothing():
    ra.build.build_engine()
    lib = _lib.load()
    n = 3
    seq = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTAC", np.uint8).copy()
    off = np.array([0, 10, 20, 30], np.uint64)
    packed, lens, flags = ra.pack_reads(_lib.RK_ALPHABET_DNA, 8, seq, off)
    m = np.full(2 * 99 + 4, POISON, np.uint64)
    fo = np.full(n, FLAG_POISON, np.uint32)
    ct = _lib.rk_counters(7, 7, 7, 7, 7, 7)
    p = _lib.rk_params(7, 0.01, _lib.RK_AMB_MEAN, float("-inf"))
    for step, word in ((0, b"handle"), (2, b"handle"), (3, b"handle"), (4, b"step"), (2 ** 32 - 1, b"step")):
        assert lib.rk_place_batch_masses(None, C.byref(p), step, n, ptr(seq), ptr(off), None, ptr(m), ptr(fo), C.byref(ct)) == _lib.RK_ERR_INVALID
        msg = lib.rk_last_error()
        assert b"rk_place_batch_masses" in msg and word in msg, (step, msg)
    assert lib.rk_place_batch_packed_masses(None, C.byref(p), n, ptr(packed), packed.shape[1], ptr(lens), 0, ptr(flags), None, None, None, ptr(m), ptr(fo),
                                            C.byref(ct)) == _lib.RK_ERR_INVALID
    assert b"rk_place_batch_packed_masses" in lib.rk_last_error()
    # keep_at_most outside 1..16 and a null mass buffer are found before the handle is looked at, too
    for K in (0, 17):
        bad = _lib.rk_params(K, 0.01, _lib.RK_AMB_MEAN, float("-inf"))
        assert lib.rk_place_batch_masses(None, C.byref(bad), 0, n, ptr(seq), ptr(off), None, ptr(m), ptr(fo), C.byref(ct)) == _lib.RK_ERR_INVALID
        assert b"keep_at_most" in lib.rk_last_error()
    assert lib.rk_place_batch_masses(None, C.byref(p), 0, n, ptr(seq), ptr(off), None, None, ptr(fo), C.byref(ct)) == _lib.RK_ERR_INVALID
    assert b"mass buffer" in lib.rk_last_error()
    assert (m == POISON).all() and (fo == FLAG_POISON).all()
    assert [getattr(ct, f) for f, _ in _lib.rk_counters._fields_] == [7] * 6


def test_the_python_wrappers_check_their_arrays_before_the_call():
    """a wrong-sized buffer must not reach a call that adds 2 * B + 4 words into it"""
    import types
    pp = ra.PlacementProcess.__new__(ra.PlacementProcess)
    pp.db = types.SimpleNamespace(info=types.SimpleNamespace(n_branches=99))
    w, m, f = pp._masses_args(5, None, None, None)
    assert w is None and m.dtype == np.uint64 and m.shape == (202,) and not m.any() and f.shape == (5,) and f.dtype == np.uint32
    for kw in (dict(masses=np.zeros(201, np.uint64)), dict(masses=np.zeros(202, np.int64)), dict(weights=np.zeros(4, np.uint32)),
               dict(weights=np.zeros(5, np.int32)), dict(flags_out=np.zeros(6, np.uint32))):
        args = dict(dict(weights=None, masses=None, flags_out=None), **kw)
        try:
            pp._masses_args(5, args["weights"], args["masses"], args["flags_out"])
        except ValueError:
            continue
        raise AssertionError(kw)
