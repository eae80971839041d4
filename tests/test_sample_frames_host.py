"""The chunked walk of the host twins (chunk_walk of rappas_amd/csrc/rk_samples_host.h over the terms and the chunk rule of
rk_samplemath.h) at the edges of the device frames it is the twin of: rk_kr_distances_host against tests/kr_ref.py and rk_epca_host
against tests/epca_ref.py, bit for bit.  B on both sides of a stage of 8 nodes (7, 8, 9), of a ring group of 32 (31, 32, 33) and of a
chunk of 2048 (2048, 2049), and two full chunks (4096).  No GPU."""
import numpy as np
import pytest

import rappas_amd as ra

from tests import epca_ref as E
from tests import kr_ref as R

S = 3
SIZES = [7, 8, 9, 31, 32, 33, 2048, 2049, 4096]


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    """(parent, bl, the sample buffer) of one size: ids out of pre-order"""
    B = request.param
    parent, bl = R.random_tree(B, 600 + B)
    return parent, bl, R.sample_buffer(B, S, 700 + B)


def test_kr_host_twin_is_kr_ref_bit_for_bit(case):
    parent, bl, m = case
    want = R.kr_ref(parent, bl, m, S)
    got = ra.kr_distances_host(parent, bl, m, S)
    assert (R.bits(got) == R.bits(want)).all(), len(parent)
    assert (R.bits(got) == R.bits(got.T)).all() and (R.bits(np.diagonal(got)) == 0).all()


def test_epca_host_twin_is_epca_ref_bit_for_bit(case):
    """k = 2, iters = 1: the output is a direct function of G, so a wrong Gram entry shows"""
    parent, bl, m = case
    want, want_info = E.epca_ref(parent, bl, m, S, 2, 1)
    got, info = ra.epca_host(parent, bl, m, S, 2, 1)
    assert info.tolist() == want_info.tolist() == [S, 2]
    assert E.same(got, want), (len(parent), np.nonzero(R.bits(got) != R.bits(want))[0][:8])
