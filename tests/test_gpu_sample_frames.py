"""The loops the sample kernels share at their own edges: the device against the host twins, word for word, for KR and edge PCA (the
tile loop of kr_pairs_kernel and epca_gram_kernel), squash and k-means (node_ring of rappas_amd/csrc/rk_samples.h), with the terms
and the chunk rule of rk_samplemath.h under all of them.  B = 7, 8, 9: the tail of a
stage of 8 nodes, the exact stage, a stage and a node; 31, 32, 33, 40, 63, 64: no ring group of 32 nodes, one group, a group and a
node, a group and a batch, a group and every other path; 128, 129: the k-means tile of rung 8 and a second tile of one node; 2048,
2056, 2080, 4096: one full chunk, a second chunk of exactly one stage or one group, two full chunks.  S = 2 and 65: one tile with two
samples, and a second tile, a second wave, of one sample."""
import functools

import numpy as np
import pytest

import rappas_amd as ra
from tests import epca_ref as E
from tests import kmeans_ref as K
from tests import kr_ref as R
from tests import squash_ref as Q
from tests.test_gpu_epca import device_raw
from tests.test_gpu_kmeans import download, to_dev
from tests.test_gpu_squash import device_rows

pytestmark = pytest.mark.gpu

SIZES = [7, 8, 9, 31, 32, 33, 40, 63, 64, 128, 129, 2048, 2056, 2080, 4096]
SAMPLES = [2, 65]
EPCA_K, KMEANS_ROUNDS = 3, 3


@functools.lru_cache(maxsize=None)
def case(B, S):
    """(parent, bl, the sample buffer) of one shape: ids out of pre-order"""
    parent, bl = R.random_tree(B, 800 + B)
    return parent, bl, R.sample_buffer(B, S, 900 + B + S)


@functools.lru_cache(maxsize=None)
def host_kr_epca(B, S):
    parent, bl, m = case(B, S)
    return ra.kr_distances_host(parent, bl, m, S), ra.epca_host(parent, bl, m, S, EPCA_K, 1)


@functools.lru_cache(maxsize=None)
def host_kmeans(B, S, k):
    parent, bl, m = case(B, S)
    return ra.kmeans_host(parent, bl, m, S, k, KMEANS_ROUNDS)


def check_kr_epca(et, dm, B, S, what):
    import torch
    want_D, (want_raw, want_info) = host_kr_epca(B, S)
    D = et.kr_distances(dm, S)
    torch.cuda.synchronize()
    assert (R.bits(D.cpu().numpy()) == R.bits(want_D)).all(), what
    raw, info = device_raw(et, dm, S, EPCA_K, 1)
    assert info.tolist() == want_info.tolist() and E.same(raw, want_raw), what


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("B", SIZES)
def test_device_equals_host_twins_word_for_word(B, S):
    parent, bl, m = case(B, S)
    et = ra.EdgeTree(parent, bl)
    try:
        dm = to_dev(m)
        check_kr_epca(et, dm, B, S, (B, S))
        rows, n = device_rows(et, dm, S)
        want_rows, n_want = ra.squash_host(parent, bl, m, S)
        assert n == n_want == S - 1 and Q.same_rows(rows, want_rows), (B, S)
        got = download(et.kmeans(dm, S, 3, KMEANS_ROUNDS, centroids=True))
        assert K.same(got, host_kmeans(B, S, 3)), (B, S, got.info)
    finally:
        et.close()


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("B", SIZES)
def test_kmeans_rungs_1_and_8(B, S, dev_lib, monkeypatch):
    """RK_KMEANS_KC (developer build) forces the rung: nine centroids are one group and a second of one centroid at rung 8"""
    parent, bl, m = case(B, S)
    want = host_kmeans(B, S, 9)
    for kc in ("1", "8"):
        monkeypatch.setenv("RK_KMEANS_KC", kc)
        et = ra.EdgeTree(parent, bl)
        try:
            got = download(et.kmeans(to_dev(m), S, 9, KMEANS_ROUNDS, centroids=True))
        finally:
            et.close()
        assert K.same(got, want), (B, S, kc, got.info)


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("B", [B for B in SIZES if B > 2048])
def test_both_forms_of_the_chunk_sum(B, S, dev_lib, monkeypatch):
    """RK_KR_PART_BYTES (developer build): the partials added in the block that holds both chunks, and through the workspace"""
    parent, bl, m = case(B, S)
    sizes = []
    for limit in ("0", str(1 << 28)):
        monkeypatch.setenv("RK_KR_PART_BYTES", limit)
        et = ra.EdgeTree(parent, bl)
        try:
            sizes.append(et.kr_work_bytes(S))
            check_kr_epca(et, to_dev(m), B, S, (B, S, limit))
        finally:
            et.close()
    assert sizes[1] == sizes[0] + 2 * S * S * 8  # two chunks of partials
