"""The numpy reference of the per-sample edge masses (include/rappas_place.h) and the membership lists the host and
the GPU tests share.  The definition restated: gather the entries of each sample and hand the gathered result set to masses_ref
(tests/masses_ref.py).  Nothing here comes from the engine.

A sample mass buffer for S samples on a tree of B branches is S * W + 1 uint64 words, W = 2 * B + 4: S mass buffers, then the count
of entries skipped because sample >= S or read >= n_reads."""
from types import SimpleNamespace

import numpy as np

from tests import masses_ref as MR


def words(B, S):
    return S * (2 * B + 4) + 1


def masses_samples_ref(B, S, s, member_sample, member_read=None, member_weight=None, masses=None):
    """`s`: a result set (n_rows [n], branch [n, K], lwr [n, K]).  member_read None: entry i is read i."""
    W = 2 * B + 4
    n = np.asarray(s.n_rows).shape[0]
    ms = np.asarray(member_sample, np.uint32).astype(np.int64)
    m = ms.shape[0]
    mr = np.arange(m, dtype=np.int64) if member_read is None else np.asarray(member_read, np.uint32).astype(np.int64)
    mw = None if member_weight is None else np.asarray(member_weight, np.uint32)
    out = np.zeros(S * W + 1, np.uint64) if masses is None else np.array(masses, dtype=np.uint64)
    ok = (ms < S) & (mr < n)
    out[S * W] += np.uint64(int((~ok).sum()))
    branch = np.asarray(s.branch, np.uint16).reshape(n, -1)
    lwr = np.asarray(s.lwr, np.float64).reshape(n, -1)
    order = np.argsort(np.where(ok, ms, S), kind="stable")
    bounds = np.searchsorted(np.where(ok, ms, S)[order], np.arange(S + 1))
    for smp in range(S):
        sel = order[bounds[smp]:bounds[smp + 1]]
        if sel.size == 0:
            continue
        rows = mr[sel]
        out[smp * W:(smp + 1) * W] = MR.masses_ref(B, np.asarray(s.n_rows)[rows], branch[rows], lwr[rows], None if mw is None else mw[sel],
                                                   masses=out[smp * W:(smp + 1) * W])
    return out


KINDS = ("identity", "runs", "interleaved", "csr")


def make_members(kind, n, m, S, seed=0, planted=True):
    """a membership list as a namespace: read (u32 [m'] or None), sample (u32 [m']), off (u64 [n + 1], the CSR over the reads, or None
    where the entries are not in read order), n_planted (entries out of range).
      identity     member_read None: entry r is read r, samples in runs (m is ignored: n entries)
      runs         m entries, sample i * S // m; the reads cycle over the first n - 7, so the last 7 sit in no sample and, with m > n,
                   some read sits in two
      interleaved  m entries, sample i mod S, the same reads
      csr          0 to 5 entries a read in read order (about m in all is not asked for), some (read, sample) pairs repeated
    planted: entries with sample == S, sample == 2^32 - 1 and (where reads are given) read == n."""
    rng = np.random.default_rng([seed, n, m, S, KINDS.index(kind)])
    off = None
    if kind == "identity":
        read, sample = None, (np.arange(n, dtype=np.int64) * S // n).astype(np.uint32)
    elif kind in ("runs", "interleaved"):
        i = np.arange(m, dtype=np.int64)
        read = (i % (n - 7)).astype(np.uint32)
        sample = (i * S // m if kind == "runs" else i % S).astype(np.uint32)
    else:
        counts = rng.integers(0, 6, n)
        counts[::9] = 0
        counts[1::9] = 5
        read = np.repeat(np.arange(n, dtype=np.uint32), counts)
        sample = rng.integers(0, S, int(counts.sum())).astype(np.uint32)
        first = np.concatenate([[0], np.cumsum(counts)[:-1]])
        firsts = first[counts > 0][:S]  # every sample is met: the first entries of the first reads name them in turn
        sample[firsts] = np.arange(len(firsts), dtype=np.uint32)
        rep = np.flatnonzero((counts >= 2) & (np.arange(n) % 4 == 1))  # the second entry of these reads repeats the first's sample
        sample[first[rep] + 1] = sample[first[rep]]
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    n_planted = 0
    if planted:
        sample = sample.copy()
        at = np.array([3, len(sample) // 2, len(sample) - 2])
        if kind == "csr":  # (kept away from the entries that make every sample non-empty)
            at = np.array([len(sample) // 2 + 1, len(sample) // 2 + 2, len(sample) - 2])
        sample[at[0]], sample[at[1]] = S, 2 ** 32 - 1
        n_planted = 2
        if read is not None:
            read = read.copy()
            if kind == "csr":  # a CSR cannot name a read beyond the batch: a third sample out of range instead
                sample[at[2]] = S + 1
            else:
                read[at[2]] = n
            n_planted = 3
    return SimpleNamespace(read=read, sample=sample, off=off, n_planted=n_planted)


def assert_not_trivial(mem, n, S):
    """every sample is non-empty; where the entries name their reads: some read sits in at least two samples and some read in none
    (the identity list has exactly one entry a read: only the first holds for it)"""
    ok = mem.sample.astype(np.int64) < S
    read = np.arange(len(mem.sample)) if mem.read is None else mem.read.astype(np.int64)
    ok &= read < n
    assert np.array_equal(np.unique(mem.sample[ok]), np.arange(S)), "an empty sample"
    if mem.read is None:
        return
    pairs = np.unique(np.stack([read[ok], mem.sample[ok].astype(np.int64)]), axis=1)
    per_read = np.bincount(pairs[0], minlength=n)
    assert per_read.max() >= 2 and per_read.min() == 0
