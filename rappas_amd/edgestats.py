"""Edge dispersion and edge correlation with sample metadata (include/rappas_place.h), over the C ABI: for every edge
the mean and the spread of its mass share and of its imbalance across the samples of a sample mass buffer, and the Pearson and
Spearman correlation of both with every metadata column.

One call path per form -- edgestat (device tensors, asynchronous), edgestat_batch (the drivers' call) and edgestat_host (no GPU) --,
each returning the raw words and the two info words; edgestat_finish turns them into the one output table, an EdgeStats.  No compute
happens in Python and nothing here falls back to a CPU implementation.
"""
import collections

import numpy as np

from . import _lib
from .placement import _alloc, _grow, _host_samples, _or_error, _ptr, _stream, _torch

MAX_SAMPLES = 4096   # RK_EDGESTAT_MAX_SAMPLES
MAX_FEATURES = 8     # RK_EDGESTAT_MAX_FEATURES
COUNT_MAX_SAMPLES = 128  # RK_EDGESTAT_COUNT_MAX_SAMPLES: rows up to this many samples are ranked by counting, longer ones by a sort
FIXED_COLUMNS = ("mass_mean", "mass_var", "mass_sd", "mass_cv", "mass_vmr", "imb_mean", "imb_var", "imb_sd")
FEATURE_COLUMNS = ("mass_pearson", "mass_spearman", "imb_pearson", "imb_spearman")

# what edgestat_finish makes of a raw output: table float64 [B, 8 + 4F], columns its names, feature_table float64 [F, 2] (mean and
# population variance of every metadata column), n_active, unusable (the mask of the columns that are not finite in an active sample)
EdgeStats = collections.namedtuple("EdgeStats", "table columns feature_table n_active unusable")


def edgestat_columns(feature_names):
    """the column names of an edge-statistics table: the eight fixed ones, then mass_pearson_<name>, mass_spearman_<name>,
    imb_pearson_<name> and imb_spearman_<name> per metadata column"""
    names = list(FIXED_COLUMNS)
    for f in feature_names:
        names += [f"{c}_{f}" for c in FEATURE_COLUMNS]
    return tuple(names)


def _meta_host(meta, n_samples):
    """the metadata of a host or batch call as the C ABI reads it: float64 [F, S]; None or empty for no column"""
    if meta is None:
        return np.zeros((0, n_samples), np.float64)
    meta = np.ascontiguousarray(meta, dtype=np.float64)
    if meta.ndim == 1:
        meta = meta.reshape(1, -1) if meta.shape[0] else meta.reshape(0, n_samples)
    if meta.ndim != 2 or meta.shape[1] != n_samples:
        raise ValueError(f"meta must be [F, {n_samples}]: one row a metadata column, one value a sample")
    return meta


def _out_words(n_branches, n_features):
    n = int(_lib.load().rk_edgestat_out_words(n_branches, n_features))
    if not n:
        raise _lib.RkError(_lib.RK_ERR_INVALID, f"edge statistics: n_branches={n_branches}, n_features={n_features}: out of 1..65535, 0..{MAX_FEATURES}")
    return n


def edgestat_host(parent, masses, n_samples, meta=None, threads=0):
    """rk_edgestat_host (no GPU): (raw, info) -- the raw edge statistics of the samples of a sample mass buffer on the tree `parent`,
    uint64 [B * (6 + 4F) + 3F] words (doubles and int64 as include/rappas_place.h names them) and uint32 [2]: n_active, the mask of the
    unusable columns -- the bits edgestat gives on the device"""
    parent, _, B, masses = _host_samples(parent, None, masses, n_samples)
    meta = _meta_host(meta, n_samples)
    F = meta.shape[0]
    raw, info = np.zeros(_out_words(B, F) if F <= MAX_FEATURES else 1, np.uint64), np.zeros(2, np.uint32)
    _lib.check(_lib.load().rk_edgestat_host(B, _ptr(parent), n_samples, _ptr(masses), F, _ptr(meta) if F else None, _ptr(raw), _ptr(info), threads))
    return raw, info


def edgestat(tree, masses, n_samples, meta=None, stream=None):
    """rk_edgestat_device on an EdgeTree: (raw, info) as device tensors (int64 words, int32 [2]: the bits are unsigned), written;
    asynchronous on the stream.  `masses` is a device sample mass buffer; `meta` a float64 device tensor [F, S], or a host array, which
    is uploaded.  Uses the tree's workspace: calls on different streams that overlap in time need a tree each."""
    torch = _torch()
    dev = tree._masses(masses, n_samples)
    if meta is None or not hasattr(meta, "data_ptr"):
        meta = torch.from_numpy(_meta_host(meta, n_samples)).to(dev)
    if meta.dtype != torch.float64 or not meta.is_contiguous() or meta.device != dev or meta.dim() != 2 or meta.shape[1] != n_samples:
        raise ValueError(f"meta must be a contiguous float64 tensor [F, {n_samples}] on {dev}")
    F = int(meta.shape[0])
    lib = tree._lib
    work = _grow(tree, "_work_buf", dev, _or_error(lib, lib.rk_edgestat_work_bytes(tree.handle, n_samples, F)))
    raw, info = _alloc(_out_words(tree.n_branches, F), np.uint64, dev), _alloc(2, np.uint32, dev)
    _lib.check(lib.rk_edgestat_device(tree.handle, n_samples, masses.data_ptr(), F, meta.data_ptr() if F else None, raw.data_ptr(), info.data_ptr(),
                                      work.data_ptr(), work.numel(), _stream(dev, stream)))
    return raw, info


def edgestat_batch(tree, db, n_samples, meta=None, masses=None):
    """rk_edgestat_batch, the drivers' call: (raw, info) on the host from a host sample mass buffer -- or, masses None, from the buffer
    the last processQueriesMassesSamples call on `db` left on the device -- and host metadata [F, S], every value finite; returns when
    they are there"""
    masses = tree._batch_masses(n_samples, masses)
    meta = _meta_host(meta, n_samples)
    F = meta.shape[0]
    raw, info = np.zeros(_out_words(tree.n_branches, F) if F <= MAX_FEATURES else 1, np.uint64), np.zeros(2, np.uint32)
    _lib.check(tree._lib.rk_edgestat_batch(db.handle, tree.handle, n_samples, _ptr(masses), F, _ptr(meta) if F else None, _ptr(raw), _ptr(info)))
    return raw, info


def edgestat_finish(n_branches, n_samples, raw, info, feature_names=None):
    """rk_edgestat_finish_host: an EdgeStats from a raw output and its info words (host arrays, or device tensors, which are
    downloaded).  The number of metadata columns follows from the length of `raw`; feature_names names them (default "0", "1", ...).
    The only square roots of the edge statistics are here."""
    if hasattr(raw, "cpu"):
        raw = raw.cpu().numpy()
    if hasattr(info, "cpu"):
        info = info.cpu().numpy()
    raw = np.ascontiguousarray(raw).reshape(-1).view(np.uint64)
    info = np.ascontiguousarray(info).reshape(-1).view(np.uint32)
    F, rest = divmod(raw.shape[0] - 6 * n_branches, 4 * n_branches + 3)
    if n_branches < 1 or F < 0 or rest or info.shape[0] != 2:
        raise ValueError(f"raw holds {raw.shape[0]} words: not the edge statistics of {n_branches} branches (B * (6 + 4F) + 3F), or info not two words")
    names = tuple(str(f) for f in range(F)) if feature_names is None else tuple(feature_names)
    if len(names) != F:
        raise ValueError(f"{len(names)} feature names for {F} metadata columns")
    table, feature_table = np.zeros((n_branches, 8 + 4 * F)), np.zeros((F, 2))
    _lib.check(_lib.load().rk_edgestat_finish_host(n_branches, n_samples, F, _ptr(raw), _ptr(info), _ptr(table), _ptr(feature_table) if F else None))
    return EdgeStats(table, edgestat_columns(names), feature_table, int(info[0]), int(info[1]))
