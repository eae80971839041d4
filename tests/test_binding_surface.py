"""The public surface of the Python binding, as a literal table: every name rappas_amd exports from placement and dbbuild, every public
method and property of PhyloKmerDB, PlacementProcess and EdgeTree with its signature, which of them carry a docstring, and the fields
of the records the calls return.  The table was printed once from the package and pasted here; a change of the binding that moves a
name, an argument or a default shows up as a difference from it.  No GPU and no library: only the package is imported."""
import ast
import dataclasses
import inspect
import os

import pytest

import rappas_amd as ra

# name -> (module, str(inspect.signature(...)) or None for a value, has a docstring)
EXPORTS = {
    "BuiltDB": ("dbbuild", "(alphabet: int, k: int, thr_log10: numpy.float32, key_codes: numpy.ndarray, row_offsets: numpy.ndarray, "
                "branch_ids: numpy.ndarray, scores: numpy.ndarray, tuples: int, visits: int, explore_ms: float, reduce_ms: float) -> None", True),
    "Diversity": ("placement", "(values, columns)", True),
    "EdgePCA": ("placement", "(eigenvalue, share, residual, projection, loading, n_active, k_eff)", True),
    "EdgeTree": ("placement", "(parent, branch_len, device=0)", True),
    "KMEANS_NONE": ("placement", None, False),
    "KMeans": ("placement", "(assign, dist, sizes, within, info, centroids)", True),
    "PhyloKmerDB": ("placement", "(alphabet, k, n_branches, thr_log10, thr, key_codes, row_offsets, branch_ids, scores, device=0, table_mode=0, "
                    "convert_uo=False)", True),
    "PlacementProcess": ("placement", "(db, ns_bound=-inf)", True),
    "Placements": ("placement", "(n_rows: numpy.ndarray, branch: numpy.ndarray, score: numpy.ndarray, lwr: numpy.ndarray, flags: numpy.ndarray, "
                   "counters: dict, frame: numpy.ndarray = None) -> None", True),
    "SQUASH_MERGE": ("placement", None, False),
    "accumulate_masses_host": ("placement", "(n_branches, placements, weights=None, masses=None, threads=0)", True),
    "accumulate_masses_samples_host": ("placement", "(n_branches, placements, n_samples, member_sample, member_read=None, member_weight=None, "
                                       "masses=None, threads=0)", True),
    "build_db": ("dbbuild", "(alphabet, k, states, pp_log10, node_branch, thr_log10, gap_off=None, gap_len=None, limit_to_1_jump=True, device=0)", True),
    "clade_masses_host": ("placement", "(parent, masses, n_samples)", True),
    "db_image_info": ("placement", "(path)", True),
    "diversity_columns": ("placement", "(theta)", True),
    "diversity_host": ("placement", "(parent, branch_len, masses, n_samples, theta=(), threads=0)", True),
    "diversity_math_host": ("placement", "(op, x, y=None)", True),
    "edpl_host": ("placement", "(parent, branch_len, keep_at_most, n_rows, branch, lwr, threads=0)", True),
    "epca_finish": ("placement", "(n_branches, n_samples, k, raw, info=None)", True),
    "epca_host": ("placement", "(parent, branch_len, masses, n_samples, k, iters, threads=0)", True),
    "host_alloc": ("placement", "(shape, dtype)", True),
    "kmeans_host": ("placement", "(parent, branch_len, masses, n_samples, k, max_rounds=100, seeds=None, centroids=True, threads=0)", True),
    "kr_distances_host": ("placement", "(parent, branch_len, masses, n_samples, threads=0)", True),
    "masses_samples_words": ("placement", "(n_branches, n_samples)", True),
    "masses_words": ("placement", "(n_branches)", True),
    "pack_reads": ("placement", "(alphabet, k, seq, seq_off, words_per_read=None, convert_uo=False, threads=0)", True),
    "save_db_image": ("placement", "(path, alphabet, k, n_branches, thr_log10, thr, key_codes, row_offsets, branch_ids, scores, table_mode=0, "
                      "convert_uo=False, user=b'')", True),
    "squash_host": ("placement", "(parent, branch_len, masses, n_samples, threads=0)", True),
    "translate_packed_host": ("placement", "(dna, frame, lens=None, fixed_len=0, aa_words=None)", True),
    "translated_words": ("placement", "(dna_len)", True),
    "tree_distance_host": ("placement", "(parent, branch_len, a, b)", True),
    "validate_db": ("placement", "(alphabet, k, n_branches, thr_log10, thr, key_codes, row_offsets, branch_ids, scores, table_mode=0, "
                    "convert_uo=False)", True),
}

_AMB = "treatAmbiguities=True, treatAmbiguitiesWithMax=False"
# class -> member -> (kind, signature or None, has a docstring)
CLASSES = {
    "EdgeTree": {
        "__init__": ("method", "(self, parent, branch_len, device=0)", False),
        "clade_masses": ("method", "(self, masses, n_samples, stream=None)", True),
        "close": ("method", "(self)", False),
        "diversity": ("method", "(self, masses, n_samples, theta=(), stream=None)", True),
        "diversity_batch": ("method", "(self, db, n_samples, theta=(), masses=None)", True),
        "diversity_work_bytes": ("method", "(self, n_samples, n_theta=0)", False),
        "edpl": ("method", "(self, out, keep_at_most, stream=None)", True),
        "edpl_batch": ("method", "(self, db, keep_at_most, n_rows, branch, lwr)", True),
        "edpl_lds_bytes": ("method", "(self)", True),
        "epca": ("method", "(self, masses, n_samples, k, iters, stream=None)", True),
        "epca_batch": ("method", "(self, db, n_samples, k, iters, masses=None)", True),
        "epca_work_bytes": ("method", "(self, n_samples, k)", False),
        "handle": ("property", None, False),
        "kmeans": ("method", "(self, masses, n_samples, k, max_rounds=100, seeds=None, centroids=False, stream=None)", True),
        "kmeans_batch": ("method", "(self, db, n_samples, k, max_rounds=100, masses=None, seeds=None, centroids=False)", True),
        "kmeans_work_bytes": ("method", "(self, n_samples, k)", False),
        "kr_distances": ("method", "(self, masses, n_samples, stream=None)", True),
        "kr_distances_batch": ("method", "(self, db, n_samples, masses=None)", True),
        "kr_work_bytes": ("method", "(self, n_samples)", False),
        "squash": ("method", "(self, masses, n_samples, stream=None)", True),
        "squash_batch": ("method", "(self, db, n_samples, masses=None)", True),
        "squash_work_bytes": ("method", "(self, n_samples)", False),
    },
    "PhyloKmerDB": {
        "__init__": ("method", "(self, alphabet, k, n_branches, thr_log10, thr, key_codes, row_offsets, branch_ids, scores, device=0, table_mode=0, "
                     "convert_uo=False)", False),
        "clone": ("method", "(self, device=0)", True),
        "close": ("method", "(self)", False),
        "fetch_row": ("method", "(self, code)", True),
        "from_synth": ("classmethod", "(cls, db, **kw)", False),
        "handle": ("property", None, False),
        "kernel_name": ("method", "(self)", False),
        "load": ("classmethod", "(cls, path, device=0)", True),
        "packed_words": ("method", "(self, max_len)", False),
        "save": ("method", "(self, path, user=b'')", True),
        "set_lanes_per_read": ("method", "(self, lanes)", False),
        "synthetic": ("classmethod", "(cls, spec, device=0, table_mode=0, convert_uo=False)", True),
    },
    "PlacementProcess": {
        "__init__": ("method", "(self, db, ns_bound=-inf)", False),
        "accumulate_masses": ("method", "(self, out, weights=None, masses=None, stream=None)", True),
        "accumulate_masses_samples": ("method", "(self, out, n_samples, member_sample, member_read=None, member_weight=None, masses=None, stream=None)", True),
        "count_work": ("method", "(self, packed, fixed_len=0, lens=None, flags_in=None, stream=None)", True),
        "pack_reads": ("method", "(self, seq_ascii, seq_off, max_len, stream=None)", False),
        "pack_reads_host": ("method", "(self, seq, seq_off, max_len=None, threads=0, out=None)", True),
        "place_packed": ("method", "(self, packed, fixed_len=0, lens=None, flags_in=None, seq_ascii=None, seq_off=None, out=None, keepAtMost=7, "
                         f"keepFactor=0.01, {_AMB}, stream=None, strand='forward')", True),
        "place_translated": ("method", "(self, dna, fixed_len=0, lens=None, flags_in=None, out=None, keepAtMost=7, keepFactor=0.01, stream=None)", True),
        "processQueries": ("method", f"(self, seq, seq_off, keepAtMost=7, keepFactor=0.01, {_AMB}, out=None, strand='forward')", True),
        "processQueriesMasses": ("method", "(self, seq, seq_off, weights=None, masses=None, strand='forward', translate=False, keepAtMost=7, "
                                 f"keepFactor=0.01, {_AMB}, flags_out=None)", True),
        "processQueriesMassesSamples": ("method", "(self, seq, seq_off, n_samples, member_sample, member_off=None, member_weight=None, masses=None, "
                                        f"strand='forward', translate=False, keepAtMost=7, keepFactor=0.01, {_AMB}, flags_out=None)", True),
        "processQueriesMulti": ("method", f"(self, dbs, seq, seq_off, keepAtMost=7, keepFactor=0.01, {_AMB}, out=None)", True),
        "processQueriesPacked": ("method", "(self, packed, lens=None, fixed_len=0, flags=None, seq=None, seq_off=None, keepAtMost=7, keepFactor=0.01, "
                                 f"{_AMB}, out=None)", True),
        "processQueriesPackedMasses": ("method", "(self, packed, lens=None, fixed_len=0, flags=None, seq=None, seq_off=None, weights=None, masses=None, "
                                       f"keepAtMost=7, keepFactor=0.01, {_AMB}, flags_out=None)", True),
        "processQueriesPackedMassesSamples": ("method", "(self, packed, n_samples, member_sample, member_off=None, member_weight=None, lens=None, "
                                              "fixed_len=0, flags=None, seq=None, seq_off=None, masses=None, keepAtMost=7, keepFactor=0.01, "
                                              f"{_AMB}, flags_out=None)", True),
        "processQueriesTranslated": ("method", "(self, seq, seq_off, keepAtMost=7, keepFactor=0.01, out=None)", True),
        "revcomp_ascii": ("method", "(self, seq_ascii, seq_off, stream=None)", True),
        "revcomp_packed": ("method", "(self, packed, fixed_len=0, lens=None, stream=None)", True),
        "translate_packed": ("method", "(self, dna, frame, fixed_len=0, lens=None, aa_words=None, stream=None)", True),
    },
}

FIELDS = {
    "Diversity": ["values", "columns"],
    "EdgePCA": ["eigenvalue", "share", "residual", "projection", "loading", "n_active", "k_eff"],
    "KMeans": ["assign", "dist", "sizes", "within", "info", "centroids"],
    "Placements": [("n_rows", None), ("branch", None), ("score", None), ("lwr", None), ("flags", None), ("counters", None), ("frame", "None")],
    "SQUASH_MERGE": [("a", "<u4"), ("b", "<u4"), ("size", "<u4"), ("reserved", "<u4"), ("distance", "<f8")],
}


def _signature(o):
    return str(inspect.signature(o)) if callable(o) else None


def _has_doc(o):
    return bool(getattr(o, "__doc__", None)) if inspect.isfunction(o) or inspect.isclass(o) else False


def _member(cls, name):
    """(kind, signature, has a docstring) of a class member, wherever in the class's bases it is written"""
    o = inspect.getattr_static(cls, name)
    if isinstance(o, property):
        return "property", None, bool(o.fget.__doc__)
    if isinstance(o, classmethod):
        return "classmethod", str(inspect.signature(o.__func__)), bool(o.__func__.__doc__)
    if inspect.isfunction(o):
        return "method", str(inspect.signature(o)), bool(o.__doc__)
    return "attr", None, False


def test_the_package_exports_the_same_names():
    src = open(os.path.join(os.path.dirname(ra.__file__), "__init__.py")).read()
    got = {a.name: node.module for node in ast.parse(src).body if isinstance(node, ast.ImportFrom) and node.module in ("placement", "dbbuild")
           for a in node.names}
    assert got == {n: mod for n, (mod, _, _) in EXPORTS.items()}


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_an_exported_name_keeps_its_signature_and_docstring(name):
    mod, sig, doc = EXPORTS[name]
    o = getattr(ra, name)
    assert getattr(o, "__module__", "rappas_amd." + mod) == "rappas_amd." + mod
    assert _signature(o) == sig
    assert _has_doc(o) or not doc


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_a_class_keeps_its_public_members(cls):
    c = getattr(ra, cls)
    public = {n for n in dir(c) if not n.startswith("_")} | {"__init__"}
    assert public == set(CLASSES[cls])
    for name, (kind, sig, doc) in CLASSES[cls].items():
        got_kind, got_sig, got_doc = _member(c, name)
        assert (got_kind, got_sig) == (kind, sig), name
        assert got_doc or not doc, name


def test_the_records_keep_their_fields():
    assert [(f.name, None if f.default is dataclasses.MISSING else repr(f.default)) for f in dataclasses.fields(ra.Placements)] == FIELDS["Placements"]
    for name in ("KMeans", "Diversity", "EdgePCA"):
        assert list(getattr(ra, name)._fields) == FIELDS[name]
    assert ra.SQUASH_MERGE.descr == FIELDS["SQUASH_MERGE"] and ra.SQUASH_MERGE.itemsize == 24
    assert ra.KMEANS_NONE == 0xFFFFFFFF
