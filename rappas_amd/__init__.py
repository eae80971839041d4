"""MI355X-native phylo-kmer placement engine for RAPPAS's `-p p` hot path.

The product is the C-ABI library `librappas_place.so` (include/rappas_place.h, gfx950 HIP kernels in
rappas_amd/csrc/).  This package is the thin host-side mirror used by tests and bench.py.
"""
from . import _lib, build, synth  # noqa: F401
from ._lib import (RK_ALPHABET_AA, RK_ALPHABET_DNA, RK_AMB_MAX, RK_AMB_MEAN, RK_AMB_SKIP, RK_FLAG_AMBIGUOUS,  # noqa: F401
                   RK_FLAG_BAD_CHAR, RK_FLAG_BELOW_NSBOUND, RK_FLAG_PLACED, RK_FLAG_REVERSE, RK_FLAG_TOO_LONG, RK_FLAG_TOO_SHORT, RK_FRAME_NONE,
                   RK_STEP_TRANSLATED, RK_STRAND_BOTH, RK_STRAND_FORWARD, RK_STRAND_REVERSE,
                   RK_TABLE_AUTO, RK_TABLE_DIRECT, RK_TABLE_DIRECT8, RK_TABLE_HASH, RkError)
from .placement import (EdgeTree, EdgePCA, PhyloKmerDB, PlacementProcess, Placements, accumulate_masses_host, clade_masses_host, kr_distances_host, accumulate_masses_samples_host, db_image_info,  # noqa: F401
                        host_alloc, masses_samples_words, masses_words, pack_reads, save_db_image, epca_finish, epca_host, edpl_host, tree_distance_host, squash_host, SQUASH_MERGE, kmeans_host, KMeans, KMEANS_NONE, diversity_host, diversity_math_host, diversity_columns, Diversity, translate_packed_host, translated_words, validate_db)
from .dbbuild import BuiltDB, build_db  # noqa: F401
from .edgestats import EdgeStats, edgestat, edgestat_batch, edgestat_columns, edgestat_finish, edgestat_host  # noqa: F401
