"""`python -m rappas_amd.tools.place`: FASTA queries + a --jsondb dump -> .jplace, through the GPU engine.

The reference's `-p p` phase for one query file (src/main_v2/Main_PLACEMENT_v07.java:150-320) with the database taken
from the JSON dump `--jsondb` writes (src/main_v2/SessionNext_v2.java:214-270) instead of the Java-serialized .union.
Only the placement itself runs on the GPU; ingest and the jplace writer are rappas_amd/hostio.py.
"""
import argparse
import contextlib
import os
import sys
from collections import namedtuple

import numpy as np

from .. import hostio
from ..placement import PhyloKmerDB, PlacementProcess


TRANSLATE_WITH_STRAND = "--translate places every read in all six reading frames, both strands included: it cannot be combined with --strand rev | both"
MASSES_ONLY_WITH_OUT = "--masses-only writes no jplace (the placements never reach the host): it cannot be combined with --out"
MASSES_ONLY_WITH_MASSES = "--masses-only writes the table --masses writes, without placing into a jplace: give one of the two"
KR_NEEDS_SAMPLE_SEP = "--kr compares the samples of one run: it needs --sample-sep (with --masses or --masses-only)"
SQUASH_NEEDS_SAMPLE_SEP = "--squash clusters the samples of one run: it needs --sample-sep (with --masses or --masses-only)"
EPCA_NEEDS_SAMPLE_SEP = "--epca finds the principal components of the samples of one run: it needs --sample-sep (with --masses or --masses-only)"
EPCA_RANGES = "--epca-components must be in 1..8, --epca-iters in 1..10000"
KMEANS_NEEDS_SAMPLE_SEP = "--kmeans clusters the samples of one run: it needs --sample-sep (with --masses or --masses-only)"
KMEANS_RANGES = "--kmeans needs --kmeans-k in 1..64; --kmeans-rounds must be in 1..1024"
DIVERSITY_NEEDS_SAMPLE_SEP = "--diversity measures the samples of one run: it needs --sample-sep (with --masses or --masses-only)"
DIVERSITY_RANGES = "--diversity-theta takes at most 8 numbers in 0..8, separated by commas"
EDGE_STATS_NEEDS_SAMPLE_SEP = "--edge-stats relates the edges to the samples of one run: it needs --sample-sep (with --masses or --masses-only)"
METADATA_NEEDS_EDGE_STATS = "--metadata names the sample metadata of the edge statistics: it needs --edge-stats"
EDPL_NEEDS_OUT ="--edpl reads the placements of a run that writes a jplace: it needs --out (and cannot be combined with --masses-only)"
SAMPLE_SEP_NEEDS_MASSES = "--sample-sep names the samples of the per-edge tables: it needs --masses or --masses-only"
TRANSLATE_NEEDS_AA = "--translate needs an amino-acid database (this one holds DNA: DNA reads are placed on it as they are, see --strand)"


@contextlib.contextmanager
def _edge_tree(tree, device=0, wanted=True):
    """the database's tree (a hostio tree) on the device, as the reports and --edpl take it; None if no one wants it"""
    if not wanted:
        yield None
        return
    from ..placement import EdgeTree
    et = EdgeTree([n.parent.id if n.parent is not None else -1 for n in tree.nodes], [n.bl for n in tree.nodes], device=device)
    try:
        yield et
    finally:
        et.close()


def _with_mass(et, n_samples, host_words):
    W = 2 * et.n_branches + 4
    host_words = np.asarray(host_words, dtype=np.uint64).reshape(-1)
    return [bool(host_words[s * W:s * W + et.n_branches].any()) for s in range(n_samples)]


# The sample reports of --sample-sep, a row each: text(edge_tree, db, sample_names, words, host_words, options) over a sample mass buffer
# and the database's tree -- words None: the buffer the per-sample profile-only call left on the device in `db`; host_words: the
# host's copy either way (it tells which samples hold mass); options: place_file's keywords of the reports
def _kr_report(et, db, names, words, host_words, o):
    return hostio.kr_table(names, et.kr_distances_batch(db, len(names), words))


def _squash_report(et, db, names, words, host_words, o):
    from ..placement import SQUASH_MERGE
    merges, n_merges = et.squash_batch(db, len(names), words) if len(names) > 1 else (np.zeros(0, SQUASH_MERGE), 0)
    return hostio.squash_table(names, merges, n_merges, _with_mass(et, len(names), host_words))


def _epca_report(et, db, names, words, host_words, o):
    from ..placement import epca_finish
    S, B, k, iters = len(names), et.n_branches, o["epca_components"], o["epca_iters"]
    if S < 2:  # one sample alone has no components: it is only counted
        return hostio.epca_table(names, B, k, iters, sum(_with_mass(et, S, host_words)), 0, np.zeros(k), np.zeros(k), np.zeros(k), np.zeros((S, k)), np.zeros((B, k)))
    raw, info = et.epca_batch(db, S, k, iters, words)
    f = epca_finish(B, S, k, raw, info)
    return hostio.epca_table(names, B, k, iters, f.n_active, f.k_eff, f.eigenvalue, f.share, f.residual, f.projection, f.loading)


def _kmeans_report(et, db, names, words, host_words, o):
    r = et.kmeans_batch(db, len(names), o["kmeans_k"], o["kmeans_rounds"], words)
    return hostio.kmeans_table(names, o["kmeans_k"], r.assign, r.dist, r.sizes, r.within, r.info)


def _diversity_report(et, db, names, words, host_words, o):
    return hostio.diversity_table(names, o["diversity_theta"], et.diversity_batch(db, len(names), o["diversity_theta"], words).values)


def _edge_stats_report(et, db, names, words, host_words, o):
    from .. import edgestats
    features = o["metadata"][0] if o["metadata"] is not None else []
    raw, info = edgestats.edgestat_batch(et, db, len(names), o["edge_stats_meta"], words)
    r = edgestats.edgestat_finish(et.n_branches, len(names), raw, info, features)
    return hostio.edge_stats_table(names, features, r.n_active, r.table, r.feature_table)


def _thetas_in_range(theta):
    return len(theta) <= 8 and all(0.0 <= t <= 8.0 for t in theta)


# name: the option `--name FILE`, the keyword of place_file and the attribute of its result; in_range(options): its own options, if any
Report = namedtuple("Report", "name needs_sample_sep in_range ranges text")
SAMPLE_REPORTS = (
    Report("kr", KR_NEEDS_SAMPLE_SEP, None, None, _kr_report),
    Report("squash", SQUASH_NEEDS_SAMPLE_SEP, None, None, _squash_report),
    Report("epca", EPCA_NEEDS_SAMPLE_SEP, lambda o: 1 <= o["epca_components"] <= 8 and 1 <= o["epca_iters"] <= 10000, EPCA_RANGES, _epca_report),
    Report("kmeans", KMEANS_NEEDS_SAMPLE_SEP, lambda o: 1 <= o["kmeans_k"] <= 64 and 1 <= o["kmeans_rounds"] <= 1024, KMEANS_RANGES, _kmeans_report),
    Report("diversity", DIVERSITY_NEEDS_SAMPLE_SEP, lambda o: _thetas_in_range(o["diversity_theta"]), DIVERSITY_RANGES, _diversity_report),
    Report("edge_stats", EDGE_STATS_NEEDS_SAMPLE_SEP, None, None, _edge_stats_report),
)


def _check_reports(requested, with_samples, options):
    """ValueError with the sentence of the first rule a requested report breaks, in the table's order"""
    for r in SAMPLE_REPORTS:
        if requested[r.name] and not with_samples:
            raise ValueError(r.needs_sample_sep)
        if requested[r.name] and r.in_range is not None and not r.in_range(options):
            raise ValueError(r.ranges)


def _parse_metadata(requested, metadata):
    """the text of `--metadata TSV` parsed (hostio.parse_metadata) before anything is opened; None without one"""
    if metadata is not None and not requested["edge_stats"]:
        raise ValueError(METADATA_NEEDS_EDGE_STATS)
    return hostio.parse_metadata(metadata) if metadata is not None else None


def _sample_metadata(requested, options, sample_names):
    """after the FASTA scan and before placing: the metadata of the run's samples [F, S] -- every sample must have a line"""
    if requested["edge_stats"]:
        options["edge_stats_meta"] = hostio.metadata_of_samples(sample_names, options["metadata"])


def _run_reports(et, db, sample_names, words, host_words, requested, options):
    """{name: text, or None if not requested} of every report"""
    return {r.name: r.text(et, db, sample_names, words, host_words, options) if requested[r.name] else None for r in SAMPLE_REPORTS}


def kr_text(db, tree, sample_names, words, device=0):
    """`--kr FILE`: the table (hostio.kr_table) of the pairwise KR distances between the samples of a sample mass buffer over the
    database's tree -- words None: the buffer the per-sample profile-only call left on the device in `db`"""
    with _edge_tree(tree, device) as et:
        return _kr_report(et, db, sample_names, words, None, None)


def squash_text(db, tree, sample_names, words, host_words, device=0):
    """`--squash FILE`: the table (hostio.squash_table) of the squash clustering of the samples, as kr_text; host_words: the host's copy
    of the buffer either way (it tells which samples hold mass)"""
    with _edge_tree(tree, device) as et:
        return _squash_report(et, db, sample_names, words, host_words, None)


def epca_text(db, tree, sample_names, words, host_words, k, iters, device=0):
    """`--epca FILE`: the table (hostio.epca_table) of the edge principal components of the samples, as squash_text"""
    with _edge_tree(tree, device) as et:
        return _epca_report(et, db, sample_names, words, host_words, dict(epca_components=k, epca_iters=iters))


def kmeans_text(db, tree, sample_names, words, k, max_rounds, device=0):
    """`--kmeans FILE`: the table (hostio.kmeans_table) of the phylogenetic k-means of the samples, as kr_text"""
    with _edge_tree(tree, device) as et:
        return _kmeans_report(et, db, sample_names, words, None, dict(kmeans_k=k, kmeans_rounds=max_rounds))


def diversity_text(db, tree, sample_names, words, theta, device=0):
    """`--diversity FILE`: the table (hostio.diversity_table) of the diversity measures of the samples, as kr_text"""
    with _edge_tree(tree, device) as et:
        return _diversity_report(et, db, sample_names, words, None, dict(diversity_theta=theta))


def edge_stats_text(db, tree, sample_names, words, metadata=None, device=0):
    """`--edge-stats FILE`: the table (hostio.edge_stats_table) of the edge dispersion of the samples and of the edge correlation with
    the sample metadata (the text of a `--metadata TSV`, or None), as kr_text"""
    parsed = hostio.parse_metadata(metadata) if metadata is not None else None
    with _edge_tree(tree, device) as et:
        return _edge_stats_report(et, db, sample_names, words, None, dict(metadata=parsed, edge_stats_meta=hostio.metadata_of_samples(sample_names, parsed)))


def _edpl_report(et, db, records, unique, res, keep_at_most):
    return hostio.edpl_table(records, unique, res.n_rows, et.edpl_batch(db, keep_at_most, res.n_rows, res.branch, res.lwr))


def edpl_text(db, tree, records, unique, res, keep_at_most, device=0):
    """`--edpl FILE`: the table (hostio.edpl_table) of the EDPL of every placed read of a result set on the host, over the database's
    tree, through rk_edpl_batch on db's device"""
    with _edge_tree(tree, device) as et:
        return _edpl_report(et, db, records, unique, res, keep_at_most)


def parse_thetas(text):
    """the values of `--diversity-theta T1,T2,...` (None or empty: none); ValueError(DIVERSITY_RANGES) for what the engine would refuse"""
    if text is None or text == "":
        return ()
    try:
        theta = tuple(float(t) for t in text.split(","))
    except ValueError:
        raise ValueError(DIVERSITY_RANGES) from None
    if not _thetas_in_range(theta):
        raise ValueError(DIVERSITY_RANGES)
    return theta


def place_file(db_text, fasta_text, keep_at_most=7, keep_factor=0.01, amb="mean", ns_bound=float("-inf"), guppy=False,
               call_string="", device=0, union=False, dbimage=None, save_dbimage=None, strand="fwd", translate=False, masses=False, sample_sep=None, kr=False,
               squash=False, epca=False, epca_components=5, epca_iters=200, edpl=False, kmeans=False, kmeans_k=0, kmeans_rounds=100, diversity=False, diversity_theta=(), edge_stats=False,
               metadata=None):
    """db_text: the bytes of a --jsondb dump, or (union=True) of a Java-serialized .union database; or dbimage = the path of the
    engine's own image file (rk_db_load: mmap + upload, the reference tree in its user blob).  strand: "fwd" (the reference's
    behaviour), "rev" or "both" (DNA: reads placed from their reverse complement / on the better strand; res.reversed is then the text of
    reversed_<query>.tsv).  translate: DNA reads on an amino-acid database, six reading frames translated on the device and the best
    one reported per read (res.frames is then the text of frames_<query>.tsv); not together with strand "rev" / "both".  masses: res.masses is
    then the text of the per-edge table `--masses FILE` writes (hostio.masses_table; a read weighs the number of FASTA records it stands for);
    with sample_sep (one character) one table per sample (hostio.sample_members, hostio.masses_samples_table), and then for every
    report of SAMPLE_REPORTS asked for by its name (kr, squash, epca, kmeans, diversity, edge_stats) res.<name> is the text
    `--<name> FILE` writes, with the report's own keywords (epca_components components after epca_iters iterations; kmeans_k clusters and
    at most kmeans_rounds rounds; the thetas diversity_theta; metadata, the text of the `--metadata TSV` of the edge statistics).  edpl: res.edpl is the text `--edpl FILE` writes (edpl_text), with any strand
    and with translate."""
    if translate and strand != "fwd":
        raise ValueError(TRANSLATE_WITH_STRAND)
    requested = dict(kr=kr, squash=squash, epca=epca, kmeans=kmeans, diversity=diversity, edge_stats=edge_stats)
    options = dict(epca_components=epca_components, epca_iters=epca_iters, kmeans_k=kmeans_k, kmeans_rounds=kmeans_rounds, diversity_theta=diversity_theta)
    _check_reports(requested, masses and sample_sep is not None, options)
    options["metadata"] = _parse_metadata(requested, metadata)
    db, tree = _open_db(db_text, union, dbimage, save_dbimage, device)
    sample_words = None
    try:
        if translate and db.info.alphabet != 20:
            raise ValueError(TRANSLATE_NEEDS_AA)
        records = hostio.read_fasta(fasta_text)
        unique, names = hostio.dedup_reads(records)
        members = hostio.sample_members(records, unique, sample_sep) if masses and sample_sep is not None else None
        if members is not None:
            _sample_metadata(requested, options, members[0])
        seq, off = hostio.pack_batch([s for _, s in unique])
        if translate:
            res = PlacementProcess(db, ns_bound).processQueriesTranslated(seq, off, keepAtMost=keep_at_most, keepFactor=keep_factor)
        else:
            res = PlacementProcess(db, ns_bound).processQueries(
                seq, off, keepAtMost=keep_at_most, keepFactor=keep_factor, treatAmbiguities=(amb != "skip"),
                treatAmbiguitiesWithMax=(amb == "max"), strand=strand)
        reports = dict.fromkeys(requested)
        with _edge_tree(tree, device, edpl or any(requested.values())) as et:
            res.edpl = _edpl_report(et, db, records, unique, res, keep_at_most) if edpl else None
            if members is not None:
                from ..placement import accumulate_masses_samples_host
                sample_names, m_off, m_sample, m_weight = members
                m_read = np.repeat(np.arange(len(unique), dtype=np.uint32), np.diff(m_off.astype(np.int64)))
                sample_words = accumulate_masses_samples_host(len(tree.nodes), res, len(sample_names), m_sample, member_read=m_read, member_weight=m_weight)
                reports = _run_reports(et, db, sample_names, sample_words, sample_words, requested, options)
    finally:
        db.close()
    for name, text in reports.items():
        setattr(res, name, text)
    pl = hostio.jplace_placements(tree, names, res.n_rows, res.branch, res.score, res.lwr, guppy)
    res.notplaced = hostio.notplaced_log(records, unique, (res.flags & 1) != 0)
    res.reversed = hostio.reversed_log(records, unique, res.flags) if strand != "fwd" else None
    res.frames = hostio.frames_log(records, unique, res.frame) if translate else None
    res.masses = None
    if members is not None:
        res.masses = hostio.masses_samples_table(tree, members[0], sample_words)
    elif masses:
        from ..placement import accumulate_masses_host
        weights = np.array([len(nm) for nm in names], dtype=np.uint32)
        res.masses = hostio.masses_table(tree, accumulate_masses_host(len(tree.nodes), res, weights))
    return hostio.jplace_document(tree, pl, call_string, guppy), res


def masses_only_file(db_text, fasta_text, keep_at_most=7, keep_factor=0.01, amb="mean", ns_bound=float("-inf"), device=0, union=False,
                     dbimage=None, save_dbimage=None, strand="fwd", translate=False, sample_sep=None, kr=False, squash=False, epca=False, epca_components=5,
                     epca_iters=200, kmeans=False, kmeans_k=0, kmeans_rounds=100, diversity=False, diversity_theta=(), edge_stats=False, metadata=None):
    """`--masses-only FILE`: scan, dedup and gather as place_file, then ONE profile-only call (processQueriesMasses) with the
    multiplicities as weights: the placements are summed on the device and only the flags come back.  -> a namespace with .masses (the
    table's text, what place_file(masses=True) gives), .notplaced, .reversed (strand "rev" / "both", else None), .flags and .counters.
    No jplace and no frames log: the rows and the frame bytes never reach the host.  With sample_sep (one character) the one call is
    processQueriesMassesSamples with the membership of hostio.sample_members, and .masses holds one table per sample; the reports of
    SAMPLE_REPORTS are then asked for as of place_file (.kr, .squash, .epca, .kmeans, .diversity, .edge_stats), each from the buffer that call left
    on the device."""
    from types import SimpleNamespace
    if translate and strand != "fwd":
        raise ValueError(TRANSLATE_WITH_STRAND)
    requested = dict(kr=kr, squash=squash, epca=epca, kmeans=kmeans, diversity=diversity, edge_stats=edge_stats)
    options = dict(epca_components=epca_components, epca_iters=epca_iters, kmeans_k=kmeans_k, kmeans_rounds=kmeans_rounds, diversity_theta=diversity_theta)
    _check_reports(requested, sample_sep is not None, options)
    options["metadata"] = _parse_metadata(requested, metadata)
    reports = dict.fromkeys(requested)
    db, tree = _open_db(db_text, union, dbimage, save_dbimage, device)
    try:
        if translate and db.info.alphabet != 20:
            raise ValueError(TRANSLATE_NEEDS_AA)
        records = hostio.read_fasta(fasta_text)
        unique, names = hostio.dedup_reads(records)
        seq, off = hostio.pack_batch([s for _, s in unique])
        weights = np.array([len(nm) for nm in names], dtype=np.uint32)
        common = dict(strand=strand, translate=translate, keepAtMost=keep_at_most, keepFactor=keep_factor, treatAmbiguities=(amb != "skip"),
                      treatAmbiguitiesWithMax=(amb == "max"))
        if sample_sep is not None:
            sample_names, m_off, m_sample, m_weight = hostio.sample_members(records, unique, sample_sep)
            _sample_metadata(requested, options, sample_names)
            words, flags, counters = PlacementProcess(db, ns_bound).processQueriesMassesSamples(
                seq, off, len(sample_names), m_sample, member_off=m_off, member_weight=m_weight, **common)
            table = hostio.masses_samples_table(tree, sample_names, words)
            with _edge_tree(tree, device, any(requested.values())) as et:
                reports = _run_reports(et, db, sample_names, None, words, requested, options)
        else:
            words, flags, counters = PlacementProcess(db, ns_bound).processQueriesMasses(seq, off, weights=weights, **common)
            table = hostio.masses_table(tree, words)
    finally:
        db.close()
    return SimpleNamespace(masses=table, notplaced=hostio.notplaced_log(records, unique, (flags & 1) != 0),
                           reversed=hostio.reversed_log(records, unique, flags) if strand != "fwd" else None, flags=flags, counters=counters, **reports)


def _open_db(db_text, union, dbimage, save_dbimage, device):
    """(handle, reference tree) of a --jsondb / --uniondb text or of an image file"""
    if dbimage is not None:
        from ..placement import db_image_info
        _, blob = db_image_info(dbimage)
        tree = hostio.tree_from_blob(blob)
        db = PhyloKmerDB.load(dbimage, device=device)
        if db.info.n_branches != len(tree.nodes):
            raise ValueError("database image: tree and database disagree on the number of branches")
    else:
        d = hostio.load_uniondb(db_text) if union else hostio.load_jsondb(db_text)
        tree = d["tree"]
        if save_dbimage is not None:
            from ..placement import save_db_image
            save_db_image(save_dbimage, d["alphabet"], d["k"], d["n_branches"], d["thr_log10"], d["thr"], d["key_codes"], d["row_offsets"],
                          d["branch_ids"], d["scores"], convert_uo=d.get("convert_uo", False), user=hostio.tree_to_blob(tree))
        db = PhyloKmerDB(d["alphabet"], d["k"], d["n_branches"], d["thr_log10"], d["thr"], d["key_codes"], d["row_offsets"],
                         d["branch_ids"], d["scores"], device=device, convert_uo=d.get("convert_uo", False))
    return db, tree


def _write_outputs(a, res, base_path):
    """every file of a run but the jplace: the per-edge table, the reports, --edpl, and the logs under --logs (default: logs/ next to
    base_path, like the reference's workdir/logs); a text that is None, or that this kind of run does not have, is not written"""
    files = [(a.masses if a.masses_only is None else a.masses_only, res.masses), (a.edpl, getattr(res, "edpl", None))]
    files += [(getattr(a, r.name), getattr(res, r.name)) for r in SAMPLE_REPORTS]
    logs = a.logs if a.logs is not None else os.path.join(os.path.dirname(os.path.abspath(base_path)), "logs")
    os.makedirs(logs, exist_ok=True)
    files += [(os.path.join(logs, kind + "_" + os.path.basename(a.fasta) + ".tsv"), getattr(res, kind, None)) for kind in ("notplaced", "reversed", "frames")]
    for path, text in files:
        if text is not None:
            with open(path, "w") as f:
                f.write(text)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="rappas_amd.tools.place", description=__doc__.splitlines()[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--jsondb", help="database dump written by the reference's --jsondb")
    g.add_argument("--uniondb", help="the reference's own database file (DB.union, Java serialization; SessionNext_v2.java:109-207)")
    g.add_argument("--dbimage", help="the engine's own database image (written by --save-dbimage / rk_db_save): mmap + upload, no parse")
    ap.add_argument("--save-dbimage", default=None, help="with --jsondb / --uniondb: also write the database as an image file")
    ap.add_argument("--fasta", required=True, help="query reads (-q)")
    ap.add_argument("--out", default=None, help="output .jplace (required unless --masses-only is given)")
    ap.add_argument("--keep-at-most", type=int, default=7)
    ap.add_argument("--keep-factor", type=float, default=0.01)
    ap.add_argument("--amb", choices=["mean", "max", "skip"], default="mean", help="--ambwithmax / --noamb")
    ap.add_argument("--nsbound", type=float, default=float("-inf"))
    ap.add_argument("--strand", choices=["fwd", "rev", "both"], default="fwd",
                    help="DNA: place the reads as given (default, the reference's behaviour), their reverse complements, or both and keep "
                         "the better strand per read; rev / both also write logs/reversed_<query>.tsv")
    ap.add_argument("--translate", action="store_true",
                    help="amino-acid database, DNA reads: translate every read in its six reading frames on the device (standard genetic "
                         "code, longest stop-free run per frame) and report the best frame; also writes logs/frames_<query>.tsv "
                         "(header<TAB>+1|+2|+3|-1|-2|-3); not with --strand rev | both")
    ap.add_argument("--masses", default=None, metavar="FILE",
                    help="also write the per-edge table of the run: one line per tree node with the reads whose best placement is its edge and "
                         "the likelihood weight on it, and the same summed over its clade; a read counts once per FASTA record")
    ap.add_argument("--masses-only", default=None, metavar="FILE",
                    help="profile-only run: write that table to FILE and nothing else but the notplaced (and, with --strand rev | both, the "
                         "reversed) log -- the placements are summed on the device and never reach the host, so no jplace is written, "
                         "--out may not be given, and with --translate the frames log is not written (the frame bytes do not come back); "
                         "not with --masses")
    ap.add_argument("--sample-sep", default=None, metavar="C",
                    help="with --masses or --masses-only: one table per sample in FILE.  A record's sample is its header up to the first "
                         "character C (a header without C is an error), samples are numbered in byte-wise order of their names, and a read "
                         "counts in every sample once per record of that sample; FILE holds, for each sample, a line "
                         "#sample<TAB>name<TAB>index and its table, and a last line #skipped_entries<TAB>n")
    ap.add_argument("--kr", default=None, metavar="FILE",
                    help="with --sample-sep: the pairwise Kantorovich-Rubinstein distances between the samples' edge masses, summed on the "
                         "device: a line #kr<TAB>S, a line per sample with its name and S distances (%%.17g), and a last line "
                         "#samples_without_mass<TAB>n; a sample without mass has nan in its row and column")
    ap.add_argument("--squash", default=None, metavar="FILE",
                    help="with --sample-sep: the squash clustering of the samples over those distances, merged on the device: a line "
                         "#squash<TAB>S<TAB>n_merges, a line k<TAB>a<TAB>b<TAB>distance<TAB>size per merge, the tree as #newick<TAB>...; "
                         "(an inner node at half its distance), #inversions<TAB>n and #samples_without_mass<TAB>n")
    ap.add_argument("--epca", default=None, metavar="FILE",
                    help="with --sample-sep: the edge principal components of the samples (the difference between the mass on the two sides "
                         "of every edge, centred), found on the device: a line #epca<TAB>S<TAB>B<TAB>k<TAB>n_active<TAB>k_eff<TAB>iters, the "
                         "lines #eigenvalue, #share, #residual (k values each, %%.17g), #projections and a line per sample, #loadings and a "
                         "line per node id, and a last line #samples_without_mass<TAB>n")
    ap.add_argument("--epca-components", type=int, default=5, metavar="K", help="--epca: the number of components, 1..8 (default 5)")
    ap.add_argument("--epca-iters", type=int, default=200, metavar="N", help="--epca: the fixed number of iterations, 1..10000 (default 200)")
    ap.add_argument("--kmeans", default=None, metavar="FILE",
                    help="with --sample-sep and --kmeans-k: the phylogenetic k-means of the samples (clusters whose centroids are the averages "
                         "of their members' mass, KR distances, farthest-first seeds), found on the device: a line "
                         "#kmeans<TAB>S<TAB>k<TAB>k_eff<TAB>n_active<TAB>rounds<TAB>converged, #clusters and a line j<TAB>size<TAB>within per "
                         "cluster, #samples and a line name<TAB>cluster<TAB>distance per sample (- and 0 without mass), and a last line "
                         "#samples_without_mass<TAB>n")
    ap.add_argument("--kmeans-k", type=int, default=0, metavar="K", help="--kmeans: the number of clusters, 1..64")
    ap.add_argument("--kmeans-rounds", type=int, default=100, metavar="N", help="--kmeans: the most rounds run, 1..1024 (default 100)")
    ap.add_argument("--diversity", default=None, metavar="FILE",
                    help="with --sample-sep: the phylogenetic diversity of every sample (what guppy fpd reports), summed on the device: a line "
                         "#diversity<TAB>S<TAB>n_theta, a line #columns with rooted_pd, pd, bwpd, quadratic, phylo_entropy and, per theta, "
                         "rooted_pd_<theta> and bwpd_<theta>, a line name<TAB>values (%%.17g) per sample (nan without mass), and a last line "
                         "#samples_without_mass<TAB>n")
    ap.add_argument("--diversity-theta", default=None, metavar="T1,T2,...", help="--diversity: at most 8 exponents in 0..8 for the one-parameter families")
    ap.add_argument("--edge-stats", default=None, metavar="FILE",
                    help="with --sample-sep: edge dispersion and edge correlation, found on the device: for every edge the mean, variance, "
                         "standard deviation, coefficient of variation and variance-to-mean ratio of its mass share across the samples, mean, "
                         "variance and standard deviation of its imbalance, and per metadata column the Pearson and Spearman correlation of "
                         "both: a line #edge_stats<TAB>S<TAB>B<TAB>F<TAB>n_active, a line #columns, a line per node id (%%.17g, nan), #features "
                         "and a line name<TAB>mean<TAB>variance per column, and a last line #samples_without_mass<TAB>n; at most 4096 samples")
    ap.add_argument("--metadata", default=None, metavar="TSV",
                    help="--edge-stats: the sample metadata, a first line sample<TAB>name_1<TAB>...<TAB>name_F (F <= 8) and a line per sample "
                         "with its name and F finite numbers; every sample of the run needs a line, lines of other samples are ignored")
    ap.add_argument("--edpl", default=None, metavar="FILE",
                    help="with --out: the EDPL of every placed read (the expected distance between its placement locations: the sum over the "
                         "pairs of its rows of LWR x LWR x the tree path between the midpoints of the two edges), computed on the device: a "
                         "line #edpl<TAB>n_lines, then header<TAB>edpl (%%.17g) per FASTA record that has a placement, in input order; "
                         "not with --masses-only")
    ap.add_argument("--timing", action="store_true", help="--masses-only: one JSON line with the run's wall-clock times on stdout")
    ap.add_argument("--guppy-compat", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--logs", default=None, help="directory of notplaced_<query>.tsv (default: logs/ next to --out, like the reference's workdir/logs)")
    a = ap.parse_args(argv)
    requested = {r.name: getattr(a, r.name) is not None for r in SAMPLE_REPORTS}
    options = dict(epca_components=a.epca_components, epca_iters=a.epca_iters, kmeans_k=a.kmeans_k, kmeans_rounds=a.kmeans_rounds, diversity_theta=())
    if a.translate and a.strand != "fwd":
        ap.error(TRANSLATE_WITH_STRAND)
    if a.masses_only is not None and a.masses is not None:
        ap.error(MASSES_ONLY_WITH_MASSES)
    if a.masses_only is not None and a.out is not None:
        ap.error(MASSES_ONLY_WITH_OUT)
    if a.sample_sep is not None and len(a.sample_sep) != 1:
        ap.error("--sample-sep takes one character")
    if a.sample_sep is not None and a.masses is None and a.masses_only is None:
        ap.error(SAMPLE_SEP_NEEDS_MASSES)
    try:
        _check_reports(requested, a.sample_sep is not None, options)  # (the thetas, asked for or not, come after the reports' rules)
        options["diversity_theta"] = parse_thetas(a.diversity_theta)
    except ValueError as e:
        ap.error(str(e))
    if a.metadata is not None and a.edge_stats is None:
        ap.error(METADATA_NEEDS_EDGE_STATS)
    if a.edpl is not None and a.out is None:
        ap.error(EDPL_NEEDS_OUT)
    if a.masses_only is None and a.out is None:
        ap.error("--out is required (or --masses-only FILE for a profile-only run)")
    db_text = None
    if a.dbimage is None:
        with open(a.jsondb or a.uniondb, "rb") as f:
            db_text = f.read()
    with open(a.fasta, "rb") as f:
        fasta_text = f.read()
    metadata = None
    if a.metadata is not None:
        with open(a.metadata, "rb") as f:
            metadata = f.read()
    call = "".join(" " + x for x in (argv if argv is not None else sys.argv[1:]))
    import json
    import time
    common = dict(device=a.device, union=a.uniondb is not None, dbimage=a.dbimage, save_dbimage=a.save_dbimage, strand=a.strand, translate=a.translate,
                  sample_sep=a.sample_sep, metadata=metadata, **requested, **options)
    t0 = time.perf_counter()
    try:
        if a.masses_only is not None:
            doc, res = None, masses_only_file(db_text, fasta_text, a.keep_at_most, a.keep_factor, a.amb, a.nsbound, **common)
        else:
            doc, res = place_file(db_text, fasta_text, a.keep_at_most, a.keep_factor, a.amb, a.nsbound, a.guppy_compat, call, masses=a.masses is not None,
                                  edpl=a.edpl is not None, **common)
    except ValueError as e:
        if str(e) != TRANSLATE_NEEDS_AA and not str(e).startswith(("--sample-sep: ", "--metadata: ", "--edge-stats: ")):
            raise
        print("rappas_amd.tools.place: " + str(e), file=sys.stderr)
        return 1
    t1 = time.perf_counter()
    if doc is not None:
        with open(a.out, "w") as f:
            f.write(doc)
    _write_outputs(a, res, a.masses_only if doc is None else a.out)
    if doc is not None:
        print(f"{len(res.n_rows)} unique reads, {int(np.count_nonzero(res.n_rows))} placed -> {a.out}", file=sys.stderr)
        return 0
    print(f"{len(res.flags)} unique reads, {res.counters['placed']} placed -> {a.masses_only}", file=sys.stderr)
    if a.timing:
        print(json.dumps({"mode": "masses_only", "unique_reads": len(res.flags), "db_and_masses_s": round(t1 - t0, 6),
                          "fasta_to_masses_s": round(time.perf_counter() - t0, 6)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
