// rk_place -- FASTA queries + a database (a `--jsondb` dump, the reference's own `.union` file, or -- round 4 -- the engine's own
// image file, `--dbimage`: mmap + upload, no parse) -> .jplace through librappas_place.so, no JVM and no Python.
// The reference's `-p p` phase for one query file (src/main_v2/Main_PLACEMENT_v07.java:150-320): ingest and the jplace writer
// are rk_hostio.hpp, the placement itself is rk_place_batch (GPU; there is no CPU fallback).
// Same options and byte-identical output as `python -m rappas_amd.tools.place`.
//
// The shape: the options in a struct, one table of rules over them (check_options), one table of sample reports (REPORTS), and one
// run over the unique reads of either ingest (run_reads): place, jplace, logs, masses, reports, EDPL.
#include <filesystem>
#include <functional>
#include <optional>

#include "../../../include/rappas_place.h"
#include "rk_place_selftest.hpp"

namespace fs = std::filesystem;

static int usage(std::ostream &os = std::cerr, int rc = 2) {
    os << "usage: rk_place (--jsondb DB.json | --uniondb DB.union | --dbimage DB.rkimg) --fasta READS.fa --out OUT.jplace [--keep-at-most 7]\n"
                 "                [--keep-factor 0.01] [--amb mean|max|skip] [--nsbound X] [--guppy-compat] [--device 0] [--logs DIR]\n"
                 "                [--threads N] [--md5-dedup] [--classic-io] [--timing] [--save-dbimage DB.rkimg] [--strand fwd|rev|both]\n"
                 "                (--strand, DNA: the reads as given = the reference's behaviour | their reverse complements | both, the better\n"
                 "                 strand per read; rev / both also write logs/reversed_<query>.tsv)\n"
                 "                [--masses FILE]  (the per-edge table of the run: one line per tree node with the reads whose best placement is its\n"
                 "                 edge and the likelihood weight on it, and the same summed over its clade; a read counts once per FASTA record)\n"
                 "                [--masses-only FILE]  (profile-only run: that table to FILE and nothing else but the notplaced and, with --strand\n"
                 "                 rev | both, the reversed log; the placements are summed on the device and never reach the host, so no jplace is\n"
                 "                 written and --out may not be given; with --translate the frames log is not written, as the frame bytes do not come\n"
                 "                 back; not with --masses; --timing prints one JSON line with keys of its own, fasta_to_masses_s among them)\n"
                 "                [--sample-sep C]  (with --masses or --masses-only: one table per sample in FILE.  A record's sample is its header up\n"
                 "                 to the first character C -- a header without C is an error --, samples are numbered in byte-wise order of their\n"
                 "                 names, and a read counts in every sample once per record of that sample; FILE holds, for each sample, a line\n"
                 "                 #sample<TAB>name<TAB>index and its table, and a last line #skipped_entries<TAB>n)\n"
                 "                [--kr FILE]  (with --sample-sep: the pairwise Kantorovich-Rubinstein distances between the samples' edge masses,\n"
                 "                 summed on the device: a line #kr<TAB>S, a line per sample with its name and S distances (%.17g), and a last line\n"
                 "                 #samples_without_mass<TAB>n; a sample without mass has nan in its row and column)\n"
                 "                [--squash FILE]  (with --sample-sep: the squash clustering of the samples over those distances, merged on the\n"
                 "                 device: a line #squash<TAB>S<TAB>n_merges, a line k<TAB>a<TAB>b<TAB>distance<TAB>size per merge, the tree as\n"
                 "                 #newick<TAB>...; (an inner node at half its distance), #inversions<TAB>n and #samples_without_mass<TAB>n)\n"
                 "                [--kmeans FILE --kmeans-k K [--kmeans-rounds N]]  (with --sample-sep: the phylogenetic k-means of the samples -- K\n"
                 "                 clusters (1..64) whose centroids are the averages of their members' mass, KR distances, farthest-first seeds, at\n"
                 "                 most N rounds (1..1024, default 100) --, found on the device: a line #kmeans<TAB>S<TAB>k<TAB>k_eff<TAB>n_active\n"
                 "                 <TAB>rounds<TAB>converged, #clusters and a line j<TAB>size<TAB>within per cluster, #samples and a line\n"
                 "                 name<TAB>cluster<TAB>distance per sample (- and 0 without mass), and a last line #samples_without_mass<TAB>n)\n"
                 "                [--diversity FILE [--diversity-theta T1,T2,...]]  (with --sample-sep: the phylogenetic diversity of every sample, what\n"
                 "                 guppy fpd reports, summed on the device: a line #diversity<TAB>S<TAB>n_theta, a line #columns with rooted_pd, pd,\n"
                 "                 bwpd, quadratic, phylo_entropy and, per theta (at most 8 exponents in 0..8), rooted_pd_<theta> and bwpd_<theta>, a\n"
                 "                 line name<TAB>values (%.17g) per sample (nan without mass), and a last line #samples_without_mass<TAB>n)\n"
                 "                [--edge-stats FILE [--metadata TSV]]  (with --sample-sep: edge dispersion and edge correlation, found on the device: for\n"
                 "                 every edge the mean, variance, standard deviation, coefficient of variation and variance-to-mean ratio of its mass\n"
                 "                 share across the samples, mean, variance and standard deviation of its imbalance, and per metadata column the\n"
                 "                 Pearson and Spearman correlation of both: a line #edge_stats<TAB>S<TAB>B<TAB>F<TAB>n_active, a line #columns, a\n"
                 "                 line per node id (%.17g, nan), #features and a line name<TAB>mean<TAB>variance per column, and a last line\n"
                 "                 #samples_without_mass<TAB>n; at most 4096 samples.  TSV: a first line sample<TAB>name_1<TAB>...<TAB>name_F, F <= 8,\n"
                 "                 and a line per sample with its name and F finite numbers; every sample of the run needs a line)\n"
                 "                [--epca FILE [--epca-components K] [--epca-iters N]]  (with --sample-sep: the edge principal components of the samples --\n"
                 "                 the difference between the mass on the two sides of every edge, centred --, found on the device: K components\n"
                 "                 (1..8, default 5) after N iterations (1..10000, default 200): a line #epca<TAB>S<TAB>B<TAB>k<TAB>n_active<TAB>k_eff\n"
                 "                 <TAB>iters, the lines #eigenvalue, #share, #residual (k values each, %.17g), #projections and a line per sample,\n"
                 "                 #loadings and a line per node id, and a last line #samples_without_mass<TAB>n)\n"
                 "                [--edpl FILE]  (with --out: the EDPL of every placed read -- the expected distance between its placement locations,\n"
                 "                 the sum over the pairs of its rows of LWR x LWR x the tree path between the midpoints of the two edges --, computed\n"
                 "                 on the device: a line #edpl<TAB>n_lines, then header<TAB>edpl (%.17g) per FASTA record that has a placement, in\n"
                 "                 input order; not with --masses-only)\n"
                 "                [--translate]  (amino-acid database, DNA reads: the six reading frames of every read are translated on the device\n"
                 "                 -- standard genetic code, longest stop-free run per frame -- and the best frame is reported; also writes\n"
                 "                 logs/frames_<query>.tsv, header<TAB>+1|+2|+3|-1|-2|-3; not with --strand rev | both)\n"
                 "       rk_place (--jsondb DB.json | --uniondb DB.union) --save-dbimage DB.rkimg      (no GPU needed)\n"
                 "       rk_place --masses-table TREE.nwk MASSES.bin OUT.tsv      (a raw little-endian u64 mass buffer as that table; no GPU needed)\n"
                 "       rk_place --sample-members READS.fa C | --masses-samples-table TREE.nwk NAMES.txt MASSES.bin OUT.tsv      (no GPU needed)\n"
                 "       rk_place --emit-tree TREE.nwk | --format-float X | --format-double X | --dedup READS.fa | --md5 TEXT\n";
    return rc;
}

static void ok(int rc, const char *call) {
    if (rc != RK_OK) throw std::runtime_error(std::string(call) + ": " + rk_last_error());
}

// ---- the options ----
static const uint32_t NO_MODE = 0xFFFFFFFFu;  // (--amb / --strand with a word that is none of theirs)

struct Options {
    std::string jsondb, uniondb, dbimage, save_image, fasta, out, logs, masses, masses_only, sample_sep, kr, squash, epca, edpl, kmeans, diversity, edge_stats, metadata, call;
    bool sample_sep_given = false, logs_given = false, md5_dedup = false, classic = false, timing = false, translate = false, guppy = false;
    unsigned threads = 0;
    uint32_t keep_at_most = 7, epca_k = 5, epca_iters = 200, kmeans_k = 0, kmeans_rounds = 100, amb_mode = RK_AMB_MEAN, strand = RK_STRAND_FORWARD;
    float keep_factor = 0.01f, nsbound = -INFINITY;
    int device = 0;
    std::vector<double> thetas;  // --diversity-theta: numbers separated by commas
    bool thetas_ok = true;
    std::optional<rkh::Metadata> meta;  // --metadata: the file, parsed before the database is opened

    int n_sources() const { return (jsondb.empty() ? 0 : 1) + (uniondb.empty() ? 0 : 1) + (dbimage.empty() ? 0 : 1); }
    bool only_convert() const { return !save_image.empty() && fasta.empty() && out.empty() && masses_only.empty(); }
};

static void parse_thetas(const std::string &text, Options &o) {
    for (size_t at = 0; !text.empty() && at <= text.size();) {
        const size_t comma = std::min(text.find(',', at), text.size());
        const std::string item = text.substr(at, comma - at);
        char *end = nullptr;
        const double v = strtod(item.c_str(), &end);
        o.thetas_ok = o.thetas_ok && !item.empty() && *end == 0 && v >= 0.0 && v <= 8.0;
        o.thetas.push_back(v);
        at = comma + 1;
    }
}

// the command line into `o`: -1, or the exit code of a line that ends here (--help, a host-only sub-command, an unknown option)
static int parse_options(int argc, char **argv, Options &o) {
    for (int i = 1; i < argc; i++) o.call += std::string(" ") + argv[i];
    Args args{argc, argv, 0};
    for (args.i = 1; args.i < argc; args.i++) {
        const std::string a = argv[args.i];
        auto val = [&]() { return args.val(a); };
        auto word = [&](std::initializer_list<std::pair<const char *, uint32_t>> words) {
            const std::string w = val();
            for (const auto &p : words) if (w == p.first) return p.second;
            return NO_MODE;
        };
        if (a == "--jsondb") o.jsondb = val();
        else if (a == "--uniondb") o.uniondb = val();
        else if (a == "--dbimage") o.dbimage = val();
        else if (a == "--save-dbimage") o.save_image = val();
        else if (a == "--threads") o.threads = (unsigned)std::stoul(val());
        else if (a == "--md5-dedup") o.md5_dedup = true;
        else if (a == "--classic-io") o.classic = true;
        else if (a == "--timing") o.timing = true;
        else if (a == "--fasta") o.fasta = val();
        else if (a == "--out") o.out = val();
        else if (a == "--keep-at-most") o.keep_at_most = (uint32_t)std::stoul(val());
        else if (a == "--keep-factor") o.keep_factor = std::stof(val());
        else if (a == "--amb") o.amb_mode = word({{"mean", RK_AMB_MEAN}, {"max", RK_AMB_MAX}, {"skip", RK_AMB_SKIP}});
        else if (a == "--strand") o.strand = word({{"fwd", RK_STRAND_FORWARD}, {"rev", RK_STRAND_REVERSE}, {"both", RK_STRAND_BOTH}});
        else if (a == "--translate") o.translate = true;
        else if (a == "--masses") o.masses = val();
        else if (a == "--masses-only") o.masses_only = val();
        else if (a == "--kr") o.kr = val();
        else if (a == "--squash") o.squash = val();
        else if (a == "--epca") o.epca = val();
        else if (a == "--edpl") o.edpl = val();
        else if (a == "--kmeans") o.kmeans = val();
        else if (a == "--kmeans-k") o.kmeans_k = (uint32_t)std::stoul(val());
        else if (a == "--kmeans-rounds") o.kmeans_rounds = (uint32_t)std::stoul(val());
        else if (a == "--diversity") o.diversity = val();
        else if (a == "--edge-stats") o.edge_stats = val();
        else if (a == "--metadata") o.metadata = val();
        else if (a == "--diversity-theta") { o.thetas.clear(); o.thetas_ok = true; parse_thetas(val(), o); }
        else if (a == "--epca-components") o.epca_k = (uint32_t)std::stoul(val());
        else if (a == "--epca-iters") o.epca_iters = (uint32_t)std::stoul(val());
        else if (a == "--sample-sep") { o.sample_sep = val(); o.sample_sep_given = true; }
        else if (a == "--help" || a == "-h") return usage(std::cout, 0);
        else if (a == "--nsbound") o.nsbound = std::stof(val());
        else if (a == "--guppy-compat") o.guppy = true;
        else if (a == "--device") o.device = std::stoi(val());
        else if (a == "--logs") { o.logs = val(); o.logs_given = true; }
        else {
            const int rc = host_subcommand(a, args, o.threads, o.md5_dedup, o.keep_at_most, o.guppy, o.call);
            return rc >= 0 ? rc : usage();
        }
    }
    return -1;
}

// ---- the sample reports of --sample-sep: one row each, run in this order ----
struct ReportCall {
    const Options &o;
    rk_db *db;
    const rk_tree *tree;
    uint32_t B;
    const std::vector<std::string> &names;
    const uint64_t *words;               // the sample mass buffer on the host, or nullptr: where the per-sample profile-only call left it on the device
    const std::vector<char> &with_mass;  // [S], from the host's copy of the buffer (filled for the rows that ask for it)
    const std::vector<double> &meta;     // [F][S], the metadata of the run's samples (--edge-stats)
};

static std::string kr_report(const ReportCall &c) {
    const uint32_t S = (uint32_t)c.names.size();
    std::vector<double> D((size_t)S * S);
    ok(rk_kr_distances_batch(c.db, c.tree, S, c.words, D.data()), "rk_kr_distances_batch");
    return rkh::kr_table(c.names, D.data());
}

static std::string squash_report(const ReportCall &c) {
    static_assert(sizeof(rkh::SquashRow) == sizeof(rk_squash_merge), "one row layout");
    const uint32_t S = (uint32_t)c.names.size();
    std::vector<rkh::SquashRow> rows(S > 1 ? S - 1 : 0);
    uint32_t n_merges = 0;
    if (S > 1) ok(rk_squash_batch(c.db, c.tree, S, c.words, (rk_squash_merge *)rows.data(), &n_merges), "rk_squash_batch");
    return rkh::squash_table(c.names, rows.data(), n_merges, c.with_mass);
}

static std::string epca_report(const ReportCall &c) {  // (one sample alone has no components: it is only counted)
    const uint32_t S = (uint32_t)c.names.size(), B = c.B, k = c.o.epca_k;
    uint32_t info[2] = {0, 0};
    std::vector<double> ev(k, 0.0), share(k, 0.0), res(k, 0.0), proj((size_t)S * k, 0.0), load((size_t)B * k, 0.0);
    if (S > 1) {
        std::vector<double> raw((size_t)rk_epca_out_doubles(B, S, k));
        ok(rk_epca_batch(c.db, c.tree, S, c.words, k, c.o.epca_iters, raw.data(), info), "rk_epca_batch");
        ok(rk_epca_finish_host(B, S, k, raw.data(), ev.data(), share.data(), res.data(), proj.data(), load.data()), "rk_epca_finish_host");
    } else {
        for (char m : c.with_mass) info[0] += m != 0;
    }
    return rkh::epca_table(c.names, B, k, c.o.epca_iters, info[0], info[1], ev.data(), share.data(), res.data(), proj.data(), load.data());
}

static std::string kmeans_report(const ReportCall &c) {
    const uint32_t S = (uint32_t)c.names.size(), k = c.o.kmeans_k;
    std::vector<uint32_t> assign(S), sizes(k);
    std::vector<double> dist(S), within(k);
    uint32_t info[4] = {0, 0, 0, 0};
    ok(rk_kmeans_batch(c.db, c.tree, S, c.words, k, c.o.kmeans_rounds, nullptr, assign.data(), dist.data(), sizes.data(), within.data(), info, nullptr), "rk_kmeans_batch");
    return rkh::kmeans_table(c.names, k, assign.data(), dist.data(), sizes.data(), within.data(), info);
}

static std::string diversity_report(const ReportCall &c) {
    const uint32_t S = (uint32_t)c.names.size();
    const std::vector<double> &thetas = c.o.thetas;
    std::vector<double> values((size_t)S * (RK_DIVERSITY_FIXED + 2 * thetas.size()));
    ok(rk_diversity_batch(c.db, c.tree, S, c.words, (uint32_t)thetas.size(), thetas.empty() ? nullptr : thetas.data(), values.data()), "rk_diversity_batch");
    return rkh::diversity_table(c.names, thetas, values.data());
}

static std::string edge_stats_report(const ReportCall &c) {
    static const std::vector<std::string> none;
    const std::vector<std::string> &features = c.o.meta ? c.o.meta->features : none;
    const uint32_t S = (uint32_t)c.names.size(), B = c.B, F = (uint32_t)features.size();
    std::vector<uint64_t> raw((size_t)rk_edgestat_out_words(B, F));
    uint32_t info[2] = {0, 0};
    ok(rk_edgestat_batch(c.db, c.tree, S, c.words, F, F ? c.meta.data() : nullptr, raw.data(), info), "rk_edgestat_batch");
    std::vector<double> table((size_t)B * (8 + 4 * F)), feature_table(2 * (size_t)F);
    ok(rk_edgestat_finish_host(B, S, F, raw.data(), info, table.data(), F ? feature_table.data() : nullptr), "rk_edgestat_finish_host");
    return rkh::edge_stats_table(c.names, features, info[0], B, table.data(), feature_table.data());
}

struct Report {
    const char *name;                        // the option `--name FILE`
    std::string Options::*path;
    const char *does;                        // "--name <does>: it needs --sample-sep ..."
    bool (*out_of_range)(const Options &);   // its own options, if it has any
    const char *range_sentence;
    bool needs_with_mass;
    std::string (*text)(const ReportCall &);
};

static const Report REPORTS[] = {
    {"kr", &Options::kr, "compares the samples of one run", nullptr, nullptr, false, kr_report},
    {"squash", &Options::squash, "clusters the samples of one run", nullptr, nullptr, true, squash_report},
    {"epca", &Options::epca, "finds the principal components of the samples of one run",
     [](const Options &o) { return o.epca_k < 1 || o.epca_k > RK_EPCA_MAX_COMPONENTS || o.epca_iters < 1 || o.epca_iters > 10000; },
     "--epca-components must be in 1..8, --epca-iters in 1..10000", true, epca_report},
    {"kmeans", &Options::kmeans, "clusters the samples of one run",
     [](const Options &o) { return o.kmeans_k < 1 || o.kmeans_k > RK_KMEANS_MAX_K || o.kmeans_rounds < 1 || o.kmeans_rounds > RK_KMEANS_MAX_ROUNDS; },
     "--kmeans needs --kmeans-k in 1..64; --kmeans-rounds must be in 1..1024", false, kmeans_report},
    {"diversity", &Options::diversity, "measures the samples of one run", nullptr, nullptr, false, diversity_report},
    {"edge-stats", &Options::edge_stats, "relates the edges to the samples of one run", nullptr, nullptr, false, edge_stats_report},
};

// ---- the rules: the first row that fires is reported, `rk_place: <sentence>` and 2 (a row without a sentence: the usage text) ----
struct Rule {
    std::function<bool(const Options &)> broken;
    std::string sentence;
};

static std::vector<Rule> rules() {
    std::vector<Rule> r = {
        {[](const Options &o) { return o.sample_sep_given && o.sample_sep.size() != 1; }, "--sample-sep takes one character"},
        {[](const Options &o) { return !o.masses_only.empty() && !o.masses.empty(); },
         "--masses-only writes the table --masses writes, without placing into a jplace: give one of the two"},
        {[](const Options &o) { return !o.masses_only.empty() && !o.out.empty(); },
         "--masses-only writes no jplace (the placements never reach the host): it cannot be combined with --out"},
        {[](const Options &o) { return !o.edpl.empty() && o.out.empty(); },
         "--edpl reads the placements of a run that writes a jplace: it needs --out (and cannot be combined with --masses-only)"},
        {[](const Options &o) { return o.sample_sep_given && o.masses_only.empty() && o.masses.empty(); },
         "--sample-sep names the samples of the per-edge tables: it needs --masses or --masses-only"},
    };
    for (const Report &rep : REPORTS) {
        r.push_back({[&rep](const Options &o) { return !(o.*rep.path).empty() && !o.sample_sep_given; },
                     std::string("--") + rep.name + " " + rep.does + ": it needs --sample-sep (with --masses or --masses-only)"});
        if (rep.out_of_range) r.push_back({[&rep](const Options &o) { return !(o.*rep.path).empty() && rep.out_of_range(o); }, rep.range_sentence});
    }
    r.push_back({[](const Options &o) { return !o.metadata.empty() && o.edge_stats.empty(); },
                 "--metadata names the sample metadata of the edge statistics: it needs --edge-stats"});
    r.push_back({[](const Options &o) { return !o.thetas_ok || o.thetas.size() > RK_DIVERSITY_MAX_THETA; },
                 "--diversity-theta takes at most 8 numbers in 0..8, separated by commas"});
    r.push_back({[](const Options &o) {
                     return o.n_sources() != 1 || (!o.only_convert() && (o.fasta.empty() || (o.out.empty() && o.masses_only.empty()))) || (o.only_convert() && !o.dbimage.empty());
                 }, ""});
    r.push_back({[](const Options &o) { return o.amb_mode == NO_MODE; }, ""});
    r.push_back({[](const Options &o) { return o.strand == NO_MODE; }, ""});
    r.push_back({[](const Options &o) { return o.translate && o.strand != RK_STRAND_FORWARD; },
                 "--translate places every read in all six reading frames, both strands included: it cannot be combined with --strand rev | both"});
    return r;
}

static int check_options(const Options &o) {
    for (const Rule &r : rules()) {
        if (!r.broken(o)) continue;
        if (r.sentence.empty()) return usage();
        std::cerr << "rk_place: " << r.sentence << "\n";
        return 2;
    }
    return 0;
}

// ---- one run ----
// the database's tree on the device, as the reports and --edpl take it
struct DeviceTree {
    rk_tree *p = nullptr;
    DeviceTree(int device, const rkh::Tree &t) {
        const uint32_t B = (uint32_t)t.nodes.size();
        std::vector<int32_t> parent(B);
        std::vector<float> bl(B);
        for (uint32_t x = 0; x < B; x++) { parent[x] = t.nodes[x].parent; bl[x] = t.nodes[x].bl; }
        ok(rk_tree_create(device, B, parent.data(), bl.data(), &p), "rk_tree_create");
    }
    DeviceTree(const DeviceTree &) = delete;
    ~DeviceTree() { rk_tree_destroy(p); }
};

struct Run {
    const Options &o;
    rk_db *db;
    const rkh::Tree &tree;
    rk_params p;
    fs::path log_dir;
    std::optional<DeviceTree> on_device;
    std::vector<double> sample_meta;  // --edge-stats: the metadata of the run's samples [F][S], looked up behind the FASTA scan
    const rk_tree *device_tree() {  // (built once, and only by a run that asks for a report or --edpl)
        if (!on_device) on_device.emplace(o.device, tree);
        return on_device->p;
    }
};

// the unique reads of the query file as either ingest leaves them, and what the steps after it ask of the file's records
struct ReadSet {
    size_t n, n_records;                                                            // unique reads, FASTA records
    const uint8_t *seq;
    const uint64_t *off;
    const uint32_t *uniq_of_rec;
    rkh::Team &team;
    std::function<std::pair<const char *, size_t>(size_t)> header;
    std::function<void(uint32_t *)> weights;                                        // [n]: a unique read weighs the FASTA records it stands for
    std::function<std::string(const uint32_t *, uint32_t, uint32_t)> flagged_log;   // `header` per record whose unique read has (flags & mask) == want
    std::function<std::string(const uint8_t *)> frames_log;
};

// the seconds of run_reads, for --timing
struct Marks {
    double ready, engine_ready, placed, written, done;
    uint64_t n_placed;
};

// the reports asked for, from the sample mass buffer: `words` as ReportCall has it, `host_words` the host's copy either way
static void write_reports(Run &run, const std::vector<std::string> &names, const uint64_t *words, const uint64_t *host_words) {
    const uint32_t B = (uint32_t)run.tree.nodes.size(), S = (uint32_t)names.size();
    std::vector<char> with_mass;
    for (const Report &rep : REPORTS) {
        const std::string &path = run.o.*rep.path;
        if (path.empty()) continue;
        if (rep.needs_with_mass && with_mass.empty()) {
            with_mass.assign(S, 0);
            for (uint32_t s = 0; s < S; s++)
                for (uint32_t x = 0; x < B && !with_mass[s]; x++) with_mass[s] = host_words[(size_t)s * (2 * (size_t)B + 4) + x] != 0;
        }
        write_text(path, rep.text(ReportCall{run.o, run.db, run.device_tree(), B, names, words, with_mass, run.sample_meta}));
    }
}

// --masses / --masses-only FILE: the per-edge table of the whole run -- with --sample-sep one per sample (`sm`: the samples and the
// membership entries of the unique reads), and then the reports.  res: the results of a placing run, summed on the host (the weight
// of a unique read is the number of FASTA records it stands for, so the table speaks of reads); nullptr: --masses-only, one
// profile-only call -- every chunk is placed and summed on the device, the flags alone come back
static void masses_step(Run &run, const ReadSet &rs, const rkh::SampleMembers *sm, const uint32_t *weight, const rk_result *res, uint32_t *flags_out, rk_counters *ct) {
    const Options &o = run.o;
    const std::string opt = res ? "--masses" : "--masses-only", &path = res ? o.masses : o.masses_only;
    const uint32_t B = (uint32_t)run.tree.nodes.size(), K = o.keep_at_most, step = o.translate ? RK_STEP_TRANSLATED : o.strand;
    if (!sm) {
        std::vector<uint64_t> words((size_t)rk_masses_words(B), 0);
        if (words.empty()) throw std::runtime_error(opt + ": the tree has no nodes, or more than 65535");
        if (res) ok(rk_masses_accumulate_host(B, K, rs.n, res, weight, words.data(), rs.team.size()), "rk_masses_accumulate_host");
        else ok(rk_place_batch_masses(run.db, &run.p, step, rs.n, rs.seq, rs.off, weight, words.data(), flags_out, ct), "rk_place_batch_masses");
        write_text(path, rkh::masses_table(run.tree, words.data(), words.size()));
        return;
    }
    const uint32_t S = (uint32_t)sm->names.size();
    std::vector<uint64_t> words((size_t)rk_masses_samples_words(B, S), 0);
    if (words.empty()) throw std::runtime_error(opt + " --sample-sep: " + std::to_string(S) + " samples on this tree are beyond the limits of a sample mass buffer");
    if (res) {
        std::vector<uint32_t> reads(sm->sample.size());
        for (uint64_t r = 0; r < rs.n; r++)
            for (uint64_t e = sm->off[r]; e < sm->off[r + 1]; e++) reads[e] = (uint32_t)r;
        ok(rk_masses_accumulate_samples_host(B, K, rs.n, res, S, reads.size(), reads.data(), sm->sample.data(), sm->weight.data(), words.data(), rs.team.size()),
           "rk_masses_accumulate_samples_host");
    } else {  // (the membership CSR in place of the weights)
        ok(rk_place_batch_masses_samples(run.db, &run.p, step, rs.n, rs.seq, rs.off, S, sm->off.data(), sm->sample.data(), sm->weight.data(), words.data(), flags_out, ct),
           "rk_place_batch_masses_samples");
    }
    write_text(path, rkh::masses_samples_table(run.tree, sm->names, words.data(), words.size()));
    write_reports(run, sm->names, res ? words.data() : nullptr, words.data());  // (--masses-only: the buffer is still on the device in the handle)
}

// notplaced_<query>.tsv under logs/ next to the output, as the reference's workdir/logs (Main_PLACEMENT_v07.java:208-214); with
// --strand rev | both reversed_<query>.tsv, and from a placing run with --translate (frame: its bytes) frames_<query>.tsv
static void write_logs(const Run &run, const ReadSet &rs, const uint32_t *flags, const uint8_t *frame) {
    const std::string query = fs::path(run.o.fasta).filename().string();
    auto log = [&](const std::string &kind, const std::string &text) {
        write_text((run.log_dir / (kind + "_" + query + ".tsv")).string(), text, "the " + kind + " log under " + run.log_dir.string());
    };
    fs::create_directories(run.log_dir);
    log("notplaced", rs.flagged_log(flags, 1u, 0u));
    if (run.o.strand != RK_STRAND_FORWARD) log("reversed", rs.flagged_log(flags, RK_FLAG_REVERSE, RK_FLAG_REVERSE));
    if (frame) log("frames", rs.frames_log(frame));
}

// everything after "the unique reads are in seq / off": --masses-only, or place, the jplace (by the ingest's own writer: -> the reads
// it placed), the logs, --masses with the reports, --edpl.  engine_ready() is waited for once the buffers are there
template <class EngineReady, class WriteJplace>
static Marks run_reads(Run &run, const ReadSet &rs, EngineReady engine_ready, WriteJplace write_jplace) {
    const Options &o = run.o;
    const size_t n = rs.n, K = o.keep_at_most;
    rkh::Team &team = rs.team;
    Marks m{};
    rkh::SampleMembers members;
    if (o.sample_sep_given) members = rkh::sample_members(rs.n_records, n, rs.header, rs.uniq_of_rec, o.sample_sep[0]);
    const rkh::SampleMembers *sm = o.sample_sep_given ? &members : nullptr;
    if (sm && !o.edge_stats.empty()) run.sample_meta = rkh::metadata_of_samples(sm->names, o.meta ? &*o.meta : nullptr);  // (before placing: every sample has its line)
    rkh::RawArray<uint32_t> weight, flags;
    flags.alloc(n);
    auto weigh = [&]() { weight.alloc(n); rs.weights(weight.data()); };
    if (!o.masses_only.empty()) {
        weigh();
        team.run([&](unsigned t, unsigned T) { memset(flags.data() + n * t / T, 0, (n * (t + 1) / T - n * t / T) * 4); });
        m.ready = now();
        engine_ready();
        m.engine_ready = now();
        rk_counters ct{};
        masses_step(run, rs, sm, weight.data(), nullptr, flags.data(), &ct);
        m.placed = now();
        write_logs(run, rs, flags.data(), nullptr);
        m.written = m.done = now();
        m.n_placed = ct.placed;
    } else {
        rkh::RawArray<uint8_t> n_rows;
        rkh::RawArray<uint16_t> branch;
        rkh::RawArray<float> score;
        rkh::RawArray<double> lwr;
        n_rows.alloc(n); branch.alloc(n * K); score.alloc(n * K); lwr.alloc(n * K);
        team.run([&](unsigned t, unsigned T) {  // (first touch by every thread at once, not by the engine's few result-copy threads)
            const size_t lo = n * t / T, hi = n * (t + 1) / T;
            memset(n_rows.data() + lo, 0, hi - lo); memset(flags.data() + lo, 0, (hi - lo) * 4);
            memset(branch.data() + lo * K, 0, (hi - lo) * K * 2); memset(score.data() + lo * K, 0, (hi - lo) * K * 4); memset(lwr.data() + lo * K, 0, (hi - lo) * K * 8);
        });
        m.ready = now();
        engine_ready();
        m.engine_ready = now();
        rk_result res{n_rows.data(), branch.data(), score.data(), lwr.data(), flags.data()};
        rk_counters ct;
        std::vector<uint8_t> frame;  // (--translate only) the reading frame of every unique read's result
        // (fwd is rk_place_batch itself: the reference's behaviour, and this driver's before it knew about strands)
        if (o.translate) {
            frame.assign(n, (uint8_t)RK_FRAME_NONE);
            ok(rk_place_batch_translated(run.db, &run.p, n, rs.seq, rs.off, &res, frame.data(), &ct), "rk_place_batch_translated");
        } else if (o.strand == RK_STRAND_FORWARD) {
            ok(rk_place_batch(run.db, &run.p, n, rs.seq, rs.off, &res, &ct), "rk_place_batch");
        } else {
            ok(rk_place_batch_strands(run.db, &run.p, o.strand, n, rs.seq, rs.off, &res, &ct), "rk_place_batch_strands");
        }
        m.placed = now();
        m.n_placed = write_jplace(res);
        m.written = now();
        write_logs(run, rs, flags.data(), o.translate ? frame.data() : nullptr);
        if (!o.masses.empty()) {
            weigh();
            masses_step(run, rs, sm, weight.data(), &res, nullptr, nullptr);
        }
        if (!o.edpl.empty()) {  // the EDPL of every unique read from the results on the host, through rk_edpl_batch; a line per FASTA record that has a placement
            std::vector<double> edpl(n, 0.0);
            ok(rk_edpl_batch(run.db, run.device_tree(), o.keep_at_most, n, &res, edpl.data()), "rk_edpl_batch");
            write_text(o.edpl, rkh::edpl_table(rs.n_records, rs.header, rs.uniq_of_rec, res.n_rows, edpl.data()));
        }
        m.done = now();
    }
    std::cerr << n << " unique reads, " << m.n_placed << " placed -> " << (o.out.empty() ? o.masses_only : o.out) << "\n";
    return m;
}

// the database on the device and its reference tree; nullptr: --save-dbimage alone, the image is written and that was all
static rk_db *open_db(const Options &o, rkh::Tree &tree) {
    rk_db *db = nullptr;
    if (!o.dbimage.empty()) {
        // the engine's own image: the reference tree travels in its user blob (rkh::tree_to_blob)
        uint64_t len = 0;
        ok(rk_db_image_user(o.dbimage.c_str(), nullptr, 0, &len), "rk_db_image_user");
        std::string blob((size_t)len, '\0');
        if (len) ok(rk_db_image_user(o.dbimage.c_str(), blob.data(), len, &len), "rk_db_image_user");
        tree = rkh::tree_from_blob(blob);
        ok(rk_db_load(o.dbimage.c_str(), o.device, &db), "rk_db_load");
        rk_db_info info;
        (void)rk_db_get_info(db, &info);
        if (info.n_branches != tree.nodes.size()) {
            rk_db_destroy(db);
            throw std::runtime_error("database image: the tree has " + std::to_string(tree.nodes.size()) + " nodes, the database " + std::to_string(info.n_branches) + " branches");
        }
        return db;
    }
    rkh::JsonDb jd;
    rkh::UnionDb ud;
    rk_db_desc d;
    memset(&d, 0, sizeof(d));
    if (!o.uniondb.empty()) {
        ud = rkh::load_uniondb(slurp(o.uniondb));
        tree = ud.tree;
        d.alphabet = ud.alphabet == 4 ? RK_ALPHABET_DNA : RK_ALPHABET_AA; d.convert_uo = ud.convert_uo ? 1 : 0; d.k = ud.k;
        d.thr_log10 = ud.thr_log10; d.thr = ud.thr; d.n_keys = ud.key_codes.size();
        d.key_codes = ud.key_codes.data(); d.row_offsets = ud.row_offsets.data(); d.branch_ids = ud.branch_ids.data(); d.scores = ud.scores.data();
    } else {
        jd = rkh::load_jsondb(slurp(o.jsondb));
        tree = rkh::parse_newick(jd.original_tree);
        d.alphabet = RK_ALPHABET_DNA; d.k = jd.k;
        d.thr_log10 = jd.thr_log10; d.thr = jd.thr; d.n_keys = jd.key_codes.size();
        d.key_codes = jd.key_codes.data(); d.row_offsets = jd.row_offsets.data(); d.branch_ids = jd.branch_ids.data(); d.scores = jd.scores.data();
    }
    d.n_branches = (uint32_t)tree.nodes.size();
    d.device = o.device; d.table_mode = RK_TABLE_AUTO;
    if (!o.save_image.empty()) {  // (built on the host: a machine without a GPU can write the image a placement node loads)
        const std::string blob = rkh::tree_to_blob(tree);
        ok(rk_db_save_desc(&d, o.save_image.c_str(), blob.data(), blob.size()), "rk_db_save_desc");
        if (o.only_convert()) { std::cerr << "database image -> " << o.save_image << "\n"; return nullptr; }
    }
    ok(rk_db_create(&d, &db), "rk_db_create");
    return db;
}

int main(int argc, char **argv) {
    try {
        Options o;
        int rc = parse_options(argc, argv, o);
        if (rc >= 0) return rc;
        if ((rc = check_options(o)) != 0) return rc;
        const double t_start = now();
        if (!o.metadata.empty()) o.meta = rkh::parse_metadata(slurp(o.metadata));  // (its syntax, before the device is opened)
        rkh::Tree tree;
        rk_db *db = open_db(o, tree);
        if (!db) return 0;
        struct DbGuard { rk_db *p; ~DbGuard() { rk_db_destroy(p); } } db_guard{db};
        if (o.translate) {
            rk_db_info info;
            ok(rk_db_get_info(db, &info), "rk_db_get_info");
            if (info.alphabet != RK_ALPHABET_AA)
                throw std::runtime_error("--translate needs an amino-acid database (this one holds DNA: DNA reads are placed on it as they are, see --strand)");
        }
        const double t_db = now();
        const uint32_t K = o.keep_at_most;
        const bool masses_only = !o.masses_only.empty();
        Run run{o, db, tree, rk_params{K, o.keep_factor, o.amb_mode, o.nsbound},
                o.logs_given ? fs::path(o.logs) : fs::absolute(fs::path(masses_only ? o.masses_only : o.out)).parent_path() / "logs", std::nullopt, {}};

        if (!o.classic) {
            // ---- every host thread on every pass (rk_fastio.hpp) ----
            unsigned hw = std::thread::hardware_concurrency();
            rkh::Team team(o.threads ? o.threads : std::max(1u, std::min(hw ? hw : 1u, 32u)));
            // the engine's first batch of a process sets up its workspaces and has its kernels loaded to the device (~100 ms): started
            // here, on a thread of its own, next to the mapping and the scan of the query file (engine start-up, like the database load)
            double warm_s = 0;
            std::thread warm([&]() { const double w0 = now(); (void)rk_reserve_host_path(db, K, 320); warm_s = now() - w0; });
            struct JoinWarm { std::thread &t; ~JoinWarm() { if (t.joinable()) t.join(); } } join_warm{warm};
            rkh::MappedFile fa;
            fa.open_file(o.fasta);
            const double t0 = now();
            const rkh::FastaScan sc = rkh::scan_fasta(fa.data, fa.size, team, o.md5_dedup);
            const double t1 = now();
            const rkh::FastDedup dd = rkh::dedup_fast(sc, team);
            const double t2 = now();
            rkh::RawArray<char> seq;
            rkh::RawArray<uint64_t> off;
            rkh::gather_unique(sc, dd, team, seq, off);
            const size_t n = dd.first_rec.size();
            const ReadSet rs{n, sc.recs.size(), (const uint8_t *)seq.data(), off.data(), dd.uniq_of_rec.data(), team,
                [&](size_t r) { return std::make_pair((const char *)sc.recs[r].hdr, (size_t)sc.recs[r].hdr_len); },
                [&](uint32_t *weight) {
                    team.run([&](unsigned t, unsigned T) {
                        for (size_t u = n * t / T; u < n * (t + 1) / T; u++) {
                            uint32_t c = 0;
                            for (uint32_t rec = dd.first_rec[u]; rec != 0xFFFFFFFFu; rec = dd.next_dup[rec]) c++;
                            weight[u] = c;
                        }
                    });
                },
                [&](const uint32_t *flags, uint32_t mask, uint32_t want) { return rkh::flagged_log_fast(sc, dd, flags, mask, want); },
                [&](const uint8_t *frame) { return rkh::frames_log_fast(sc, dd, frame); }};
            rkh::FastWriteStats ws{};
            const Marks m = run_reads(run, rs, [&]() { warm.join(); }, [&](const rk_result &res) {
                ws = rkh::write_jplace_fast(o.out, tree, sc, dd, K, res.n_rows, res.branch, res.score, res.lwr, o.call, o.guppy, team);
                return ws.placed;
            });
            if (o.timing && masses_only) {
                char buf[600];
                snprintf(buf, sizeof(buf),
                         "{\"mode\": \"masses_only\", \"reads\": %zu, \"unique\": %zu, \"placed\": %llu, \"fasta_bytes\": %zu, \"threads\": %u, \"db_s\": %.6f, "
                         "\"engine_warm_up_s\": %.6f, \"scan_s\": %.6f, \"dedup_s\": %.6f, \"gather_s\": %.6f, \"place_and_sum_s\": %.6f, "
                         "\"place_wait_for_warm_up_s\": %.6f, \"logs_s\": %.6f, \"fasta_to_masses_s\": %.6f}",
                         sc.recs.size(), n, (unsigned long long)m.n_placed, fa.size, team.size(), t_db - t_start, warm_s, t1 - t0, t2 - t1, m.ready - t2, m.placed - m.ready,
                         m.engine_ready - m.ready, m.done - m.placed, m.done - t0);
                std::cout << buf << std::endl;
            } else if (o.timing) {  // one JSON line (bench.py's fasta_to_jplace leg reads it): seconds per pass, FASTA bytes in -> jplace bytes out
                char buf[700];
                snprintf(buf, sizeof(buf),
                         "{\"reads\": %zu, \"unique\": %zu, \"placed\": %llu, \"fasta_bytes\": %zu, \"jplace_bytes\": %llu, \"threads\": %u, \"db_s\": %.6f, \"engine_warm_up_s\": %.6f, \"scan_s\": %.6f, "
                         "\"dedup_s\": %.6f, \"gather_s\": %.6f, \"place_s\": %.6f, \"place_wait_for_warm_up_s\": %.6f, \"write_s\": %.6f, \"write_format_s\": %.6f, \"write_io_s\": %.6f, \"notplaced_log_s\": %.6f, \"fasta_to_jplace_s\": %.6f, "
                         "\"exact_writer\": %s}",
                         sc.recs.size(), n, (unsigned long long)ws.placed, fa.size, (unsigned long long)ws.bytes, team.size(), t_db - t_start, warm_s, t1 - t0, t2 - t1, m.ready - t2,
                         m.placed - m.ready, m.engine_ready - m.ready, m.written - m.placed, ws.format_s, ws.io_s, m.done - m.written, m.written - t0, ws.exact_path ? "true" : "false");
                std::cout << buf << std::endl;
            }
            return 0;
        }

        // ---- the one-string-at-a-time path of rk_hostio.hpp (the definition the fast path is held to) ----
        const double tc0 = now();
        const std::vector<rkh::Fasta> records = rkh::read_fasta(slurp(o.fasta));
        const rkh::Dedup dd = rkh::dedup_index(records);
        const std::vector<std::vector<std::string>> names = rkh::dedup_names(records, dd);
        const size_t n = dd.first_rec.size();
        std::string seq;
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + records[dd.first_rec[i]].seq.size();
        seq.reserve(off[n]);
        for (size_t i = 0; i < n; i++) seq += records[dd.first_rec[i]].seq;
        rkh::Team alone(1);
        const ReadSet rs{n, records.size(), (const uint8_t *)seq.data(), off.data(), dd.uniq_of_rec.data(), alone,
            [&](size_t r) { return std::make_pair(records[r].header.data(), records[r].header.size()); },
            [&](uint32_t *weight) { for (size_t i = 0; i < n; i++) weight[i] = (uint32_t)names[i].size(); },
            [&](const uint32_t *flags, uint32_t mask, uint32_t want) { return rkh::flagged_log(records, dd, flags, mask, want); },
            [&](const uint8_t *frame) { return rkh::frames_log(records, dd, frame); }};
        run_reads(run, rs, []() {}, [&](const rk_result &res) {
            const auto pl = rkh::jplace_placements(tree, names, n, K, res.n_rows, res.branch, res.score, res.lwr, o.guppy);
            write_text(o.out, rkh::jplace_document(tree, pl, o.call, o.guppy));
            return (uint64_t)pl.size();
        });
        if (o.timing)
            std::cout << (masses_only ? "{\"mode\": \"masses_only\", \"reads\": " : "{\"reads\": ") << records.size() << ", \"unique\": " << n << ", \"db_s\": " << (t_db - t_start)
                      << (masses_only ? ", \"fasta_to_masses_s\": " : ", \"fasta_to_jplace_s\": ") << (now() - tc0) << ", \"classic\": true}" << std::endl;
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "rk_place: " << e.what() << "\n";
        return 1;
    }
}
