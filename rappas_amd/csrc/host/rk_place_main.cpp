// rk_place -- FASTA queries + a database (a `--jsondb` dump, the reference's own `.union` file, or -- round 4 -- the engine's own
// image file, `--dbimage`: mmap + upload, no parse) -> .jplace through librappas_place.so, no JVM and no Python.
// The reference's `-p p` phase for one query file (src/main_v2/Main_PLACEMENT_v07.java:150-320): ingest and the jplace writer
// are rk_hostio.hpp, the placement itself is rk_place_batch (GPU; there is no CPU fallback).
// Same options and byte-identical output as `python -m rappas_amd.tools.place`.
#include <chrono>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>

#include <sys/resource.h>

#include "../../../include/rappas_place.h"
#include "rk_hostio.hpp"
#include "rk_fastio.hpp"

static std::string slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::ostringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

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

int main(int argc, char **argv) {
    try {
        std::string jsondb, uniondb, dbimage, save_image, fasta, out, amb = "mean", logs, strand_name = "fwd", masses_path, masses_only_path, sample_sep, kr_path, squash_path, epca_path, edpl_path, kmeans_path, diversity_path, diversity_theta;
        bool logs_given = false, md5_dedup = false, classic = false, timing = false, translate = false;
        unsigned threads = 0;
        uint32_t keep_at_most = 7, epca_k = 5, epca_iters = 200, kmeans_k = 0, kmeans_rounds = 100;
        float keep_factor = 0.01f, nsbound = -INFINITY;
        bool guppy = false;
        int device = 0;
        std::string call;
        for (int i = 1; i < argc; i++) call += std::string(" ") + argv[i];
        for (int i = 1; i < argc; i++) {
            const std::string a = argv[i];
            auto val = [&]() -> std::string { if (i + 1 >= argc) throw std::runtime_error("missing value after " + a); return argv[++i]; };
            if (a == "--jsondb") jsondb = val();
            else if (a == "--uniondb") uniondb = val();
            else if (a == "--dbimage") dbimage = val();
            else if (a == "--save-dbimage") save_image = val();
            else if (a == "--threads") threads = (unsigned)std::stoul(val());
            else if (a == "--md5-dedup") md5_dedup = true;
            else if (a == "--classic-io") classic = true;
            else if (a == "--timing") timing = true;
            else if (a == "--fasta") fasta = val();
            else if (a == "--out") out = val();
            else if (a == "--keep-at-most") keep_at_most = (uint32_t)std::stoul(val());
            else if (a == "--keep-factor") keep_factor = std::stof(val());
            else if (a == "--amb") amb = val();
            else if (a == "--strand") strand_name = val();
            else if (a == "--translate") translate = true;
            else if (a == "--masses") masses_path = val();
            else if (a == "--masses-only") masses_only_path = val();
            else if (a == "--kr") kr_path = val();
            else if (a == "--squash") squash_path = val();
            else if (a == "--epca") epca_path = val();
            else if (a == "--edpl") edpl_path = val();
            else if (a == "--kmeans") kmeans_path = val();
            else if (a == "--kmeans-k") kmeans_k = (uint32_t)std::stoul(val());
            else if (a == "--kmeans-rounds") kmeans_rounds = (uint32_t)std::stoul(val());
            else if (a == "--diversity") diversity_path = val();
            else if (a == "--diversity-theta") diversity_theta = val();
            else if (a == "--epca-components") epca_k = (uint32_t)std::stoul(val());
            else if (a == "--epca-iters") epca_iters = (uint32_t)std::stoul(val());
            else if (a == "--sample-sep") { sample_sep = val(); if (sample_sep.size() != 1) throw std::runtime_error("--sample-sep takes one character"); }
            else if (a == "--help" || a == "-h") return usage(std::cout, 0);
            else if (a == "--nsbound") nsbound = std::stof(val());
            else if (a == "--guppy-compat") guppy = true;
            else if (a == "--device") device = std::stoi(val());
            else if (a == "--logs") { logs = val(); logs_given = true; }
            // ---- host-side pieces on their own (no device needed): used by the CPU tests ----
            else if (a == "--emit-tree") {
                const rkh::Tree t = rkh::parse_newick(slurp(val()));
                std::cout << rkh::jplace_newick(t) << "\n" << rkh::write_newick(t, false, false, false) << "\n" << (t.rooted() ? "rooted" : "unrooted");
                for (const auto &n : t.nodes) std::cout << "\n" << n.id << "\t" << n.label << "\t" << n.jplace_edge << "\t" << n.parent;
                std::cout << "\n";
                return 0;
            } else if (a == "--format-float") { std::cout << rkh::java_float_to_string(strtof(val().c_str(), nullptr)) << "\n"; return 0; }
            else if (a == "--format-double") { std::cout << rkh::java_double_to_string(strtod(val().c_str(), nullptr)) << "\n"; return 0; }
            else if (a == "--md5") {
                for (uint8_t b : rkh::md5(val())) printf("%02x", b);
                printf("\n");
                return 0;
            } else if (a == "--dedup") {
                std::vector<rkh::Fasta> uniq;
                std::vector<std::vector<std::string>> names;
                rkh::dedup_reads(rkh::read_fasta(slurp(val())), uniq, names);
                for (size_t r = 0; r < uniq.size(); r++) {
                    std::cout << uniq[r].seq;
                    for (const auto &n : names[r]) std::cout << "\t" << n;
                    std::cout << "\n";
                }
                return 0;
            } else if (a == "--fast-rate") {  // FASTA [TREE]: the fast path's host passes on their own, timed (no device needed); with a tree also the writer, on made-up placements
                const std::string path = val();
                const std::string tpath = (i + 1 < argc && argv[i + 1][0] != '-') ? val() : std::string();
                auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
                unsigned hw = std::thread::hardware_concurrency();
                rkh::Team team(threads ? threads : std::max(1u, std::min(hw ? hw : 1u, 32u)));
                rkh::MappedFile fa;
                fa.open_file(path);
                for (int rep = 0; rep < 3; rep++) {
                    const double t0 = now();
                    const rkh::FastaScan sc = rkh::scan_fasta(fa.data, fa.size, team, md5_dedup);
                    const double t1 = now();
                    const rkh::FastDedup dd = rkh::dedup_fast(sc, team);
                    const double t2 = now();
                    rkh::RawArray<char> seq;
                    rkh::RawArray<uint64_t> off;
                    rkh::gather_unique(sc, dd, team, seq, off);
                    const double t3 = now();
                    printf("%zu reads, %zu unique, %u threads: scan %.1f ms (%.2f GB/s), dedup %.1f ms, gather %.1f ms", sc.recs.size(), dd.first_rec.size(), team.size(),
                           (t1 - t0) * 1e3, fa.size / (t1 - t0) / 1e9, (t2 - t1) * 1e3, (t3 - t2) * 1e3);
                    if (!tpath.empty()) {
                        const rkh::Tree t = rkh::parse_newick(slurp(tpath));
                        const size_t n = dd.first_rec.size();
                        const uint32_t K = keep_at_most;
                        std::vector<uint8_t> n_rows(n, 3);
                        std::vector<uint16_t> branch(n * K);
                        std::vector<float> score(n * K);
                        std::vector<double> lwr(n * K);
                        uint64_t seed = 7;
                        for (size_t q = 0; q < n * K; q++) {
                            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
                            branch[q] = (uint16_t)((seed >> 33) % t.nodes.size());
                            score[q] = -(float)((seed >> 20) & 0xFFFFF) / 1713.0f;
                            lwr[q] = (double)(seed >> 11) * 0x1.0p-53;
                        }
                        const double t4 = now();
                        const rkh::FastWriteStats ws = rkh::write_jplace_fast("/dev/shm/rk_fast_rate.jplace", t, sc, dd, K, n_rows.data(), branch.data(), score.data(), lwr.data(), call, guppy, team);
                        const double t5 = now();
                        printf(", write %.1f ms (format %.1f, io %.1f; %.0f MB)", (t5 - t4) * 1e3, ws.format_s * 1e3, ws.io_s * 1e3, ws.bytes / 1e6);
                        (void)unlink("/dev/shm/rk_fast_rate.jplace");
                    }
                    printf("\n");
                }
                return 0;
            } else if (a == "--dedup-fast") {  // the fast path's scan + dedup, printed like --dedup (CPU tests hold the two together)
                const std::string path = val();
                rkh::Team team(threads ? threads : 4);
                rkh::MappedFile fa;
                fa.open_file(path);
                const rkh::FastaScan sc = rkh::scan_fasta(fa.data, fa.size, team, md5_dedup);
                const rkh::FastDedup dd = rkh::dedup_fast(sc, team);
                for (size_t u = 0; u < dd.first_rec.size(); u++) {
                    uint32_t rec = dd.first_rec[u];
                    std::cout << std::string(sc.recs[rec].seq, sc.recs[rec].seq_len);
                    bool first = true;
                    while (rec != 0xFFFFFFFFu) {
                        std::string name(sc.recs[rec].hdr, sc.recs[rec].hdr_len);
                        if (!first) { const size_t cut = name.find(' '); if (cut != std::string::npos) name.resize(cut); }
                        std::cout << "\t" << name;
                        first = false;
                        rec = dd.next_dup[rec];
                    }
                    std::cout << "\n";
                }
                return 0;
            } else if (a == "--write-selftest") {  // FASTA TREE OUT_FAST OUT_CLASSIC SEED: both jplace writers on the same made-up placements
                const std::string fpath = val(), tpath = val(), out_fast = val(), out_classic = val();
                uint64_t seed = std::stoull(val());
                auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
                const rkh::Tree t = rkh::parse_newick(slurp(tpath));
                rkh::Team team(threads ? threads : 4);
                rkh::MappedFile fa;
                fa.open_file(fpath);
                const rkh::FastaScan sc = rkh::scan_fasta(fa.data, fa.size, team, md5_dedup);
                const rkh::FastDedup dd = rkh::dedup_fast(sc, team);
                const size_t n = dd.first_rec.size();
                const uint32_t K = keep_at_most;
                std::vector<uint8_t> n_rows(n);
                std::vector<uint16_t> branch(n * K);
                std::vector<float> score(n * K);
                std::vector<double> lwr(n * K);
                for (size_t i = 0; i < n; i++) {
                    n_rows[i] = (uint8_t)(rnd() % (K + 1));
                    if (rnd() % 7 == 0) n_rows[i] = 0;
                    for (uint32_t j = 0; j < K; j++) {
                        branch[i * K + j] = (uint16_t)(rnd() % t.nodes.size());
                        score[i * K + j] = -(float)(rnd() % 100000) / 97.0f - (j ? 0.0f : 1e-3f * (float)(rnd() % 10));
                        lwr[i * K + j] = (double)(rnd() % 1000003) / 1000003.0 * (rnd() % 5 == 0 ? 1e-9 : 1.0);
                    }
                }
                const rkh::FastWriteStats ws = rkh::write_jplace_fast(out_fast, t, sc, dd, K, n_rows.data(), branch.data(), score.data(), lwr.data(), call, guppy, team);
                // classic: the records as rk_hostio.hpp sees them
                const std::vector<rkh::Fasta> records = rkh::read_fasta(slurp(fpath));
                const rkh::Dedup cd = rkh::dedup_index(records);
                if (cd.first_rec.size() != n) throw std::runtime_error("the two dedups disagree on the number of unique reads");
                const auto names = rkh::dedup_names(records, cd);
                const auto pl = rkh::jplace_placements(t, names, n, K, n_rows.data(), branch.data(), score.data(), lwr.data(), guppy);
                std::ofstream of(out_classic, std::ios::binary);
                of << rkh::jplace_document(t, pl, call, guppy);
                std::cout << n << " " << ws.placed << " " << (ws.exact_path ? "exact" : "direct") << "\n";
                return 0;
            } else if (a == "--masses-table") {  // TREE MASSES OUT: the table writer on its own (compared with the Python twin)
                const std::string tpath = val(), mpath = val(), opath = val();
                const rkh::Tree t = rkh::parse_newick(slurp(tpath));
                const std::string raw = slurp(mpath);
                if (raw.size() % 8) throw std::runtime_error(mpath + ": not a whole number of 64-bit words");
                std::vector<uint64_t> m(raw.size() / 8);
                if (!m.empty()) memcpy(m.data(), raw.data(), raw.size());
                std::ofstream of(opath, std::ios::binary);
                if (!of) throw std::runtime_error("cannot write " + opath);
                of << rkh::masses_table(t, m.data(), m.size());
                return 0;
            } else if (a == "--sample-members") {  // FASTA C: the samples and the membership CSR of --sample-sep (compared with the Python twin)
                const std::string path = val(), sep = val();
                if (sep.size() != 1) throw std::runtime_error("--sample-members takes one separator character");
                const std::vector<rkh::Fasta> records = rkh::read_fasta(slurp(path));
                const rkh::Dedup cd = rkh::dedup_index(records);
                const rkh::SampleMembers sm = rkh::sample_members(records.size(), cd.first_rec.size(),
                    [&](size_t r) { return std::make_pair(records[r].header.data(), records[r].header.size()); }, cd.uniq_of_rec.data(), sep[0]);
                for (size_t s = 0; s < sm.names.size(); s++) std::cout << "#sample\t" << sm.names[s] << "\t" << s << "\n";
                for (size_t u = 0; u + 1 < sm.off.size(); u++) {
                    std::cout << u;
                    for (uint64_t e = sm.off[u]; e < sm.off[u + 1]; e++) std::cout << "\t" << sm.sample[e] << ":" << sm.weight[e];
                    std::cout << "\n";
                }
                return 0;
            } else if (a == "--masses-samples-table") {  // TREE NAMES MASSES OUT: the per-sample table writer on its own (one name a line)
                const std::string tpath = val(), npath = val(), mpath = val(), opath = val();
                const rkh::Tree t = rkh::parse_newick(slurp(tpath));
                std::vector<std::string> names;
                {
                    std::istringstream ns(slurp(npath));
                    for (std::string line; std::getline(ns, line);) names.push_back(line);
                }
                const std::string raw = slurp(mpath);
                if (raw.size() % 8) throw std::runtime_error(mpath + ": not a whole number of 64-bit words");
                std::vector<uint64_t> m(raw.size() / 8);
                if (!m.empty()) memcpy(m.data(), raw.data(), raw.size());
                std::ofstream of(opath, std::ios::binary);
                if (!of) throw std::runtime_error("cannot write " + opath);
                of << rkh::masses_samples_table(t, names, m.data(), m.size());
                return 0;
            } else if (a == "--ingest-rate") {  // N3 throughput: FASTA parse, MD5 dedup, host-side packing (no device needed)
                const std::string text = slurp(val());
                auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
                const double t0 = now();
                const std::vector<rkh::Fasta> recs = rkh::read_fasta(text);
                const double t1 = now();
                const rkh::Dedup dd = rkh::dedup_index(recs);
                const double t2 = now();
                std::cout << recs.size() << " reads, " << dd.first_rec.size() << " unique, " << text.size() << " bytes\n"
                          << "parse " << recs.size() / (t1 - t0) / 1e6 << " Mreads/s (" << text.size() / (t1 - t0) / 1e6 << " MB/s)\n"
                          << "dedup " << recs.size() / (t2 - t1) / 1e6 << " Mreads/s\n";
                return 0;
            } else if (a == "--uniondb-stats") {  // load a `.union` file and say what it cost: rows, entries, peak resident memory (CPU tests)
                const std::string path = val();
                size_t rows, entries, nodes;
                {
                    const rkh::UnionDb db = rkh::load_uniondb(slurp(path));
                    rows = db.key_codes.size(); entries = db.scores.size(); nodes = db.tree.nodes.size();
                }
                struct rusage ru;
                getrusage(RUSAGE_SELF, &ru);
                std::cout << rows << " " << entries << " " << nodes << " " << ru.ru_maxrss << "\n";  // (ru_maxrss: kilobytes on Linux)
                return 0;
            } else if (a == "--load-uniondb") {  // what load_uniondb makes of a `.union` stream (compared with the Python twin)
                const rkh::UnionDb db = rkh::load_uniondb(slurp(val()));
                std::cout << db.alphabet << " " << db.k << " " << (db.convert_uo ? 1 : 0) << " " << (db.only_fakes ? 1 : 0) << " "
                          << rkh::java_float_to_string(db.thr) << " " << rkh::java_float_to_string(db.thr_log10) << " "
                          << rkh::java_float_to_string(db.omega) << " " << rkh::java_float_to_string(db.calibration) << " "
                          << db.key_codes.size() << " " << db.scores.size() << "\n" << rkh::jplace_newick(db.tree) << "\n";
                for (const auto &n : db.tree.nodes) std::cout << n.id << "\t" << n.label << "\t" << n.jplace_edge << "\t" << n.parent << "\n";
                for (size_t r = 0; r < db.key_codes.size(); r++) {
                    std::cout << db.key_codes[r];
                    for (uint64_t e = db.row_offsets[r]; e < db.row_offsets[r + 1]; e++)
                        std::cout << " " << db.branch_ids[e] << ":" << rkh::java_float_to_string(db.scores[e]);
                    std::cout << "\n";
                }
                return 0;
            } else if (a == "--load-jsondb") {
                const rkh::JsonDb db = rkh::load_jsondb(slurp(val()));
                std::cout << db.k << " " << rkh::java_float_to_string(db.thr) << " " << rkh::java_float_to_string(db.thr_log10) << " "
                          << db.key_codes.size() << " " << db.scores.size() << "\n" << db.original_tree << "\n";
                for (size_t r = 0; r < db.key_codes.size(); r++) {
                    std::cout << db.key_codes[r];
                    for (uint64_t e = db.row_offsets[r]; e < db.row_offsets[r + 1]; e++)
                        std::cout << " " << db.branch_ids[e] << ":" << rkh::java_float_to_string(db.scores[e]);
                    std::cout << "\n";
                }
                return 0;
            } else return usage();
        }
        const int n_sources = (jsondb.empty() ? 0 : 1) + (uniondb.empty() ? 0 : 1) + (dbimage.empty() ? 0 : 1);
        const bool masses_only = !masses_only_path.empty();
        if (masses_only && !masses_path.empty()) {
            std::cerr << "rk_place: --masses-only writes the table --masses writes, without placing into a jplace: give one of the two\n";
            return 2;
        }
        if (masses_only && !out.empty()) {
            std::cerr << "rk_place: --masses-only writes no jplace (the placements never reach the host): it cannot be combined with --out\n";
            return 2;
        }
        if (!edpl_path.empty() && out.empty()) {
            std::cerr << "rk_place: --edpl reads the placements of a run that writes a jplace: it needs --out (and cannot be combined with --masses-only)\n";
            return 2;
        }
        if (!sample_sep.empty() && !masses_only && masses_path.empty()) {
            std::cerr << "rk_place: --sample-sep names the samples of the per-edge tables: it needs --masses or --masses-only\n";
            return 2;
        }
        if (!kr_path.empty() && sample_sep.empty()) {
            std::cerr << "rk_place: --kr compares the samples of one run: it needs --sample-sep (with --masses or --masses-only)\n";
            return 2;
        }
        if (!squash_path.empty() && sample_sep.empty()) {
            std::cerr << "rk_place: --squash clusters the samples of one run: it needs --sample-sep (with --masses or --masses-only)\n";
            return 2;
        }
        if (!epca_path.empty() && sample_sep.empty()) {
            std::cerr << "rk_place: --epca finds the principal components of the samples of one run: it needs --sample-sep (with --masses or --masses-only)\n";
            return 2;
        }
        if (!epca_path.empty() && (epca_k < 1 || epca_k > RK_EPCA_MAX_COMPONENTS || epca_iters < 1 || epca_iters > 10000)) {
            std::cerr << "rk_place: --epca-components must be in 1..8, --epca-iters in 1..10000\n";
            return 2;
        }
        if (!kmeans_path.empty() && sample_sep.empty()) {
            std::cerr << "rk_place: --kmeans clusters the samples of one run: it needs --sample-sep (with --masses or --masses-only)\n";
            return 2;
        }
        if (!kmeans_path.empty() && (kmeans_k < 1 || kmeans_k > RK_KMEANS_MAX_K || kmeans_rounds < 1 || kmeans_rounds > RK_KMEANS_MAX_ROUNDS)) {
            std::cerr << "rk_place: --kmeans needs --kmeans-k in 1..64; --kmeans-rounds must be in 1..1024\n";
            return 2;
        }
        if (!diversity_path.empty() && sample_sep.empty()) {
            std::cerr << "rk_place: --diversity measures the samples of one run: it needs --sample-sep (with --masses or --masses-only)\n";
            return 2;
        }
        std::vector<double> thetas;  // --diversity-theta: numbers separated by commas
        bool thetas_ok = true;
        for (size_t at = 0; !diversity_theta.empty() && at <= diversity_theta.size();) {
            const size_t comma = std::min(diversity_theta.find(',', at), diversity_theta.size());
            const std::string item = diversity_theta.substr(at, comma - at);
            char *end = nullptr;
            const double v = strtod(item.c_str(), &end);
            thetas_ok = thetas_ok && !item.empty() && *end == 0 && v >= 0.0 && v <= 8.0;
            thetas.push_back(v);
            at = comma + 1;
        }
        if (!thetas_ok || thetas.size() > RK_DIVERSITY_MAX_THETA) {
            std::cerr << "rk_place: --diversity-theta takes at most 8 numbers in 0..8, separated by commas\n";
            return 2;
        }
        const bool only_convert = !save_image.empty() && fasta.empty() && out.empty() && !masses_only;
        if (n_sources != 1 || (!only_convert && (fasta.empty() || (out.empty() && !masses_only))) || (only_convert && !dbimage.empty())) return usage();
        uint32_t amb_mode;
        if (amb == "mean") amb_mode = RK_AMB_MEAN; else if (amb == "max") amb_mode = RK_AMB_MAX; else if (amb == "skip") amb_mode = RK_AMB_SKIP;
        else return usage();
        uint32_t strand;
        if (strand_name == "fwd") strand = RK_STRAND_FORWARD; else if (strand_name == "rev") strand = RK_STRAND_REVERSE; else if (strand_name == "both") strand = RK_STRAND_BOTH;
        else return usage();
        if (translate && strand != RK_STRAND_FORWARD) {
            std::cerr << "rk_place: --translate places every read in all six reading frames, both strands included: it cannot be combined with --strand rev | both\n";
            return 2;
        }
        std::vector<uint8_t> frame;  // (--translate only) the reading frame of every unique read's result
        // (fwd is rk_place_batch itself: the reference's behaviour, and this driver's before it knew about strands)
        auto place = [&](rk_db *h, const rk_params *pp, uint64_t m, const uint8_t *sq, const uint64_t *so, rk_result *rs, rk_counters *c) {
            if (translate) {
                frame.assign(m, (uint8_t)RK_FRAME_NONE);
                if (rk_place_batch_translated(h, pp, m, sq, so, rs, frame.data(), c) != RK_OK) throw std::runtime_error(std::string("rk_place_batch_translated: ") + rk_last_error());
                return;
            }
            const int rc = strand == RK_STRAND_FORWARD ? rk_place_batch(h, pp, m, sq, so, rs, c) : rk_place_batch_strands(h, pp, strand, m, sq, so, rs, c);
            if (rc != RK_OK) throw std::runtime_error(std::string(strand == RK_STRAND_FORWARD ? "rk_place_batch: " : "rk_place_batch_strands: ") + rk_last_error());
        };
        // --kr: the samples' distance matrix from the sample mass buffer -- `words` on the host, or nullptr: where the per-sample
        // profile-only call left it on the device -- over the database's tree, through rk_kr_distances_batch
        rk_db *kr_db = nullptr;  // (the handle, once it is open)
        // --squash: the same, through rk_squash_batch; `host_words` is the host's copy either way (it tells which samples hold mass)
        // --epca: the same, through rk_epca_batch and rk_epca_finish_host (one sample alone has no components: it is only counted)
        // --kmeans: the same, through rk_kmeans_batch
        // --diversity: the same, through rk_diversity_batch
        auto write_kr = [&](const rkh::Tree &t, const rkh::SampleMembers &sm, const uint64_t *words, const uint64_t *host_words) {
            if (kr_path.empty() && squash_path.empty() && epca_path.empty() && kmeans_path.empty() && diversity_path.empty()) return;
            const uint32_t B = (uint32_t)t.nodes.size(), S = (uint32_t)sm.names.size();
            std::vector<int32_t> parent(B);
            std::vector<float> bl(B);
            for (uint32_t x = 0; x < B; x++) { parent[x] = t.nodes[x].parent; bl[x] = t.nodes[x].bl; }
            rk_tree *kt = nullptr;
            if (rk_tree_create(device, B, parent.data(), bl.data(), &kt) != RK_OK) throw std::runtime_error(std::string("rk_tree_create: ") + rk_last_error());
            struct TreeGuard { rk_tree *p; ~TreeGuard() { rk_tree_destroy(p); } } tree_guard{kt};
            if (!kr_path.empty()) {
                std::vector<double> D((size_t)S * S);
                if (rk_kr_distances_batch(kr_db, kt, S, words, D.data()) != RK_OK) throw std::runtime_error(std::string("rk_kr_distances_batch: ") + rk_last_error());
                std::ofstream kf(kr_path, std::ios::binary);
                if (!kf) throw std::runtime_error("cannot write " + kr_path);
                kf << rkh::kr_table(sm.names, D.data());
            }
            if (!squash_path.empty()) {
                static_assert(sizeof(rkh::SquashRow) == sizeof(rk_squash_merge), "one row layout");
                std::vector<rkh::SquashRow> rows(S > 1 ? S - 1 : 0);
                uint32_t n_merges = 0;
                if (S > 1 && rk_squash_batch(kr_db, kt, S, words, (rk_squash_merge *)rows.data(), &n_merges) != RK_OK)
                    throw std::runtime_error(std::string("rk_squash_batch: ") + rk_last_error());
                std::vector<char> with_mass(S, 0);
                for (uint32_t s = 0; s < S; s++)
                    for (uint32_t x = 0; x < B && !with_mass[s]; x++) with_mass[s] = host_words[(size_t)s * (2 * (size_t)B + 4) + x] != 0;
                std::ofstream qf(squash_path, std::ios::binary);
                if (!qf) throw std::runtime_error("cannot write " + squash_path);
                qf << rkh::squash_table(sm.names, rows.data(), n_merges, with_mass);
            }
            if (!epca_path.empty()) {
                const uint32_t k = epca_k;
                uint32_t info[2] = {0, 0};
                std::vector<double> ev(k, 0.0), share(k, 0.0), res(k, 0.0), proj((size_t)S * k, 0.0), load((size_t)B * k, 0.0);
                if (S > 1) {
                    std::vector<double> raw((size_t)rk_epca_out_doubles(B, S, k));
                    if (rk_epca_batch(kr_db, kt, S, words, k, epca_iters, raw.data(), info) != RK_OK) throw std::runtime_error(std::string("rk_epca_batch: ") + rk_last_error());
                    if (rk_epca_finish_host(B, S, k, raw.data(), ev.data(), share.data(), res.data(), proj.data(), load.data()) != RK_OK)
                        throw std::runtime_error(std::string("rk_epca_finish_host: ") + rk_last_error());
                } else {
                    for (uint32_t s = 0; s < S; s++) {
                        bool any = false;
                        for (uint32_t x = 0; x < B && !any; x++) any = host_words[(size_t)s * (2 * (size_t)B + 4) + x] != 0;
                        info[0] += any;
                    }
                }
                std::ofstream ef(epca_path, std::ios::binary);
                if (!ef) throw std::runtime_error("cannot write " + epca_path);
                ef << rkh::epca_table(sm.names, B, k, epca_iters, info[0], info[1], ev.data(), share.data(), res.data(), proj.data(), load.data());
            }
            if (!kmeans_path.empty()) {
                const uint32_t k = kmeans_k;
                std::vector<uint32_t> assign(S), sizes(k);
                std::vector<double> dist(S), within(k);
                uint32_t info[4] = {0, 0, 0, 0};
                if (rk_kmeans_batch(kr_db, kt, S, words, k, kmeans_rounds, nullptr, assign.data(), dist.data(), sizes.data(), within.data(), info, nullptr) != RK_OK)
                    throw std::runtime_error(std::string("rk_kmeans_batch: ") + rk_last_error());
                std::ofstream mf(kmeans_path, std::ios::binary);
                if (!mf) throw std::runtime_error("cannot write " + kmeans_path);
                mf << rkh::kmeans_table(sm.names, k, assign.data(), dist.data(), sizes.data(), within.data(), info);
            }
            if (!diversity_path.empty()) {
                std::vector<double> values((size_t)S * (RK_DIVERSITY_FIXED + 2 * thetas.size()));
                if (rk_diversity_batch(kr_db, kt, S, words, (uint32_t)thetas.size(), thetas.empty() ? nullptr : thetas.data(), values.data()) != RK_OK)
                    throw std::runtime_error(std::string("rk_diversity_batch: ") + rk_last_error());
                std::ofstream df(diversity_path, std::ios::binary);
                if (!df) throw std::runtime_error("cannot write " + diversity_path);
                df << rkh::diversity_table(sm.names, thetas, values.data());
            }
        };
        // --edpl: the EDPL of every unique read from the results on the host, over the database's tree as --epca builds it, through
        // rk_edpl_batch; a line per FASTA record that has a placement
        auto write_edpl = [&](const rkh::Tree &t, uint64_t m, const rk_result *rs, size_t n_records, auto header_of, const uint32_t *uniq_of_rec) {
            if (edpl_path.empty()) return;
            const uint32_t B = (uint32_t)t.nodes.size();
            std::vector<int32_t> parent(B);
            std::vector<float> bl(B);
            for (uint32_t x = 0; x < B; x++) { parent[x] = t.nodes[x].parent; bl[x] = t.nodes[x].bl; }
            rk_tree *kt = nullptr;
            if (rk_tree_create(device, B, parent.data(), bl.data(), &kt) != RK_OK) throw std::runtime_error(std::string("rk_tree_create: ") + rk_last_error());
            struct TreeGuard { rk_tree *p; ~TreeGuard() { rk_tree_destroy(p); } } tree_guard{kt};
            std::vector<double> edpl(m, 0.0);
            if (rk_edpl_batch(kr_db, kt, keep_at_most, m, rs, edpl.data()) != RK_OK) throw std::runtime_error(std::string("rk_edpl_batch: ") + rk_last_error());
            std::ofstream ef(edpl_path, std::ios::binary);
            if (!ef) throw std::runtime_error("cannot write " + edpl_path);
            ef << rkh::edpl_table(n_records, header_of, uniq_of_rec, rs->n_rows, edpl.data());
        };
        // --masses: the per-edge table of the whole run.  The results are on the host already, so the sums are rk_masses_accumulate_host's;
        // the weight of a unique read is the number of FASTA records it stands for, so the table speaks of reads
        // (--sample-sep: `sm` holds the samples and the membership entries of the unique reads, and the table is one per sample)
        auto write_masses = [&](const rkh::Tree &t, uint64_t m, const rk_result *rs, const uint32_t *w, uint32_t n_threads, const rkh::SampleMembers *sm) {
            if (sm) {
                const uint32_t S = (uint32_t)sm->names.size();
                std::vector<uint64_t> words((size_t)rk_masses_samples_words((uint32_t)t.nodes.size(), S), 0);
                if (words.empty()) throw std::runtime_error("--masses --sample-sep: " + std::to_string(sm->names.size()) + " samples on this tree are beyond the limits of a sample mass buffer");
                std::vector<uint32_t> reads(sm->sample.size());
                for (uint64_t r = 0; r < m; r++)
                    for (uint64_t e = sm->off[r]; e < sm->off[r + 1]; e++) reads[e] = (uint32_t)r;
                if (rk_masses_accumulate_samples_host((uint32_t)t.nodes.size(), keep_at_most, m, rs, S, reads.size(), reads.data(), sm->sample.data(), sm->weight.data(),
                                                      words.data(), n_threads) != RK_OK)
                    throw std::runtime_error(std::string("rk_masses_accumulate_samples_host: ") + rk_last_error());
                std::ofstream mf(masses_path, std::ios::binary);
                if (!mf) throw std::runtime_error("cannot write " + masses_path);
                mf << rkh::masses_samples_table(t, sm->names, words.data(), words.size());
                write_kr(t, *sm, words.data(), words.data());
                return;
            }
            std::vector<uint64_t> words((size_t)rk_masses_words((uint32_t)t.nodes.size()), 0);
            if (words.empty()) throw std::runtime_error("--masses: the tree has no nodes, or more than 65535");
            if (rk_masses_accumulate_host((uint32_t)t.nodes.size(), keep_at_most, m, rs, w, words.data(), n_threads) != RK_OK)
                throw std::runtime_error(std::string("rk_masses_accumulate_host: ") + rk_last_error());
            std::ofstream mf(masses_path, std::ios::binary);
            if (!mf) throw std::runtime_error("cannot write " + masses_path);
            mf << rkh::masses_table(t, words.data(), words.size());
        };
        // --masses-only: one profile-only call with the multiplicities as weights -- every chunk is summed on the device, the flags
        // alone come back -- then the table through the same writer
        auto place_masses_only = [&](rk_db *h, const rk_params *pp, const rkh::Tree &t, uint64_t m, const uint8_t *sq, const uint64_t *so, const uint32_t *w,
                                     uint32_t *flags_out, rk_counters *c, const rkh::SampleMembers *sm) {
            if (sm) {  // --sample-sep: one per-sample call, the membership CSR in place of the weights
                const uint32_t S = (uint32_t)sm->names.size();
                std::vector<uint64_t> words((size_t)rk_masses_samples_words((uint32_t)t.nodes.size(), S), 0);
                if (words.empty()) throw std::runtime_error("--masses-only --sample-sep: " + std::to_string(sm->names.size()) + " samples on this tree are beyond the limits of a sample mass buffer");
                if (rk_place_batch_masses_samples(h, pp, translate ? RK_STEP_TRANSLATED : strand, m, sq, so, S, sm->off.data(), sm->sample.data(), sm->weight.data(),
                                                  words.data(), flags_out, c) != RK_OK)
                    throw std::runtime_error(std::string("rk_place_batch_masses_samples: ") + rk_last_error());
                std::ofstream mf(masses_only_path, std::ios::binary);
                if (!mf) throw std::runtime_error("cannot write " + masses_only_path);
                mf << rkh::masses_samples_table(t, sm->names, words.data(), words.size());
                write_kr(t, *sm, nullptr, words.data());  // (the buffer is still on the device in the handle)
                return;
            }
            std::vector<uint64_t> words((size_t)rk_masses_words((uint32_t)t.nodes.size()), 0);
            if (words.empty()) throw std::runtime_error("--masses-only: the tree has no nodes, or more than 65535");
            if (rk_place_batch_masses(h, pp, translate ? RK_STEP_TRANSLATED : strand, m, sq, so, w, words.data(), flags_out, c) != RK_OK)
                throw std::runtime_error(std::string("rk_place_batch_masses: ") + rk_last_error());
            std::ofstream mf(masses_only_path, std::ios::binary);
            if (!mf) throw std::runtime_error("cannot write " + masses_only_path);
            mf << rkh::masses_table(t, words.data(), words.size());
        };
        auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double t_start = now();

        rkh::JsonDb jd;
        rkh::UnionDb ud;
        rkh::Tree tree;
        rk_db_desc d;
        memset(&d, 0, sizeof(d));
        rk_db *db = nullptr;
        if (!dbimage.empty()) {
            // the engine's own image: the reference tree travels in its user blob (rkh::tree_to_blob)
            uint64_t len = 0;
            if (rk_db_image_user(dbimage.c_str(), nullptr, 0, &len) != RK_OK) throw std::runtime_error(std::string("rk_db_image_user: ") + rk_last_error());
            std::string blob((size_t)len, '\0');
            if (len && rk_db_image_user(dbimage.c_str(), blob.data(), len, &len) != RK_OK) throw std::runtime_error(std::string("rk_db_image_user: ") + rk_last_error());
            tree = rkh::tree_from_blob(blob);
            if (rk_db_load(dbimage.c_str(), device, &db) != RK_OK) throw std::runtime_error(std::string("rk_db_load: ") + rk_last_error());
            rk_db_info info;
            (void)rk_db_get_info(db, &info);
            if (info.n_branches != tree.nodes.size()) throw std::runtime_error("database image: the tree has " + std::to_string(tree.nodes.size()) + " nodes, the database " + std::to_string(info.n_branches) + " branches");
        } else {
            if (!uniondb.empty()) {
                ud = rkh::load_uniondb(slurp(uniondb));
                tree = ud.tree;
                d.alphabet = ud.alphabet == 4 ? RK_ALPHABET_DNA : RK_ALPHABET_AA; d.convert_uo = ud.convert_uo ? 1 : 0; d.k = ud.k;
                d.thr_log10 = ud.thr_log10; d.thr = ud.thr; d.n_keys = ud.key_codes.size();
                d.key_codes = ud.key_codes.data(); d.row_offsets = ud.row_offsets.data(); d.branch_ids = ud.branch_ids.data(); d.scores = ud.scores.data();
            } else {
                jd = rkh::load_jsondb(slurp(jsondb));
                tree = rkh::parse_newick(jd.original_tree);
                d.alphabet = RK_ALPHABET_DNA; d.k = jd.k;
                d.thr_log10 = jd.thr_log10; d.thr = jd.thr; d.n_keys = jd.key_codes.size();
                d.key_codes = jd.key_codes.data(); d.row_offsets = jd.row_offsets.data(); d.branch_ids = jd.branch_ids.data(); d.scores = jd.scores.data();
            }
            d.n_branches = (uint32_t)tree.nodes.size();
            d.device = device; d.table_mode = RK_TABLE_AUTO;
            if (!save_image.empty()) {  // (built on the host: a machine without a GPU can write the image a placement node loads)
                const std::string blob = rkh::tree_to_blob(tree);
                if (rk_db_save_desc(&d, save_image.c_str(), blob.data(), blob.size()) != RK_OK) throw std::runtime_error(std::string("rk_db_save_desc: ") + rk_last_error());
                if (only_convert) { std::cerr << "database image -> " << save_image << "\n"; return 0; }
            }
            if (rk_db_create(&d, &db) != RK_OK) throw std::runtime_error(std::string("rk_db_create: ") + rk_last_error());
        }
        struct DbGuard { rk_db *p; ~DbGuard() { if (p) rk_db_destroy(p); } } db_guard{db};
        kr_db = db;
        if (translate) {
            rk_db_info info;
            if (rk_db_get_info(db, &info) != RK_OK) throw std::runtime_error(std::string("rk_db_get_info: ") + rk_last_error());
            if (info.alphabet != RK_ALPHABET_AA)
                throw std::runtime_error("--translate needs an amino-acid database (this one holds DNA: DNA reads are placed on it as they are, see --strand)");
        }
        const double t_db = now();
        const uint32_t K = keep_at_most;
        rk_params p{K, keep_factor, amb_mode, nsbound};
        namespace fs = std::filesystem;
        const fs::path log_dir = logs_given ? fs::path(logs) : fs::absolute(fs::path(out.empty() ? masses_only_path : out)).parent_path() / "logs";
        const std::string notplaced_name = "notplaced_" + fs::path(fasta).filename().string() + ".tsv";
        const std::string reversed_name = "reversed_" + fs::path(fasta).filename().string() + ".tsv";  // (--strand rev | both only)
        const std::string frames_name = "frames_" + fs::path(fasta).filename().string() + ".tsv";      // (--translate only)

        if (!classic) {
            // ---- every host thread on every pass (rk_fastio.hpp) ----
            unsigned hw = std::thread::hardware_concurrency();
            rkh::Team team(threads ? threads : std::max(1u, std::min(hw ? hw : 1u, 32u)));
            // the engine's first batch of a process sets up its workspaces and has its kernels loaded to the device (~100 ms): started
            // here, on a thread of its own, next to the mapping and the scan of the query file (engine start-up, like the database load)
            double warm_s = 0;
            std::thread warm([&]() { const double w0 = now(); (void)rk_reserve_host_path(db, K, 320); warm_s = now() - w0; });
            struct JoinWarm { std::thread &t; ~JoinWarm() { if (t.joinable()) t.join(); } } join_warm{warm};
            rkh::MappedFile fa;
            fa.open_file(fasta);
            const double t0 = now();
            const rkh::FastaScan sc = rkh::scan_fasta(fa.data, fa.size, team, md5_dedup);
            const double t1 = now();
            const rkh::FastDedup dd = rkh::dedup_fast(sc, team);
            const double t2 = now();
            rkh::RawArray<char> seq;
            rkh::RawArray<uint64_t> off;
            rkh::gather_unique(sc, dd, team, seq, off);
            const size_t n = dd.first_rec.size();
            rkh::SampleMembers members;  // (--sample-sep only)
            if (!sample_sep.empty())
                members = rkh::sample_members(sc.recs.size(), n, [&](size_t r) { return std::make_pair((const char *)sc.recs[r].hdr, (size_t)sc.recs[r].hdr_len); },
                                              dd.uniq_of_rec.data(), sample_sep[0]);
            const rkh::SampleMembers *sm = sample_sep.empty() ? nullptr : &members;
            auto count_weights = [&](rkh::RawArray<uint32_t> &weight) {  // a unique read weighs the FASTA records it stands for
                weight.alloc(n);
                team.run([&](unsigned t, unsigned T) {
                    for (size_t u = n * t / T; u < n * (t + 1) / T; u++) {
                        uint32_t c = 0;
                        for (uint32_t rec = dd.first_rec[u]; rec != 0xFFFFFFFFu; rec = dd.next_dup[rec]) c++;
                        weight[u] = c;
                    }
                });
            };
            if (masses_only) {
                rkh::RawArray<uint32_t> weight, flags;
                count_weights(weight);
                flags.alloc(n);
                team.run([&](unsigned t, unsigned T) { memset(flags.data() + n * t / T, 0, (n * (t + 1) / T - n * t / T) * 4); });
                const double t3 = now();
                warm.join();
                const double t3b = now();
                rk_counters ct{};
                place_masses_only(db, &p, tree, n, (const uint8_t *)seq.data(), off.data(), weight.data(), flags.data(), &ct, sm);
                const double t4 = now();
                fs::create_directories(log_dir);
                {
                    std::ofstream nf(log_dir / notplaced_name, std::ios::binary);
                    if (!nf) throw std::runtime_error("cannot write the notplaced log under " + log_dir.string());
                    nf << rkh::notplaced_log_fast(sc, dd, flags.data());
                }
                if (strand != RK_STRAND_FORWARD) {
                    std::ofstream rf(log_dir / reversed_name, std::ios::binary);
                    if (!rf) throw std::runtime_error("cannot write the reversed log under " + log_dir.string());
                    rf << rkh::flagged_log_fast(sc, dd, flags.data(), RK_FLAG_REVERSE, RK_FLAG_REVERSE);
                }
                const double t5 = now();
                std::cerr << n << " unique reads, " << ct.placed << " placed -> " << masses_only_path << "\n";
                if (timing) {
                    char buf[600];
                    snprintf(buf, sizeof(buf),
                             "{\"mode\": \"masses_only\", \"reads\": %zu, \"unique\": %zu, \"placed\": %llu, \"fasta_bytes\": %zu, \"threads\": %u, \"db_s\": %.6f, "
                             "\"engine_warm_up_s\": %.6f, \"scan_s\": %.6f, \"dedup_s\": %.6f, \"gather_s\": %.6f, \"place_and_sum_s\": %.6f, "
                             "\"place_wait_for_warm_up_s\": %.6f, \"logs_s\": %.6f, \"fasta_to_masses_s\": %.6f}",
                             sc.recs.size(), n, (unsigned long long)ct.placed, fa.size, team.size(), t_db - t_start, warm_s, t1 - t0, t2 - t1, t3 - t2, t4 - t3,
                             t3b - t3, t5 - t4, t5 - t0);
                    std::cout << buf << std::endl;
                }
                return 0;
            }
            rkh::RawArray<uint8_t> n_rows;
            rkh::RawArray<uint16_t> branch;
            rkh::RawArray<float> score;
            rkh::RawArray<double> lwr;
            rkh::RawArray<uint32_t> flags;
            n_rows.alloc(n); branch.alloc(n * K); score.alloc(n * K); lwr.alloc(n * K); flags.alloc(n);
            team.run([&](unsigned t, unsigned T) {  // (first touch by every thread at once, not by the engine's few result-copy threads)
                const size_t lo = n * t / T, hi = n * (t + 1) / T;
                memset(n_rows.data() + lo, 0, hi - lo); memset(flags.data() + lo, 0, (hi - lo) * 4);
                memset(branch.data() + lo * K, 0, (hi - lo) * K * 2); memset(score.data() + lo * K, 0, (hi - lo) * K * 4); memset(lwr.data() + lo * K, 0, (hi - lo) * K * 8);
            });
            const double t3 = now();
            warm.join();
            const double t3b = now();
            rk_result res{n_rows.data(), branch.data(), score.data(), lwr.data(), flags.data()};
            rk_counters ct;
            place(db, &p, n, (const uint8_t *)seq.data(), off.data(), &res, &ct);
            const double t4 = now();
            const rkh::FastWriteStats ws = rkh::write_jplace_fast(out, tree, sc, dd, K, n_rows.data(), branch.data(), score.data(), lwr.data(), call, guppy, team);
            const double t5 = now();
            fs::create_directories(log_dir);
            {
                std::ofstream nf(log_dir / notplaced_name, std::ios::binary);
                if (!nf) throw std::runtime_error("cannot write the notplaced log under " + log_dir.string());
                nf << rkh::notplaced_log_fast(sc, dd, flags.data());
            }
            if (strand != RK_STRAND_FORWARD) {
                std::ofstream rf(log_dir / reversed_name, std::ios::binary);
                if (!rf) throw std::runtime_error("cannot write the reversed log under " + log_dir.string());
                rf << rkh::flagged_log_fast(sc, dd, flags.data(), RK_FLAG_REVERSE, RK_FLAG_REVERSE);
            }
            if (translate) {
                std::ofstream ff(log_dir / frames_name, std::ios::binary);
                if (!ff) throw std::runtime_error("cannot write the frames log under " + log_dir.string());
                ff << rkh::frames_log_fast(sc, dd, frame.data());
            }
            if (!masses_path.empty()) {
                rkh::RawArray<uint32_t> weight;
                count_weights(weight);
                write_masses(tree, n, &res, weight.data(), team.size(), sm);
            }
            write_edpl(tree, n, &res, sc.recs.size(), [&](size_t r) { return std::make_pair((const char *)sc.recs[r].hdr, (size_t)sc.recs[r].hdr_len); }, dd.uniq_of_rec.data());
            const double t6 = now();
            std::cerr << n << " unique reads, " << ws.placed << " placed -> " << out << "\n";
            if (timing) {  // one JSON line (bench.py's fasta_to_jplace leg reads it): seconds per pass, FASTA bytes in -> jplace bytes out
                char buf[700];
                snprintf(buf, sizeof(buf),
                         "{\"reads\": %zu, \"unique\": %zu, \"placed\": %llu, \"fasta_bytes\": %zu, \"jplace_bytes\": %llu, \"threads\": %u, \"db_s\": %.6f, \"engine_warm_up_s\": %.6f, \"scan_s\": %.6f, "
                         "\"dedup_s\": %.6f, \"gather_s\": %.6f, \"place_s\": %.6f, \"place_wait_for_warm_up_s\": %.6f, \"write_s\": %.6f, \"write_format_s\": %.6f, \"write_io_s\": %.6f, \"notplaced_log_s\": %.6f, \"fasta_to_jplace_s\": %.6f, "
                         "\"exact_writer\": %s}",
                         sc.recs.size(), n, (unsigned long long)ws.placed, fa.size, (unsigned long long)ws.bytes, team.size(), t_db - t_start, warm_s, t1 - t0, t2 - t1, t3 - t2,
                         t4 - t3, t3b - t3, t5 - t4, ws.format_s, ws.io_s, t6 - t5, t5 - t0, ws.exact_path ? "true" : "false");
                std::cout << buf << std::endl;
            }
            return 0;
        }

        // ---- the one-string-at-a-time path of rk_hostio.hpp (the definition the fast path is held to) ----
        const double tc0 = now();
        const std::vector<rkh::Fasta> records = rkh::read_fasta(slurp(fasta));
        const rkh::Dedup dd = rkh::dedup_index(records);
        const std::vector<std::vector<std::string>> names = rkh::dedup_names(records, dd);
        const size_t n = dd.first_rec.size();
        std::string seq;
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + records[dd.first_rec[i]].seq.size();
        seq.reserve(off[n]);
        for (size_t i = 0; i < n; i++) seq += records[dd.first_rec[i]].seq;
        rkh::SampleMembers members;  // (--sample-sep only)
        if (!sample_sep.empty())
            members = rkh::sample_members(records.size(), n, [&](size_t r) { return std::make_pair(records[r].header.data(), records[r].header.size()); },
                                          dd.uniq_of_rec.data(), sample_sep[0]);
        const rkh::SampleMembers *sm = sample_sep.empty() ? nullptr : &members;
        if (masses_only) {
            std::vector<uint32_t> weight(n), flags(n, 0);
            for (size_t i = 0; i < n; i++) weight[i] = (uint32_t)names[i].size();
            rk_counters ct{};
            place_masses_only(db, &p, tree, n, (const uint8_t *)seq.data(), off.data(), weight.data(), flags.data(), &ct, sm);
            fs::create_directories(log_dir);
            std::ofstream nf(log_dir / notplaced_name, std::ios::binary);
            if (!nf) throw std::runtime_error("cannot write the notplaced log under " + log_dir.string());
            nf << rkh::notplaced_log(records, dd, flags.data());
            if (strand != RK_STRAND_FORWARD) {
                std::ofstream rf(log_dir / reversed_name, std::ios::binary);
                if (!rf) throw std::runtime_error("cannot write the reversed log under " + log_dir.string());
                rf << rkh::flagged_log(records, dd, flags.data(), RK_FLAG_REVERSE, RK_FLAG_REVERSE);
            }
            std::cerr << n << " unique reads, " << ct.placed << " placed -> " << masses_only_path << "\n";
            if (timing) std::cout << "{\"mode\": \"masses_only\", \"reads\": " << records.size() << ", \"unique\": " << n << ", \"db_s\": " << (t_db - t_start) << ", \"fasta_to_masses_s\": " << (now() - tc0) << ", \"classic\": true}" << std::endl;
            return 0;
        }
        std::vector<uint8_t> n_rows(n);
        std::vector<uint16_t> branch(n * K);
        std::vector<float> score(n * K);
        std::vector<double> lwr(n * K);
        std::vector<uint32_t> flags(n);
        rk_result res{n_rows.data(), branch.data(), score.data(), lwr.data(), flags.data()};
        rk_counters ct;
        place(db, &p, n, (const uint8_t *)seq.data(), off.data(), &res, &ct);

        const auto pl = rkh::jplace_placements(tree, names, n, K, n_rows.data(), branch.data(), score.data(), lwr.data(), guppy);
        std::ofstream of(out, std::ios::binary);
        if (!of) throw std::runtime_error("cannot write " + out);
        of << rkh::jplace_document(tree, pl, call, guppy);
        {   // notplaced_<query>.tsv under logs/ next to the output, as the reference's workdir/logs (Main_PLACEMENT_v07.java:208-214)
            fs::create_directories(log_dir);
            std::ofstream nf(log_dir / notplaced_name, std::ios::binary);
            if (!nf) throw std::runtime_error("cannot write the notplaced log under " + log_dir.string());
            nf << rkh::notplaced_log(records, dd, flags.data());
            if (strand != RK_STRAND_FORWARD) {
                std::ofstream rf(log_dir / reversed_name, std::ios::binary);
                if (!rf) throw std::runtime_error("cannot write the reversed log under " + log_dir.string());
                rf << rkh::flagged_log(records, dd, flags.data(), RK_FLAG_REVERSE, RK_FLAG_REVERSE);
            }
            if (translate) {
                std::ofstream ff(log_dir / frames_name, std::ios::binary);
                if (!ff) throw std::runtime_error("cannot write the frames log under " + log_dir.string());
                ff << rkh::frames_log(records, dd, frame.data());
            }
        }
        if (!masses_path.empty()) {
            std::vector<uint32_t> weight(n);
            for (size_t i = 0; i < n; i++) weight[i] = (uint32_t)names[i].size();
            write_masses(tree, n, &res, weight.data(), 1, sm);
        }
        write_edpl(tree, n, &res, records.size(), [&](size_t r) { return std::make_pair(records[r].header.data(), records[r].header.size()); }, dd.uniq_of_rec.data());
        std::cerr << n << " unique reads, " << pl.size() << " placed -> " << out << "\n";
        if (timing) std::cout << "{\"reads\": " << records.size() << ", \"unique\": " << n << ", \"db_s\": " << (t_db - t_start) << ", \"fasta_to_jplace_s\": " << (now() - tc0) << ", \"classic\": true}" << std::endl;
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "rk_place: " << e.what() << "\n";
        return 1;
    }
}
