// rk_place's host-side pieces on their own (no device needed): the sub-commands the CPU tests hold against the Python twin
// (rappas_amd/hostio.py) and the host passes' rate probes.  A sub-command is met in the option loop of rk_place_main.cpp, reads its
// own values from there on, and sees the options that stand before it (--threads, --md5-dedup, --keep-at-most, --guppy-compat).
// Above them the few helpers they share with the driver: slurp, write_text, now, and the option loop's cursor.
#pragma once
#include <chrono>
#include <fstream>
#include <iostream>
#include <sstream>

#include <sys/resource.h>

#include "rk_hostio.hpp"
#include "rk_fastio.hpp"

static std::string slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::ostringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// (every file the driver writes goes through here)
static void write_text(const std::string &path, const std::string &text, const std::string &what = std::string()) {
    std::ofstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot write " + (what.empty() ? path : what));
    f << text;
}

static std::vector<uint64_t> slurp_words(const std::string &path) {
    const std::string raw = slurp(path);
    if (raw.size() % 8) throw std::runtime_error(path + ": not a whole number of 64-bit words");
    std::vector<uint64_t> m(raw.size() / 8);
    if (!m.empty()) memcpy(m.data(), raw.data(), raw.size());
    return m;
}

// the command line and the place the option loop has reached in it
struct Args {
    int argc;
    char **argv;
    int i;
    std::string val(const std::string &a) {
        if (i + 1 >= argc) throw std::runtime_error("missing value after " + a);
        return argv[++i];
    }
};

// option `a` as a host-only sub-command: its exit code, or -1 if it is none
static int host_subcommand(const std::string &a, Args &args, unsigned threads, bool md5_dedup, uint32_t keep_at_most, bool guppy, const std::string &call) {
    auto val = [&]() { return args.val(a); };
    if (a == "--emit-tree") {
        const rkh::Tree t = rkh::parse_newick(slurp(val()));
        std::cout << rkh::jplace_newick(t) << "\n" << rkh::write_newick(t, false, false, false) << "\n" << (t.rooted() ? "rooted" : "unrooted");
        for (const auto &n : t.nodes) std::cout << "\n" << n.id << "\t" << n.label << "\t" << n.jplace_edge << "\t" << n.parent;
        std::cout << "\n";
    } else if (a == "--format-float") {
        std::cout << rkh::java_float_to_string(strtof(val().c_str(), nullptr)) << "\n";
    } else if (a == "--format-double") {
        std::cout << rkh::java_double_to_string(strtod(val().c_str(), nullptr)) << "\n";
    } else if (a == "--md5") {
        for (uint8_t b : rkh::md5(val())) printf("%02x", b);
        printf("\n");
    } else if (a == "--dedup") {
        std::vector<rkh::Fasta> uniq;
        std::vector<std::vector<std::string>> names;
        rkh::dedup_reads(rkh::read_fasta(slurp(val())), uniq, names);
        for (size_t r = 0; r < uniq.size(); r++) {
            std::cout << uniq[r].seq;
            for (const auto &n : names[r]) std::cout << "\t" << n;
            std::cout << "\n";
        }
    } else if (a == "--fast-rate") {  // FASTA [TREE]: the fast path's host passes on their own, timed (no device needed); with a tree also the writer, on made-up placements
        const std::string path = val();
        const std::string tpath = (args.i + 1 < args.argc && args.argv[args.i + 1][0] != '-') ? val() : std::string();
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
    } else if (a == "--masses-table") {  // TREE MASSES OUT: the table writer on its own (compared with the Python twin)
        const std::string tpath = val(), mpath = val(), opath = val();
        const rkh::Tree t = rkh::parse_newick(slurp(tpath));
        const std::vector<uint64_t> m = slurp_words(mpath);
        write_text(opath, rkh::masses_table(t, m.data(), m.size()));
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
    } else if (a == "--masses-samples-table") {  // TREE NAMES MASSES OUT: the per-sample table writer on its own (one name a line)
        const std::string tpath = val(), npath = val(), mpath = val(), opath = val();
        const rkh::Tree t = rkh::parse_newick(slurp(tpath));
        std::vector<std::string> names;
        std::istringstream ns(slurp(npath));
        for (std::string line; std::getline(ns, line);) names.push_back(line);
        const std::vector<uint64_t> m = slurp_words(mpath);
        write_text(opath, rkh::masses_samples_table(t, names, m.data(), m.size()));
    } else if (a == "--ingest-rate") {  // N3 throughput: FASTA parse, MD5 dedup, host-side packing (no device needed)
        const std::string text = slurp(val());
        const double t0 = now();
        const std::vector<rkh::Fasta> recs = rkh::read_fasta(text);
        const double t1 = now();
        const rkh::Dedup dd = rkh::dedup_index(recs);
        const double t2 = now();
        std::cout << recs.size() << " reads, " << dd.first_rec.size() << " unique, " << text.size() << " bytes\n"
                  << "parse " << recs.size() / (t1 - t0) / 1e6 << " Mreads/s (" << text.size() / (t1 - t0) / 1e6 << " MB/s)\n"
                  << "dedup " << recs.size() / (t2 - t1) / 1e6 << " Mreads/s\n";
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
    } else {
        return -1;
    }
    return 0;
}
