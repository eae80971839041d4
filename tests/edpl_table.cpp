// rkh::edpl_table (rappas_amd/csrc/host/rk_hostio.hpp) on its own: HEADERS.txt (one header a line), UNIQ.bin (raw uint32: the unique
// read of every record), NROWS.bin (raw bytes, one per unique read) and EDPL.bin (raw doubles, one per unique read) -> the table on
// stdout.  tests/test_edpl_host.py compares it byte for byte with hostio.edpl_table.
#include "host/rk_hostio.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

static std::string slurp_file(const char *path) {
    std::ifstream f(path, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    std::vector<std::string> headers;
    {
        std::ifstream f(argv[1]);
        for (std::string line; std::getline(f, line);) headers.push_back(line);
    }
    const std::string uniq_raw = slurp_file(argv[2]), rows_raw = slurp_file(argv[3]), edpl_raw = slurp_file(argv[4]);
    const size_t n_unique = rows_raw.size();
    if (uniq_raw.size() != headers.size() * sizeof(uint32_t) || edpl_raw.size() != n_unique * sizeof(double)) return 3;
    std::vector<uint32_t> uniq(headers.size());
    std::vector<double> edpl(n_unique);
    if (!uniq.empty()) memcpy(uniq.data(), uniq_raw.data(), uniq_raw.size());
    if (n_unique) memcpy(edpl.data(), edpl_raw.data(), edpl_raw.size());
    for (uint32_t u : uniq)
        if (u >= n_unique) return 4;
    std::cout << rkh::edpl_table(headers.size(), [&](size_t r) { return std::make_pair(headers[r].data(), headers[r].size()); }, uniq.data(),
                                 (const uint8_t *)rows_raw.data(), edpl.data());
    return 0;
}
