// rkh::squash_table (rappas_amd/csrc/host/rk_hostio.hpp) on its own: NAMES.txt (one name a line), MERGES.bin (raw 24-byte rows),
// N_MERGES and MASS.txt (one 0 or 1 a line: the samples with mass) -> the table on stdout.  tests/test_squash_host.py compares it
// byte for byte with hostio.squash_table.
#include "host/rk_hostio.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    std::vector<std::string> names;
    {
        std::ifstream f(argv[1]);
        for (std::string line; std::getline(f, line);) names.push_back(line);
    }
    std::ifstream f(argv[2], std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string raw = ss.str();
    if (names.empty() || raw.size() != (names.size() - 1) * sizeof(rkh::SquashRow)) return 3;
    std::vector<rkh::SquashRow> rows(names.size() - 1);
    if (!raw.empty()) memcpy(rows.data(), raw.data(), raw.size());
    std::vector<char> with_mass;
    {
        std::ifstream g(argv[4]);
        for (std::string line; std::getline(g, line);) with_mass.push_back(line == "1");
    }
    if (with_mass.size() != names.size()) return 4;
    std::cout << rkh::squash_table(names, rows.data(), (uint32_t)strtoul(argv[3], nullptr, 10), with_mass);
    return 0;
}
