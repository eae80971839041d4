// rkh::diversity_table (rappas_amd/csrc/host/rk_hostio.hpp) on its own: NAMES.txt (one name a line), N_THETA and RUN.bin -- raw
// little-endian binary64: theta [n_theta], then values [S][5 + 2 n_theta] -- -> the table on stdout.
// tests/test_diversity_host.py compares it byte for byte with hostio.diversity_table.
#include "host/rk_hostio.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    std::vector<std::string> names;
    {
        std::ifstream f(argv[1]);
        for (std::string line; std::getline(f, line);) names.push_back(line);
    }
    const size_t S = names.size(), n = strtoul(argv[2], nullptr, 10);
    std::ifstream f(argv[3], std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string raw = ss.str();
    if (raw.size() != (n + S * (5 + 2 * n)) * 8) return 3;
    std::vector<double> doubles(raw.size() / 8);
    if (!doubles.empty()) memcpy(doubles.data(), raw.data(), raw.size());
    const std::vector<double> theta(doubles.begin(), doubles.begin() + n);
    std::cout << rkh::diversity_table(names, theta, doubles.data() + n);
    return 0;
}
