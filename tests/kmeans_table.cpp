// rkh::kmeans_table (rappas_amd/csrc/host/rk_hostio.hpp) on its own: NAMES.txt (one name a line), K and RUN.bin -- raw little-endian
// assign [S] (32-bit), sizes [k] (32-bit), info [4] (32-bit), then dist [S] and within [k] (binary64) -- -> the table on stdout.
// tests/test_kmeans_host.py compares it byte for byte with hostio.kmeans_table.
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
    const size_t S = names.size(), k = strtoul(argv[2], nullptr, 10);
    std::ifstream f(argv[3], std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string raw = ss.str();
    if (raw.size() != (S + k + 4) * 4 + (S + k) * 8) return 3;
    std::vector<uint32_t> words(S + k + 4);
    std::vector<double> doubles(S + k);
    memcpy(words.data(), raw.data(), words.size() * 4);
    if (!doubles.empty()) memcpy(doubles.data(), raw.data() + words.size() * 4, doubles.size() * 8);
    std::cout << rkh::kmeans_table(names, (uint32_t)k, words.data(), doubles.data(), words.data() + S, doubles.data() + S, words.data() + S + k);
    return 0;
}
