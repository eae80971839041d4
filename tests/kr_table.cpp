// rkh::kr_table (rappas_amd/csrc/host/rk_hostio.hpp) on its own: NAMES.txt (one name a line) and D.bin (S * S raw doubles) -> the
// table on stdout.  tests/test_samples_host.py compares it byte for byte with hostio.kr_table.
#include "host/rk_hostio.hpp"

#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::vector<std::string> names;
    {
        std::ifstream f(argv[1]);
        for (std::string line; std::getline(f, line);) names.push_back(line);
    }
    std::ifstream f(argv[2], std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string raw = ss.str();
    if (raw.size() != names.size() * names.size() * sizeof(double)) return 3;
    std::vector<double> D(names.size() * names.size());
    memcpy(D.data(), raw.data(), raw.size());
    std::cout << rkh::kr_table(names, D.data());
    return 0;
}
