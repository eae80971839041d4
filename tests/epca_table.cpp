// rkh::epca_table (rappas_amd/csrc/host/rk_hostio.hpp) on its own: NAMES.txt (one name a line), B, K, ITERS, N_ACTIVE, K_EFF and
// VALUES.bin (raw doubles: eigenvalue[k] | share[k] | residual[k] | projection[S][k] | loading[B][k]) -> the table on stdout.
// tests/test_epca_host.py compares it byte for byte with hostio.epca_table.
#include "host/rk_hostio.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

int main(int argc, char **argv) {
    if (argc != 8) return 2;
    std::vector<std::string> names;
    {
        std::ifstream f(argv[1]);
        for (std::string line; std::getline(f, line);) names.push_back(line);
    }
    const uint32_t B = (uint32_t)strtoul(argv[2], nullptr, 10), k = (uint32_t)strtoul(argv[3], nullptr, 10), iters = (uint32_t)strtoul(argv[4], nullptr, 10);
    const uint32_t n_active = (uint32_t)strtoul(argv[5], nullptr, 10), k_eff = (uint32_t)strtoul(argv[6], nullptr, 10);
    std::ifstream f(argv[7], std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string raw = ss.str();
    const size_t S = names.size(), n = (size_t)k * (3 + S + B);
    if (raw.size() != n * sizeof(double)) return 3;
    std::vector<double> v(n);
    if (n) memcpy(v.data(), raw.data(), raw.size());
    std::cout << rkh::epca_table(names, B, k, iters, n_active, k_eff, v.data(), v.data() + k, v.data() + 2 * k, v.data() + 3 * k, v.data() + 3 * k + S * k);
    return 0;
}
