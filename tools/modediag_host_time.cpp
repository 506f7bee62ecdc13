// modediag_host_time.cpp -- what the mode table's diagnostics cost on one host thread: the lag products of every column
// (tmd_lag_serial) and the sums of products of every pair of the upper triangle (tmd_cov_serial), the serial statements of
// tamcmc-c-_amd/csrc/tamcmc_modediag.h, on a synthetic column-major table.  tools/summary_time.py --modes-ess / --modes-cov
// builds this with g++ -O2 -ffp-contract=off and quotes its times beside the kernels'.  Not the code under test.
//   modediag_host_time <n> <n_cols> <L> <n_sel>     prints one JSON line
#include "tamcmc_modediag.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: modediag_host_time <n> <n_cols> <L> <n_sel>\n"); return 1; }
    const long long n = std::atoll(argv[1]);
    const int n_cols = std::atoi(argv[2]), L = std::atoi(argv[3]), n_sel = std::atoi(argv[4]);
    if (n < 2 || n_cols < 1 || L < 0 || L > TM_MD_MAX_LAG || L > n - 1 || n_sel < 0 || n_sel > n_cols) return 1;
    std::vector<double> table((size_t)n_cols * (size_t)n), mean((size_t)n_cols);
    std::mt19937_64 g(1u);
    std::normal_distribution<double> N(0.0, 1.0);
    for (int c = 0; c < n_cols; c++) {
        double v = N(g), m = 0.0, q = 0.0;
        for (long long t = 0; t < n; t++) {
            table[(size_t)c * (size_t)n + (size_t)t] = 100.0 + v;
            tme_welford(&m, &q, t + 1, 100.0 + v);
            v = 0.8 * v + N(g);
        }
        mean[(size_t)c] = m;
    }
    using clk = std::chrono::steady_clock;
    std::vector<double> A((size_t)L + 1);
    double sink = 0.0;
    const auto t0 = clk::now();
    for (int c = 0; c < n_cols; c++) {
        tmd_lag_serial(table.data() + (size_t)c * (size_t)n, n, mean[(size_t)c], L, A.data(), 1);
        sink += A[(size_t)L];
    }
    const auto t1 = clk::now();
    for (int i = 0; i < n_sel; i++)
        for (int j = i; j < n_sel; j++)
            sink += tmd_cov_serial(table.data() + (size_t)i * (size_t)n, mean[(size_t)i], table.data() + (size_t)j * (size_t)n, mean[(size_t)j], n);
    const auto t2 = clk::now();
    std::printf("{\"host_lag_ms\": %.3f, \"host_cov_ms\": %.3f, \"host_sink\": %.6g}\n", std::chrono::duration<double, std::milli>(t1 - t0).count(),
                std::chrono::duration<double, std::milli>(t2 - t1).count(), sink);
    return 0;
}
