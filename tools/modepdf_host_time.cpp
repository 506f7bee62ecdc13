// modepdf_host_time.cpp -- what the mode table's histograms, shortest intervals and pair densities cost on one host thread:
// the plain statements of tamcmc-c-_amd/csrc/tamcmc_modepdf.h (tmp_host_hist, std::sort and tmp_host_hpd, tmp_host_hist2d
// and tmp_level) on a synthetic column-major table, every column over its own min ... max.
// tools/summary_time.py --modes-pdf builds this with g++ -O2 -ffp-contract=off and quotes its times beside the kernels'.
// Not the code under test.
//   modepdf_host_time <n> <n_cols> <n_pairs>     prints one JSON line
#include "tamcmc_modepdf.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: modepdf_host_time <n> <n_cols> <n_pairs>\n"); return 1; }
    const long long n = std::atoll(argv[1]);
    const int n_cols = std::atoi(argv[2]), n_pairs = std::atoi(argv[3]);
    if (n < 4 || n_cols < 2 || n_pairs < 1) return 1;
    const size_t sn = (size_t)n;
    std::vector<double> table((size_t)n_cols * sn), mn((size_t)n_cols), mx((size_t)n_cols);
    std::mt19937_64 g(1u);
    std::normal_distribution<double> N(0.0, 1.0);
    for (int c = 0; c < n_cols; c++) {
        double v = N(g);
        for (size_t t = 0; t < sn; t++) { table[(size_t)c * sn + t] = 100.0 + v; v = 0.8 * v + N(g); }
        mn[(size_t)c] = *std::min_element(table.begin() + (size_t)c * sn, table.begin() + ((size_t)c + 1) * sn);
        mx[(size_t)c] = *std::max_element(table.begin() + (size_t)c * sn, table.begin() + ((size_t)c + 1) * sn);
    }
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    double sink = 0.0;
    const int bins = 50, bins2 = 32;
    std::vector<int64_t> cnt((size_t)bins), cells((size_t)bins2 * bins2);
    int64_t below, above, outside, start;
    const auto t0 = clk::now();
    for (int c = 0; c < n_cols; c++) {
        tmp_host_hist(table.data() + (size_t)c * sn, n, mn[(size_t)c], mx[(size_t)c], bins, cnt.data(), &below, &above);
        sink += (double)cnt[bins / 2];
    }
    const auto t1 = clk::now();
    double sort_ms = 0.0;
    const long long k68 = tmp_window(0.68, n), k95 = tmp_window(0.95, n);
    for (int c = 0; c < n_cols; c++) {
        const auto s0 = clk::now();
        const std::vector<uint64_t> keys = tmp_host_sorted(table.data() + (size_t)c * sn, n);
        sort_ms += ms(s0, clk::now());
        double lo, hi;
        tmp_host_hpd(keys.data(), n, k68, &start, &lo, &hi);
        sink += hi - lo;
        tmp_host_hpd(keys.data(), n, k95, &start, &lo, &hi);
        sink += hi - lo;
    }
    const auto t2 = clk::now();
    for (int p = 0; p < n_pairs; p++) {
        const int a = (2 * p) % n_cols, b = (2 * p + 1) % n_cols;
        tmp_host_hist2d(table.data() + (size_t)a * sn, table.data() + (size_t)b * sn, n, mn[(size_t)a], mx[(size_t)a], mn[(size_t)b], mx[(size_t)b], bins2,
                        cells.data(), &outside);
        const std::vector<int64_t> desc = tmp_sorted_counts(cells.data(), cells.size());
        sink += (double)tmp_level(desc, n - outside, 0.68) + (double)tmp_level(desc, n - outside, 0.95);
    }
    const auto t3 = clk::now();
    std::printf("{\"host_hist_ms\": %.3f, \"host_hpd_ms\": %.3f, \"host_hpd_sort_ms\": %.3f, \"host_hist2d_ms\": %.3f, \"host_sink\": %.6g}\n", ms(t0, t1), ms(t1, t2),
                sort_ms, ms(t2, t3), sink);
    return 0;
}
