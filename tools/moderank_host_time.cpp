// moderank_host_time.cpp -- what the mode table's rank-normalised diagnostics cost on one host thread: per column the sorted
// keys (std::sort) of the values and of the folded values, rank2 of every sample by the two binary searches, z, the tail
// indicators and the Welford means -- the serial statements of tamcmc-c-_amd/csrc/tamcmc_moderank.h -- and then the lag
// products of the four series (tmd_lag_serial) and their finish, on a synthetic column-major table.
// tools/summary_time.py --modes-rank builds this with g++ -O2 -ffp-contract=off and quotes its times beside the kernels'.
// Not the code under test.
//   moderank_host_time <n> <n_cols> <L>     prints one JSON line
#include "tamcmc_moderank.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: moderank_host_time <n> <n_cols> <L>\n"); return 1; }
    const long long n = std::atoll(argv[1]);
    const int n_cols = std::atoi(argv[2]), L = std::atoi(argv[3]);
    if (n < 4 || n_cols < 1 || L < 1 || L > TM_MD_MAX_LAG || L > n - 1) return 1;
    const size_t sn = (size_t)n;
    std::vector<double> table((size_t)n_cols * sn);
    std::mt19937_64 g(1u);
    std::normal_distribution<double> N(0.0, 1.0);
    for (int c = 0; c < n_cols; c++) {
        double v = N(g);
        for (size_t t = 0; t < sn; t++) { table[(size_t)c * sn + t] = 100.0 + v; v = 0.8 * v + N(g); }
    }
    using clk = std::chrono::steady_clock;
    std::vector<uint64_t> sv(sn), sf(sn);
    std::vector<double> series(TM_MR_NSERIES * sn), A((size_t)L + 1);
    double sink = 0.0, sort_ms = 0.0, transform_ms = 0.0, lag_ms = 0.0;
    const long long r05 = (long long)tmq_rank(0.05, n), r95 = (long long)tmq_rank(0.95, n);
    const double tau_floor = 1.0 / std::log10((double)n);
    for (int c = 0; c < n_cols; c++) {
        const double *v = table.data() + (size_t)c * sn;
        const auto t0 = clk::now();
        for (size_t t = 0; t < sn; t++) sv[t] = tmq_key(v[t]);
        std::sort(sv.begin(), sv.end());
        const double med = tmr_median(sv.data(), n), Q05 = tmq_unkey(sv[(size_t)r05]), Q95 = tmq_unkey(sv[(size_t)r95]);
        for (size_t t = 0; t < sn; t++) sf[t] = tmq_key(tmr_fold(v[t], med));
        std::sort(sf.begin(), sf.end());
        const auto t1 = clk::now();
        double mean[TM_MR_NSERIES] = {}, M2[TM_MR_NSERIES] = {};
        for (size_t t = 0; t < sn; t++) {
            series[TM_MR_Z * sn + t] = tmr_z(tmr_rank2(sv.data(), n, tmq_key(v[t])), n);
            series[TM_MR_ZFOLD * sn + t] = tmr_z(tmr_rank2(sf.data(), n, tmq_key(tmr_fold(v[t], med))), n);
            series[TM_MR_I05 * sn + t] = tmr_indicator(v[t], Q05);
            series[TM_MR_I95 * sn + t] = tmr_indicator(v[t], Q95);
        }
        for (int s = 0; s < TM_MR_NSERIES; s++)
            for (size_t t = 0; t < sn; t++) tme_welford(&mean[s], &M2[s], (long long)t + 1, series[(size_t)s * sn + t]);
        const auto t2 = clk::now();
        for (int s = 0; s < TM_MR_NSERIES; s++) {
            tmd_lag_serial(series.data() + (size_t)s * sn, n, mean[s], L, A.data(), 1);
            sink += tme_finish(A.data(), 1, L, (double)n, tau_floor).ess;
        }
        const auto t3 = clk::now();
        sort_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
        transform_ms += std::chrono::duration<double, std::milli>(t2 - t1).count();
        lag_ms += std::chrono::duration<double, std::milli>(t3 - t2).count();
    }
    std::printf("{\"host_sort_ms\": %.3f, \"host_transform_ms\": %.3f, \"host_lag_ms\": %.3f, \"host_sink\": %.6g}\n", sort_ms, transform_ms, lag_ms, sink);
    return 0;
}
