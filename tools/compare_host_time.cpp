// compare_host_time.cpp -- the serial statements of tamcmc_compare.h on one host thread, for the timing table of the comparison
// of fits (tools/summary_time.py --compare K,R builds and runs it): the Bayesian bootstrap's variates and sums of `replicates`
// replicates over N units and K fits, two replicates per Philox call as on the device, and `iterations` iterations of the
// stacking fit with the table of P formed once.  The inputs are a fixed pseudo-random case; nothing is checked here.
//
//   compare_host_time N K replicates iterations   ->   one JSON line: host_bootstrap_ms_per_replicate, host_stack_prepare_ms,
//                                                      host_stack_ms_per_iteration
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tamcmc_compare.h"

static double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char **argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: compare_host_time N K replicates iterations\n"); return 2; }
    const long long N = std::atoll(argv[1]);
    const int K = std::atoi(argv[2]);
    const long long R = std::atoll(argv[3]), iters = std::atoll(argv[4]);
    if (N < 1 || K < 2 || K > TM_CMP_MAX_FITS || R < 2 || iters < 1) return 2;
    std::vector<double> elpd((size_t)K * (size_t)N);
    uint64_t s = 88172645463325252ull;
    for (double &v : elpd) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; v = -3.0 + (double)(s >> 11) * 0x1p-53; }

    // bootstrap: D once, then per pair of replicates one Philox call and two logarithms per unit
    std::vector<double> D((size_t)(K - 1) * (size_t)N);
    for (int k = 1; k < K; k++)
        for (long long i = 0; i < N; i++) D[(size_t)(k - 1) * N + i] = elpd[(size_t)k * N + i] - elpd[i];
    double sink = 0.0;
    const double t0 = now_ms();
    for (long long pair = 0; pair < (R + 1) / 2; pair++) {
        double A[2] = {0.0, 0.0}, B[2][TM_CMP_MAX_FITS] = {{0.0}};
        for (long long i = 0; i < N; i++) {
            double e[2];
            tmc_variates2(12345, (uint64_t)pair, (uint32_t)i, &e[0], &e[1]);
            for (int h = 0; h < 2; h++) {
                A[h] += e[h];
                for (int k = 1; k < K; k++) B[h][k] += e[h] * D[(size_t)(k - 1) * N + i];
            }
        }
        for (int h = 0; h < 2; h++)
            for (int k = 1; k < K; k++) sink += tmc_z(N, A[h], B[h][k]);
    }
    const double boot_ms = (now_ms() - t0) / (double)(2 * ((R + 1) / 2));

    // stacking: the table of P, then the iterations
    const double t1 = now_ms();
    std::vector<double> P((size_t)K * (size_t)N);
    for (long long i = 0; i < N; i++) {
        double p[TM_CMP_MAX_FITS];
        tmc_P_unit(K, elpd.data(), N, i, 1.0, p);
        for (int k = 0; k < K; k++) P[(size_t)k * N + i] = p[k];
    }
    const double prep_ms = now_ms() - t1;
    TmCmpStack st;
    tmc_em_init(K, &st);
    const double t2 = now_ms();
    for (long long it = 0; it < iters; it++) {
        double sum[TM_CMP_MAX_FITS] = {0.0}, sumlog = 0.0, p[TM_CMP_MAX_FITS];
        for (long long i = 0; i < N; i++) {
            for (int k = 0; k < K; k++) p[k] = P[(size_t)k * N + i];
            const double den = tmc_den(K, st.w, p);
            for (int k = 0; k < K; k++) sum[k] += p[k] / den;
            sumlog += log(den);
        }
        tmc_em_step(K, N, sum, sumlog, 0.0, iters + 1, &st);
    }
    const double iter_ms = (now_ms() - t2) / (double)iters;
    std::printf("{\"N\": %lld, \"K\": %d, \"host_bootstrap_ms_per_replicate\": %.6g, \"host_stack_prepare_ms\": %.6g, \"host_stack_ms_per_iteration\": %.6g, "
                "\"sink\": %.3g}\n", N, K, boot_ms, prep_ms, iter_ms, sink + st.gap);
    return 0;
}
