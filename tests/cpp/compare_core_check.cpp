// compare_core_check.cpp -- the shared arithmetic of tamcmc_compare.h on the CPU, plain g++ (-std=c++17 -O1 -ffp-contract=off;
// `make compare-core-check CHECKFLAGS=-fsanitize=address,undefined` for a sanitizer build): the inclusion rule with NaN and
// +-inf, the pair totals on a case worked by hand, the pairing of replicates over one Philox call, the chunk and slot rules,
// the counting and rank rules, the softmax at equal and at hugely different z, and the EM step on identical fits (one
// iteration, gap 0, w = 1 / K exactly), on a dominated fit, at max_iter and once frozen.  Prints one line,
// "ok compare_core_check ...", or what failed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tamcmc_compare.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

// the stacking fit as the header states it, one unit after the other
static TmCmpStack em_run(const int K, const long long N, const std::vector<double> &elpd, const double s, const double tol, const long long max_iter,
                         std::vector<double> *f_trace = nullptr)
{
    TmCmpStack st;
    tmc_em_init(K, &st);
    long long Np = 0;
    for (long long i = 0; i < N; i++) Np += tmc_included(K, elpd.data(), N, i) ? 1 : 0;
    for (long long it = 0; it < max_iter + 5 && !st.frozen; it++) {
        double sum[TM_CMP_MAX_FITS] = {0.0}, sumlog = 0.0, P[TM_CMP_MAX_FITS];
        for (long long i = 0; i < N; i++) {
            if (!tmc_included(K, elpd.data(), N, i)) continue;
            tmc_P_unit(K, elpd.data(), N, i, s, P);
            const double den = tmc_den(K, st.w, P);
            for (int k = 0; k < K; k++) sum[k] += P[k] / den;
            sumlog += log(den);
        }
        tmc_em_step(K, Np, sum, sumlog, tol, max_iter, &st);
        if (f_trace) f_trace->push_back(st.f);
    }
    return st;
}

int main()
{
    const double inf = INFINITY, nan = std::nan("");

    // inclusion
    CHECK(tmc_finite(0.0) && tmc_finite(-1e308) && tmc_finite(5e-324) && !tmc_finite(nan) && !tmc_finite(inf) && !tmc_finite(-inf));
    {
        const double e[2 * 5] = {1.0, 2.0, nan, 4.0, 0.5, /**/ 0.5, 3.0, 1.0, 4.0, inf};
        const bool want[5] = {true, true, false, true, false};
        for (int i = 0; i < 5; i++) CHECK(tmc_included(2, e, 5, i) == want[i]);
        const double m[2 * 2] = {-inf, 1.0, 2.0, 3.0};
        CHECK(!tmc_included(2, m, 2, 0) && tmc_included(2, m, 2, 1));

        // pair totals by hand: the included units 0, 1, 3 have d = 0.5, -1, 0: sum -1/2, mean -1/6,
        // sum of squares 4/9 + 25/36 + 1/36 = 7/6, se = sqrt(3/2 * 7/6) = sqrt(7) / 2
        const double kh[2 * 5] = {0.8, nan, 5.0, 0.1, 0.9, /**/ 0.1, inf, 0.2, 0.7, 0.9};
        TmCmpTotals t = tmc_pair_totals(2, 5, e, kh, 0, 1);
        CHECK(t.n_included == 3 && t.n_excluded == 2 && t.n_better == 1 && t.n_worse == 1);
        CHECK(t.elpd_diff == -0.5 && std::fabs(t.se_diff - std::sqrt(7.0) / 2.0) < 1e-15);
        CHECK(t.n_k_high == 2 && t.diff_k_high == -0.5);               // unit 0 (0.8), unit 1 (+inf; the NaN is skipped); not unit 3 (0.7)
        TmCmpTotals u = tmc_pair_totals(2, 5, e, nullptr, 1, 0);
        CHECK(u.elpd_diff == 0.5 && u.se_diff == t.se_diff && u.n_better == 1 && u.n_worse == 1 && u.n_k_high == -1 && std::isnan(u.diff_k_high));
        TmCmpTotals same = tmc_pair_totals(2, 5, e, kh, 1, 1);
        CHECK(same.elpd_diff == 0.0 && same.se_diff == 0.0 && same.n_better == 0 && same.n_worse == 0);
        const double one[2] = {1.0, 3.0};
        TmCmpTotals o = tmc_pair_totals(2, 1, one, nullptr, 1, 0);
        CHECK(o.n_included == 1 && o.elpd_diff == 2.0 && std::isnan(o.se_diff));
        const double none[2] = {nan, 3.0};
        TmCmpTotals z = tmc_pair_totals(2, 1, none, one, 1, 0);
        CHECK(z.n_included == 0 && z.n_excluded == 1 && std::isnan(z.elpd_diff) && std::isnan(z.se_diff) && std::isnan(z.diff_k_high) && z.n_k_high == 0);
    }

    // the variate: replicates 2 m and 2 m + 1 share the call of replicate word m
    for (const uint64_t seed : {(uint64_t)12345, (uint64_t)0x9E3779B97F4A7C15ull})
        for (const uint64_t m : {(uint64_t)0, (uint64_t)7, ((uint64_t)1 << 32) - 1, (uint64_t)1 << 32})
            for (const uint32_t i : {0u, 1u, 2047u, 0x7FFFFFFEu}) {
                double ue, uo, e0, e1;
                tmn_uniforms(seed, m, i, 0u, &ue, &uo);
                tmc_variates2(seed, m, i, &e0, &e1);
                CHECK(e0 == -log(ue) && e1 == -log(uo) && e0 > 0.0 && e1 > 0.0 && e0 != e1);
                CHECK(tmc_variate(seed, 2 * m, i) == e0 && tmc_variate(seed, 2 * m + 1, i) == e1);
                CHECK(tmc_variate(seed, 2 * m + 2, i) != e0 && tmc_variate(seed, 2 * m + 2, i) != e1);
            }

    // chunks and slots
    CHECK(tmc_tiles(1) == 1 && tmc_tiles(TM_CMP_TILE) == 1 && tmc_tiles(TM_CMP_TILE + 1) == 2 && tmc_stack_tiles(TM_CMP_STACK_TILE + 1) == 2);
    for (const int K : {2, 3, 8})
        for (const long long tiles : {1LL, 3LL}) {
            const long long per = tiles * K * 8 + (K - 1) * 8;
            CHECK(tmc_chunk(1, tiles, K) == 1 && tmc_chunk(per, tiles, K) == 1 && tmc_chunk(2 * per, tiles, K) == 2 && tmc_chunk(3 * per + per - 1, tiles, K) == 3);
            CHECK(tmc_chunk(0, tiles, K) == std::min<long long>(TM_CMP_SCRATCH / per, TM_CMP_CHUNK_MAX));
        }
    CHECK(tmc_chunk(0, 1 << 20, 2) == 3 && tmc_chunk((long long)1 << 40, 1 << 20, 2) == 2 * TM_CMP_PAIRS * 4 - 2);       // 2^31 units: the launch's size
    CHECK(tmc_slots(0, 1) == 1 && tmc_slots(1, 1) == 1 && tmc_slots(0, 2) == 1 && tmc_slots(1, 2) == 2 && tmc_slots(3, 5) == 3 && tmc_slots(4, 5) == 3);
    for (long long c = 1; c < 40; c++)
        for (unsigned long long g0 = 0; g0 < 4; g0++) CHECK(tmc_slots(g0, c) <= tmc_slots_max(c));
    CHECK(tmc_z(4, 2.0, 3.0) == 6.0 && tmc_z(1000, 1.0, 0.0) == 0.0);

    // counting and ranks
    CHECK(tmc_rank(0.0, 7) == 0 && tmc_rank(1.0, 7) == 6 && tmc_rank(0.5, 4) == 1 && tmc_rank(0.51, 4) == 2 && tmc_rank(0.05, 4000) == 199 &&
          tmc_rank(0.95, 4000) == 3799 && tmc_rank(0.3, 1) == 0);
    {
        // K = 3, R = 5: z_1 = {1, -1, 0, 2, 2}, z_2 = {1, 3, 0, -2, 2}
        const double z[10] = {1.0, 1.0, -1.0, 3.0, 0.0, 0.0, 2.0, -2.0, 2.0, 2.0};
        long long gt, eq;
        tmc_prob(z, 3, 5, 1, 0, &gt, &eq); CHECK(gt == 3 && eq == 1);
        tmc_prob(z, 3, 5, 0, 1, &gt, &eq); CHECK(gt == 1 && eq == 1);
        tmc_prob(z, 3, 5, 1, 2, &gt, &eq); CHECK(gt == 1 && eq == 3);
        tmc_prob(z, 3, 5, 2, 2, &gt, &eq); CHECK(gt == 0 && eq == 5);
        // z_1 - z_2 = {0, -4, 0, 4, 0}: sorted -4 0 0 0 4
        CHECK(tmc_interval(z, 3, 5, 1, 2, 0.0) == -4.0 && tmc_interval(z, 3, 5, 1, 2, 0.2) == -4.0 && tmc_interval(z, 3, 5, 1, 2, 0.21) == 0.0 &&
              tmc_interval(z, 3, 5, 1, 2, 0.8) == 0.0 && tmc_interval(z, 3, 5, 1, 2, 0.81) == 4.0 && tmc_interval(z, 3, 5, 1, 2, 1.0) == 4.0);
        CHECK(tmc_interval(z, 3, 5, 2, 0, 0.5) == 1.0 && tmc_interval(z, 3, 5, 0, 2, 0.5) == -1.0);
    }

    // softmax
    for (int K = 2; K <= TM_CMP_MAX_FITS; K++) {
        double x[TM_CMP_MAX_FITS], w[TM_CMP_MAX_FITS];
        for (int k = 0; k < K; k++) x[k] = -1234.5;
        tmc_softmax(K, x, w);
        for (int k = 0; k < K; k++) CHECK(w[k] == 1.0 / (double)K);
    }
    {
        double x[3] = {0.0, 1e6, -1e300}, w[3];
        tmc_softmax(3, x, w);
        CHECK(w[0] == 0.0 && w[1] == 1.0 && w[2] == 0.0);
        double y[2] = {0.0, std::log(3.0)}, v[2];
        tmc_softmax(2, y, v);
        CHECK(std::fabs(v[0] - 0.25) < 1e-15 && std::fabs(v[1] - 0.75) < 1e-15);
        // pseudo-BMA+: two replicates, z_1 = +-1e6: each fit wins once
        const double z[2] = {1e6, -1e6};
        double b[2];
        tmc_bma_plus(z, 2, 2, 1.0, b);
        CHECK(b[0] == 0.5 && b[1] == 0.5);
        tmc_bma_plus(z, 2, 1, 0.5, b);
        CHECK(b[0] == 0.0 && b[1] == 1.0);
    }

    // EM on identical fits: one iteration, gap 0, w = 1 / K exactly (K with an exact sum of the K products w_k P_k)
    for (const int K : {2, 3, 4, 8}) {
        const long long N = 777;
        std::vector<double> elpd((size_t)K * N);
        for (int k = 0; k < K; k++)
            for (long long i = 0; i < N; i++) elpd[(size_t)k * N + i] = -3.0 - 0.01 * (double)i;
        elpd[5] = nan;                                                   // an excluded unit enters nothing
        const TmCmpStack st = em_run(K, N, elpd, 1.0, 0.0, 100);
        CHECK(st.iterations == 1 && st.converged == 1 && st.frozen == 1 && st.gap == 0.0 && st.f == 0.0);
        for (int k = 0; k < K; k++) CHECK(st.w[k] == 1.0 / (double)K && st.g[k] == 1.0);
    }
    // EM on a dominated fit: fit 1 is 0.01 worse in every unit
    {
        const long long N = 300;
        std::vector<double> elpd(2 * N);
        for (long long i = 0; i < N; i++) { elpd[i] = -2.0 + 0.5 * std::sin((double)i); elpd[N + i] = elpd[i] - 0.01; }
        std::vector<double> f;
        const TmCmpStack st = em_run(2, N, elpd, 1.0, 1e-9, 100000, &f);
        CHECK(st.converged == 1 && st.gap <= 1e-9 && st.gap >= 0.0 && st.w[1] < 1e-6 && st.w[1] > 0.0 && std::fabs(st.w[0] + st.w[1] - 1.0) < 1e-12);
        CHECK(st.iterations > 1000 && st.iterations < 3000 && (long long)f.size() == st.iterations && f.back() <= 0.0 && f.back() > -1e-8);
        for (size_t i = 1; i < f.size(); i++) CHECK(f[i] >= f[i - 1] - 1e-15);       // EM never lowers the objective
        // max_iter: not converged, the state after max_iter - 1 updates, its own gap; a frozen state stays
        TmCmpStack three = em_run(2, N, elpd, 1.0, 1e-9, 3);
        const TmCmpStack nine = em_run(2, N, elpd, 1.0, 1e-9, 9);
        CHECK(three.iterations == 3 && three.converged == 0 && three.frozen == 1 && three.gap > 1e-9 && nine.iterations == 9 && nine.w[1] < three.w[1]);
        const double c = std::exp(-0.01), a1 = 0.5 * c / (0.5 + 0.5 * c), a0 = 0.5 / (0.5 + 0.5 * c), w2 = a1 * c / (a0 + a1 * c);
        CHECK(std::fabs(three.w[1] / w2 - 1.0) < 1e-12 && std::fabs(three.gap - (1.0 / (three.w[0] + three.w[1] * c) - 1.0)) < 1e-12);
        const TmCmpStack before = three;
        const double sum[2] = {5.0, 7.0};
        tmc_em_step(2, N, sum, -1.0, 1e-9, 100, &three);
        CHECK(three.iterations == before.iterations && three.w[0] == before.w[0] && three.w[1] == before.w[1] && three.gap == before.gap && three.f == before.f);
    }

    if (failures) return 1;
    std::printf("ok compare_core_check: inclusion, pair totals, replicate pairing, chunks, counting, softmax, EM\n");
    return 0;
}
