// modediag_core_check.cpp -- the arithmetic of tamcmc_modediag.h on the CPU (plain g++, no GPU, no library):
//   * the lag kernel's walk -- tiles of TM_MD_TILE samples behind a halo, lag blocks, lanes of TM_MD_G lags, the four-at-a-time
//     and the guarded path of tmd_lag_tile -- fed tile by tile on the host, against the plain serial loops, bit for bit:
//     n on either side of every tile edge up to 3 TM_MD_TILE + 1, L in {1, 3, 15, 17, 255, 1023} and L = n - 1, series
//     holding +-inf and NaN (no 0 x inf from the samples before the lag);
//   * the covariance kernel's walk -- strips of TM_MD_CT columns, stages of TM_MD_CS samples, the strip pairs of the upper
//     triangle -- against the plain serial loop, bit for bit, with a column stride larger than n and permuted subsets; the
//     matrix is symmetric and its diagonal is lag product 0;
//   * the strip-pair map, the correlation finish on hand cases (zero variance, +-inf, NaN, the clamp) and the totals.
// Prints "ok modediag_core_check ..." and exits 0, or says what failed and exits 1.  May be built with
// -fsanitize=address,undefined and run as it is.
#define TMD_HOST_FEED
#include "tamcmc_modediag.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <utility>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static bool same_bits(const double a, const double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (std::isnan(a) && std::isnan(b)); }

static std::vector<double> ar1(const double phi, const long long n, const unsigned seed, const double offset)
{
    std::mt19937_64 g(seed);
    std::normal_distribution<double> N(0.0, 1.0);
    std::vector<double> x((size_t)n);
    double v = N(g);
    for (long long t = 0; t < n; t++) { x[(size_t)t] = v + offset; v = phi * v + N(g); }
    return x;
}

static double welford_mean(const std::vector<double> &x)
{
    double m = 0.0, q = 0.0;
    for (size_t t = 0; t < x.size(); t++) tme_welford(&m, &q, (long long)t + 1, x[t]);
    return m;
}

static long check_lags(const std::vector<double> &x, const double mean, const int L, const char *tag)
{
    const long long n = (long long)x.size();
    std::vector<double> got((size_t)L + 1, -1.0), want((size_t)L + 1, -2.0);
    tmd_host_lag_column(x.data(), n, mean, L, got.data());
    tmd_lag_serial(x.data(), n, mean, L, want.data(), 1);
    for (int k = 0; k <= L; k++)
        CHECK(same_bits(got[(size_t)k], want[(size_t)k]), "%s n %lld L %d lag %d: walk %a, serial %a", tag, n, L, k, got[(size_t)k], want[(size_t)k]);
    return L + 1;
}

int main()
{
    static_assert(TM_MD_TILE % TM_MD_G == 0 && TM_MD_TILE % TM_MD_LANES == 0 && TM_MD_HALO % TM_MD_G == 0, "tile geometry");
    static_assert(TM_MD_HALO > TM_MD_MAX_LAG && TM_MD_TILE >= TM_MD_HALO && TM_MD_HALO % TM_MD_LANES == 0, "halo geometry");
    static_assert((TM_MD_HALO + TM_MD_TILE) * sizeof(double) <= 64 * 1024, "lag kernel LDS");
    static_assert(2 * TM_MD_CS * TM_MD_CROW * sizeof(double) <= 64 * 1024 && TM_MD_CROW % 2 == 0 && TM_MD_CT % 2 == 0, "cov kernel LDS");
    static_assert(TM_MD_CTHREADS == (TM_MD_CT / 2) * (TM_MD_CT / 2) && TM_MD_CS == 64, "cov kernel threads");
    long lags = 0, pairs = 0;
    const int T = TM_MD_TILE;
    // ---- the lag walk against the serial loops ----
    std::vector<long long> ns = {1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1022};
    for (int e = 1; e <= 3; e++) for (int d = -1; d <= 1; d++) ns.push_back((long long)e * T + d);
    for (const long long n : ns) {
        const std::vector<double> x = ar1(0.8, n, 11u + (unsigned)n, 3000.0);
        const double mean = welford_mean(x);
        std::set<int> Ls;
        for (const int Lreq : {1, 3, 15, 17, 255, 1023}) if (tme_lag_limit(Lreq, n) >= 1) Ls.insert(tme_lag_limit(Lreq, n));
        if (n - 1 >= 1 && n - 1 <= TM_MD_MAX_LAG) Ls.insert((int)(n - 1));     // (odd or even: the walk takes either)
        for (const int L : Ls) lags += check_lags(x, mean, L, "ar1");
    }
    CHECK(tmd_lag_blocks(1) == 1 && tmd_lag_blocks(255) == 1 && tmd_lag_blocks(256) == 2 && tmd_lag_blocks(1023) == 4, "lag blocks");
    CHECK(tmd_tile_len(5, 0) == 5 && tmd_tile_len(T, 0) == T && tmd_tile_len(T + 1, T) == 1 && tmd_tile_len(3LL * T, T) == T, "tile length");
    {   // a constant column centres to exact zeros: every lag product is +0 and the finish says NaN, cut 0
        const std::vector<double> x((size_t)(T + 7), 1234.5678);
        const double mean = welford_mean(x);
        CHECK(same_bits(mean, 1234.5678), "Welford's mean of equal values is %a", mean);
        std::vector<double> A(256);
        tmd_host_lag_column(x.data(), (long long)x.size(), mean, 255, A.data());
        for (int k = 0; k <= 255; k++) CHECK(same_bits(A[(size_t)k], 0.0), "constant column: lag %d is %a", k, A[(size_t)k]);
        const TmeFinish f = tme_finish(A.data(), 1, 255, (double)x.size(), 1.0 / std::log10((double)x.size()));
        CHECK(std::isnan(f.tau) && std::isnan(f.ess) && f.cut == 0, "constant column: tau %g ess %g cut %d", f.tau, f.ess, f.cut);
    }
    for (const double bad : {(double)INFINITY, -(double)INFINITY, (double)NAN})
        for (const long long where : {0LL, 1LL, 1023LL, 1024LL, 1300LL}) {
            std::vector<double> x = ar1(0.5, T + 300, 3u, 0.0);
            x[(size_t)where] = bad;
            for (const int L : {17, 1023}) {
                lags += check_lags(x, 0.25, L, "bad value");
                std::vector<double> A((size_t)L + 1);
                tmd_host_lag_column(x.data(), (long long)x.size(), 0.25, L, A.data());
                for (int k = 0; k <= L; k++) {
                    const bool meets = where >= k || where + k < (long long)x.size();
                    CHECK(meets || std::isfinite(A[(size_t)k]), "bad value at %lld lag %d: not finite without meeting it", where, k);
                }
            }
        }
    // ---- the strip-pair map ----
    for (const int n_sel : {1, 31, 32, 33, 64, 65, 277, 1024}) {
        const int nt = tmd_cov_strips(n_sel);
        std::set<std::pair<int, int>> seen;
        for (int b = 0; b < tmd_cov_blocks(n_sel); b++) {
            int bi = -1, bj = -1;
            tmd_tile_pair(b, nt, &bi, &bj);
            CHECK(0 <= bi && bi <= bj && bj < nt && seen.insert({bi, bj}).second, "strip pair %d of %d: (%d, %d)", b, nt, bi, bj);
        }
        CHECK((int)seen.size() == nt * (nt + 1) / 2, "strip pairs of %d columns", n_sel);
    }
    // ---- the covariance walk against the serial loop ----
    {
        const int n_cols = 70;
        std::mt19937_64 g(99u);
        for (const long long n : {1LL, 2LL, 5LL, 63LL, 64LL, 65LL, 127LL, 128LL, 129LL, 191LL, 192LL, 193LL, 1000LL}) {
            const size_t stride = (size_t)n + 37;
            std::vector<double> table((size_t)n_cols * stride, 1e300), mean((size_t)n_cols);
            for (int c = 0; c < n_cols; c++) {
                std::vector<double> x = ar1(0.1 * (c % 9), n, 5u + (unsigned)c, 100.0 * c);
                if (c == 3) x.assign((size_t)n, 42.0);                           // a constant column
                if (c > 0 && c % 7 == 0) for (long long t = 0; t < n; t++) x[(size_t)t] += 0.5 * table[(size_t)(c - 1) * stride + (size_t)t];
                for (long long t = 0; t < n; t++) table[(size_t)c * stride + (size_t)t] = x[(size_t)t];
                mean[(size_t)c] = welford_mean(x);
            }
            for (const int n_sel : {1, 2, 31, 32, 33, 64, 65, 70}) {
                std::vector<int32_t> sel((size_t)n_cols);
                for (int c = 0; c < n_cols; c++) sel[(size_t)c] = c;
                if (n_sel != 70) std::shuffle(sel.begin(), sel.end(), g);
                std::vector<double> S((size_t)n_sel * n_sel, -7.0);
                tmd_host_cov(table.data(), stride, n, mean.data(), sel.data(), n_sel, S.data());
                for (int i = 0; i < n_sel; i++)
                    for (int j = 0; j < n_sel; j++) {
                        const int ci = sel[(size_t)i], cj = sel[(size_t)j];
                        const double want = tmd_cov_serial(table.data() + (size_t)ci * stride, mean[(size_t)ci], table.data() + (size_t)cj * stride, mean[(size_t)cj], n);
                        CHECK(same_bits(S[(size_t)i * n_sel + j], want), "cov n %lld n_sel %d (%d, %d): walk %a, serial %a", n, n_sel, i, j, S[(size_t)i * n_sel + j], want);
                        CHECK(same_bits(S[(size_t)i * n_sel + j], S[(size_t)j * n_sel + i]), "cov n %lld n_sel %d (%d, %d): not symmetric", n, n_sel, i, j);
                        pairs++;
                    }
                for (int i = 0; i < n_sel; i++) {
                    double A0 = -1.0;
                    tmd_lag_serial(table.data() + (size_t)sel[(size_t)i] * stride, n, mean[(size_t)sel[(size_t)i]], 0, &A0, 1);
                    CHECK(same_bits(S[(size_t)i * n_sel + i], A0), "cov n %lld n_sel %d: S_%d%d %a is not A_0 %a", n, n_sel, i, i, S[(size_t)i * n_sel + i], A0);
                    if (sel[(size_t)i] == 3) CHECK(same_bits(A0, 0.0), "the constant column's A_0 is %a", A0);
                }
            }
        }
    }
    // ---- the correlation finish ----
    CHECK(tmd_corr(2.0, 4.0, 1.0, false) == 1.0 && tmd_corr(-1.0, 4.0, 1.0, false) == -0.5 && tmd_corr(0.0, 4.0, 1.0, false) == 0.0, "corr values");
    CHECK(tmd_corr(4.0, 4.0, 4.0, true) == 1.0 && tmd_corr(3.9999999, 4.0, 4.0, true) == 1.0, "corr diagonal");
    CHECK(tmd_corr(2.0000001, 4.0, 1.0, false) == 1.0 && tmd_corr(-2.0000001, 4.0, 1.0, false) == -1.0, "corr clamp");
    CHECK(std::isnan(tmd_corr(0.0, 0.0, 1.0, false)) && std::isnan(tmd_corr(0.0, 1.0, 0.0, false)) && std::isnan(tmd_corr(0.0, 0.0, 0.0, true)), "corr zero variance");
    CHECK(std::isnan(tmd_corr(1.0, (double)INFINITY, 1.0, false)) && std::isnan(tmd_corr(1.0, 1.0, (double)INFINITY, false)) &&
          std::isnan(tmd_corr((double)INFINITY, (double)INFINITY, (double)INFINITY, true)), "corr infinite variance");
    CHECK(std::isnan(tmd_corr(1.0, (double)NAN, 1.0, false)) && std::isnan(tmd_corr(1.0, -1.0, 1.0, false)) && std::isnan(tmd_corr((double)NAN, 1.0, 1.0, false)), "corr NaN");
    CHECK(std::isnan(tmd_corr((double)INFINITY, 1.0, 1.0, false)) == false && tmd_corr((double)INFINITY, 1.0, 1.0, false) == 1.0, "corr of an infinite covariance clamps");
    // ---- the totals ----
    {
        const double nan = (double)NAN;
        const double ess[6] = {nan, 50.0, 20.0, 20.0, nan, 70.0}, rhat[6] = {nan, 1.005, 1.2, 1.0100000000000002, 1.2, 1.01};
        const int32_t cut[6] = {0, 16, 4, 16, 0, 2};
        const double A0[6] = {0.0, 1.0, 2.0, 3.0, -0.0, (double)INFINITY};
        const TmdTotals t = tmd_totals(6, 1000, 15, ess, rhat, cut, A0);
        CHECK(t.n_used == 1000 && t.lag == 15 && t.min_ess == 20.0 && t.col_min_ess == 2 && t.max_rhat == 1.2 && t.col_max_rhat == 2, "totals: extremes");
        CHECK(t.n_truncated == 2 && t.n_constant == 2 && t.n_rhat_high == 3, "totals: counts %lld %lld %lld", (long long)t.n_truncated, (long long)t.n_constant, (long long)t.n_rhat_high);
        const double all_nan[2] = {nan, nan};
        const int32_t c0[2] = {0, 0};
        const double z[2] = {0.0, 0.0};
        const TmdTotals u = tmd_totals(2, 10, 3, all_nan, all_nan, c0, z);
        CHECK(std::isnan(u.min_ess) && u.col_min_ess == -1 && std::isnan(u.max_rhat) && u.col_max_rhat == -1 && u.n_constant == 2 && u.n_rhat_high == 0, "totals: all NaN");
    }
    CHECK(tmd_acc_bytes(255, 277) == (size_t)(8 * (255 + 4) * 277 + 4 * 277) && tmd_cov_bytes(129) == (size_t)(8 * 129 * 129 + 4 * 129), "byte counts");
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok modediag_core_check: %ld lag products and %ld column pairs equal the serial loops bit for bit; strip pairs, correlation finish, totals\n", lags, pairs);
    return 0;
}
