// ess_core_check.cpp -- the arithmetic of tamcmc_ess.h on the CPU (plain g++, no GPU, no library):
//   * the lag products through the chunked ring-and-carry path of the device code against a brute-force long-double
//     autocovariance, on AR(1) series (phi = -0.5, 0, 0.8, 0.99), constant series and series holding +-inf and NaN;
//   * the same bits whether a series is fed in pieces of 1, L - 1, L, L + 1, TM_ESS_G +- 1, or all at once;
//   * the finish against a second, array-based statement of Geyer's initial monotone sequence, and its edge cases;
//   * the lag limit and the split R-hat formula.
// Prints "ok ess_core_check ..." and exits 0, or says what failed and exits 1.  May be built with
// -fsanitize=address,undefined and run as it is.
#define TME_HOST_FEED
#include "tamcmc_ess.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static bool same_bits(const double a, const double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static std::vector<double> ar1(const double phi, const int n, const unsigned seed, const double offset)
{
    std::mt19937_64 g(seed);
    std::normal_distribution<double> N(0.0, 1.0);
    std::vector<double> x((size_t)n);
    double v = N(g) / std::sqrt(1.0 - phi * phi);
    for (int t = 0; t < n; t++) { x[(size_t)t] = v + offset; v = phi * v + N(g); }
    return x;
}

static std::vector<double> feed(const std::vector<double> &d, const int L, const long long piece)
{
    TmeHostSeries s(L);
    const long long n = (long long)d.size();
    for (long long k = 0; k < n; k += piece) s.push(d.data() + k, n - k < piece ? n - k : piece);
    return s.acc;
}

// array-based Geyer: every rho, every P, then the rule
static TmeFinish finish_plain(const std::vector<double> &A, const int L, const double dn, const double floor_)
{
    TmeFinish f;
    if (A[0] == 0.0 || !std::isfinite(A[0])) { f.tau = f.ess = NAN; f.cut = 0; return f; }
    std::vector<double> rho((size_t)L + 1), P((size_t)(L + 1) / 2);
    for (int k = 0; k <= L; k++) rho[(size_t)k] = A[(size_t)k] / A[0];
    for (size_t m = 0; m < P.size(); m++) P[m] = rho[2 * m] + rho[2 * m + 1];
    size_t K = P.size();
    for (size_t m = 0; m < P.size(); m++) if (!(P[m] >= 0.0)) { K = m; break; }
    for (size_t m = 1; m < K; m++) P[m] = P[m] < P[m - 1] ? P[m] : P[m - 1];
    double sum = 0.0;
    for (size_t m = 0; m < K; m++) sum += P[m];
    double tau = -1.0 + 2.0 * sum;
    tau = tau < floor_ ? floor_ : tau;
    f.tau = tau; f.ess = dn / tau; f.cut = (int32_t)(2 * K);
    return f;
}

int main()
{
    double worst = 0.0;
    long checked = 0;
    const int Ls[] = {1, 3, 15, 17, 63, 255};
    // ---- lag products against long double, and the pieces ----
    for (const double phi : {-0.5, 0.0, 0.8, 0.99})
        for (const int n : {4, 5, 17, 64, 65, 300, 1000})
            for (const int Lreq : Ls) {
                const int L = tme_lag_limit(Lreq, n);
                std::vector<double> x = ar1(phi, n, 7u + (unsigned)n, 3.0);
                long double mean = 0.0L;
                for (double v : x) mean += v;
                const double mu = (double)(mean / n);
                std::vector<double> d((size_t)n);
                for (int t = 0; t < n; t++) d[(size_t)t] = tme_centre_model(x[(size_t)t], mu);
                const std::vector<double> all = feed(d, L, n);
                for (int k = 0; k <= L; k++) {
                    long double ref = 0.0L, mag = 0.0L;
                    for (int t = k; t < n; t++) { const long double pr = (long double)d[(size_t)t] * (long double)d[(size_t)(t - k)]; ref += pr; mag += fabsl(pr); }
                    // n - k fused multiply-adds, each within half an ulp of a partial sum that never exceeds mag
                    const long double bound = (long double)(n - k) * 0x1p-53L * mag;
                    const long double err = fabsl((long double)all[(size_t)k] - ref);
                    CHECK(err <= bound, "phi %g n %d L %d k %d: |err| %Lg > %Lg", phi, n, L, k, err, bound);
                    if (bound > 0) worst = (double)(err / bound) > worst ? (double)(err / bound) : worst;
                    checked++;
                }
                for (const long long piece : {1LL, (long long)L - 1, (long long)L, (long long)L + 1, (long long)TM_ESS_G - 1, (long long)TM_ESS_G + 1,
                                              (long long)TM_ESS_CHUNK, (long long)TM_ESS_CHUNK + 1, 7LL}) {
                    if (piece < 1) continue;
                    const std::vector<double> got = feed(d, L, piece);
                    for (int k = 0; k <= L; k++)
                        CHECK(same_bits(got[(size_t)k], all[(size_t)k]), "phi %g n %d L %d piece %lld lag %d: %a != %a", phi, n, L, piece, k, got[(size_t)k], all[(size_t)k]);
                }
                // the plain one-sample walk (no chunks, no groups): the same bits
                for (int k = 0; k <= L; k++) {
                    double A = 0.0;
                    for (int t = k; t < n; t++) A = tme_acc(A, d[(size_t)t], d[(size_t)(t - k)]);
                    CHECK(same_bits(A, all[(size_t)k]), "phi %g n %d L %d lag %d: plain walk %a != %a", phi, n, L, k, A, all[(size_t)k]);
                }
            }
    // ---- constant series: every lag product is +0 and the finish says NaN, cut 0 ----
    {
        const int n = 200, L = 63;
        std::vector<double> d((size_t)n, 0.0);
        const std::vector<double> A = feed(d, L, 13);
        for (int k = 0; k <= L; k++) CHECK(same_bits(A[(size_t)k], 0.0), "constant series: lag %d is %a", k, A[(size_t)k]);
        const TmeFinish f = tme_finish(A.data(), 1, L, (double)n, 1.0 / std::log10((double)n));
        CHECK(std::isnan(f.tau) && std::isnan(f.ess) && f.cut == 0, "constant series: tau %g ess %g cut %d", f.tau, f.ess, f.cut);
    }
    // ---- +-inf and NaN: no 0 x inf from samples before the lag; the pieces agree; the finish refuses A_0 ----
    for (const double bad : {(double)INFINITY, -(double)INFINITY, (double)NAN})
        for (const int where : {0, 1, 40, 199}) {
            const int n = 200, L = 31;
            std::vector<double> d = ar1(0.5, n, 3u, 0.0);
            d[(size_t)where] = bad;
            const std::vector<double> all = feed(d, L, n);
            for (int k = 0; k <= L; k++) {
                double A = 0.0;
                for (int t = k; t < n; t++) A = tme_acc(A, d[(size_t)t], d[(size_t)(t - k)]);
                CHECK(same_bits(A, all[(size_t)k]) || (std::isnan(A) && std::isnan(all[(size_t)k])), "bad value at %d lag %d: %a != %a", where, k, all[(size_t)k], A);
                // the lags that never meet the bad sample stay finite
                const bool meets = where >= k || where + k < n;
                CHECK(meets || std::isfinite(all[(size_t)k]), "bad value at %d lag %d: not finite without meeting it", where, k);
            }
            for (const long long piece : {1LL, 30LL, 31LL, 32LL}) {
                const std::vector<double> got = feed(d, L, piece);
                for (int k = 0; k <= L; k++)
                    CHECK(same_bits(got[(size_t)k], all[(size_t)k]) || (std::isnan(got[(size_t)k]) && std::isnan(all[(size_t)k])), "bad value at %d piece %lld lag %d", where, piece, k);
            }
            const TmeFinish f = tme_finish(all.data(), 1, L, (double)n, 1.0 / std::log10((double)n));
            CHECK(std::isnan(f.tau) && std::isnan(f.ess) && f.cut == 0, "bad value at %d: tau %g cut %d", where, f.tau, f.cut);
        }
    // ---- the finish ----
    for (const double phi : {-0.5, 0.0, 0.8, 0.99})
        for (const int Lreq : {1, 15, 63, 255}) {
            const int n = 4000, L = tme_lag_limit(Lreq, n);
            std::vector<double> d = ar1(phi, n, 11u, 0.0);
            const std::vector<double> A = feed(d, L, 64);
            const double fl = 1.0 / std::log10((double)n);
            const TmeFinish f = tme_finish(A.data(), 1, L, (double)n, fl), g = finish_plain(A, L, (double)n, fl);
            CHECK(same_bits(f.tau, g.tau) && same_bits(f.ess, g.ess) && f.cut == g.cut, "finish phi %g L %d: %g %g %d against %g %g %d", phi, L, f.tau, f.ess, f.cut, g.tau, g.ess, g.cut);
            const double expect = n * (1.0 - phi) / (1.0 + phi);
            if (phi == 0.99 && L == 15) CHECK(f.cut == L + 1, "phi 0.99 at L 15 must be truncated: cut %d", f.cut);
            if (L == 255 && phi < 0.9) CHECK(f.ess > 0.5 * expect && f.ess < 2.0 * expect && f.cut < L + 1, "phi %g: ess %g, expected about %g, cut %d", phi, f.ess, expect, f.cut);
            if (phi == -0.5) CHECK(f.ess > n && f.ess <= n * std::log10((double)n), "phi -0.5: ess %g", f.ess);
        }
    {   // a NaN lag stops the sum; a negative pair stops it; the floor holds
        std::vector<double> A = {4.0, 2.0, 1.0, 0.5, NAN, 0.1, 0.05, 0.01};
        TmeFinish f = tme_finish(A.data(), 1, 7, 100.0, 0.5);
        CHECK(f.cut == 4 && f.tau == -1.0 + 2.0 * ((1.0 + 0.5) + (0.25 + 0.125)), "NaN lag: cut %d tau %g", f.cut, f.tau);
        A = {4.0, -3.9, 1.0, 0.5};
        f = tme_finish(A.data(), 1, 3, 100.0, 0.5);
        CHECK(f.cut == 4 && f.tau == 0.5 && f.ess == 200.0, "floor: cut %d tau %g ess %g", f.cut, f.tau, f.ess);
        A = {4.0, 1.0, -2.0, 0.5, 3.0, 3.0};
        f = tme_finish(A.data(), 1, 5, 100.0, 0.5);
        CHECK(f.cut == 2 && f.tau == -1.0 + 2.0 * 1.25, "negative pair: cut %d tau %g", f.cut, f.tau);
        A = {4.0, 0.0, 4.0, 4.0, 1.0, 1.0};                   // P = 1, 2, 0.5 -> monotone 1, 1, 0.5, truncated
        f = tme_finish(A.data(), 1, 5, 100.0, 0.5);
        CHECK(f.cut == 6 && f.tau == -1.0 + 2.0 * 2.5, "monotone: cut %d tau %g", f.cut, f.tau);
        A = {INFINITY, 1.0};
        f = tme_finish(A.data(), 1, 1, 100.0, 0.5);
        CHECK(std::isnan(f.tau) && f.cut == 0, "infinite A_0");
    }
    // ---- the lag limit ----
    CHECK(tme_lag_limit(0, 70000) == 255 && tme_lag_limit(0, 4) == 3 && tme_lag_limit(0, 5) == 3 && tme_lag_limit(0, 6) == 5, "default lag limit");
    CHECK(tme_lag_limit(1, 100) == 1 && tme_lag_limit(2, 100) == 3 && tme_lag_limit(62, 100) == 63 && tme_lag_limit(1023, 100) == 99 &&
          tme_lag_limit(1023, 101) == 99 && tme_lag_limit(1023, 2000) == 1023 && tme_lag_limit(1022, 2000) == 1023, "lag limit");
    // ---- split R-hat against long double ----
    for (const double shift : {0.0, 3.0})
        for (const int n : {4, 5, 1000, 1001}) {
            std::vector<double> x = ar1(0.3, n, 5u, 10.0);
            const long long h = n / 2;
            for (int t = n / 2; t < n; t++) x[(size_t)t] += shift;
            double m[2] = {0, 0}, q[2] = {0, 0};
            for (long long t = 0; t < n; t++) {
                if (t < h) tme_welford(&m[0], &q[0], t + 1, x[(size_t)t]);
                if (t >= n - h) tme_welford(&m[1], &q[1], t - (n - h) + 1, x[(size_t)t]);
            }
            const double got = tme_rhat(m[0], q[0], m[1], q[1], h);
            long double mu[2] = {0, 0}, var[2] = {0, 0};
            for (long long t = 0; t < h; t++) { mu[0] += x[(size_t)t]; mu[1] += x[(size_t)(n - h + t)]; }
            mu[0] /= h; mu[1] /= h;
            for (long long t = 0; t < h; t++) {
                var[0] += (x[(size_t)t] - mu[0]) * (x[(size_t)t] - mu[0]);
                var[1] += (x[(size_t)(n - h + t)] - mu[1]) * (x[(size_t)(n - h + t)] - mu[1]);
            }
            const long double W = (var[0] + var[1]) / (h - 1) / 2, mb = (mu[0] + mu[1]) / 2;
            const long double Bn = (mu[0] - mb) * (mu[0] - mb) + (mu[1] - mb) * (mu[1] - mb);
            const long double want = sqrtl(((long double)(h - 1) / h * W + Bn) / W);
            CHECK(fabsl(got - want) <= 1e-12L * want, "rhat n %d shift %g: %.17g against %.17Lg", n, shift, got, want);
            if (n >= 1000) CHECK(shift == 0.0 ? got < 1.01 : got > 1.5, "rhat n %d shift %g: %g", n, shift, got);
        }
    CHECK(std::isnan(tme_rhat(1.0, 0.0, 2.0, 0.0, 5)), "rhat of two constant halves");
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok ess_core_check: %ld lag products within their bound (worst ratio %.3f), pieces, finish, lag limit, R-hat\n", checked, worst);
    return 0;
}
