// predictive_core_check -- the per-sample arithmetic of the posterior predictive check (tamcmc-c-_amd/csrc/
// tamcmc_predictive.h) on the CPU, with the header's own functions: log P and log Q of chi(2,2p) and of the Gaussian
// against a long-double brute force, their sum, their monotony across every branch switch, and the guarded log-sum-exp.
//   g++ -std=c++17 -O1 -I tamcmc-c-_amd/csrc tests/cpp/predictive_core_check.cpp -o predictive_core_check && ./predictive_core_check
// Prints one `ok` line; any failure prints what failed and exits 1.  (tests/test_summary_predictive_host.py builds and
// runs it.)
//
// Bounds, relative to max(1, |value|):
//   p = 1, Gaussian   16 x 2^-52: a handful of correctly rounded operations and libm calls of about an ulp each.
//   p > 1             2^-42 = 4 ulp(256): at p = 64 and z near p the terms -z, (p-1) log z and log (p-1)! are 200 ... 260
//                     each, every one carries a rounding of up to ulp(256) / 2 (log z another (p-1) ulp(log z)), and they
//                     cancel to a value of order 1.
// The brute force's own error is below 1e-15 (long double sums of at most a few thousand positive terms; the largest
// logarithm it forms is 3e4).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "tamcmc_predictive.h"

typedef long double LD;

static int failures = 0;
#define CHECK(cond, ...)                                                            \
    do {                                                                            \
        if (!(cond)) {                                                              \
            if (failures++ < 20) { fprintf(stderr, "FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
        }                                                                           \
    } while (0)

static const double INF = std::numeric_limits<double>::infinity();
static const double TOL_1 = 16.0 * 0x1p-52, TOL_P = 0x1p-42;
static double worst_1 = 0.0, worst_p = 0.0, worst_g = 0.0;

static LD lse(const std::vector<LD> &t)
{
    LD m = t[0];
    for (LD v : t) m = v > m ? v : m;
    LD s = 0.0L;
    for (LD v : t) s += expl(v - m);
    return m + logl(s);
}

// log Q(p, z) = log(exp(-z) sum_{k<p} z^k / k!)
static LD ref_logQ(int p, double z)
{
    if (z <= 0.0) return 0.0L;
    std::vector<LD> t;
    for (int k = 0; k < p; k++) t.push_back((LD)k * logl((LD)z) - lgammal((LD)k + 1.0L) - (LD)z);
    return lse(t);
}

// log P(p, z) = log(exp(-z) sum_{k>=p} z^k / k!): the Poisson tail summed until it is exhausted; past z = 4000, where
// Q < 1e-1000, log(1 - Q) = -Q to every digit
static LD ref_logP(int p, double z)
{
    if (z <= 0.0) return -(LD)INF;
    if (z > 4000.0) return -expl(ref_logQ(p, z));
    const int kmax = p + (int)(z + 12.0 * std::sqrt(z + 1.0) + 80.0);
    std::vector<LD> t;
    for (int k = p; k <= kmax; k++) t.push_back((LD)k * logl((LD)z) - lgammal((LD)k + 1.0L) - (LD)z);
    return lse(t);
}

// log(erfc(r) / 2); past r = 100 erfcl underflows and the asymptotic series takes over (its terms fall below 1e-22 at once)
static LD ref_log_half_erfc(double r)
{
    const LD x = (LD)r;
    if (r < 0.0) return log1pl(-0.5L * erfcl(-x));
    if (r <= 100.0) return logl(0.5L * erfcl(x));
    LD s = 1.0L, t = 1.0L;
    for (int k = 1; k < 40; k++) {
        t *= -(LD)(2 * k - 1) / (2.0L * x * x);
        s += t;
        if (fabsl(t) < 1e-22L) break;
    }
    return -x * x - logl(x) - 0.5L * logl(acosl(-1.0L)) + logl(s) - logl(2.0L);
}

static double rel(double got, LD want)
{
    if (std::isinf(got) || std::isinf((double)want)) return (LD)got == want ? 0.0 : INF;
    const LD scale = fabsl(want) > 1.0L ? fabsl(want) : 1.0L;
    return (double)(fabsl((LD)got - want) / scale);
}

static double logaddexp(double a, double b)
{
    const double m = a > b ? a : b, d = a > b ? b - a : a - b;
    return d == -INF ? m : m + std::log1p(std::exp(d));
}

static void chi(int p, double z, double *lP, double *lQ)
{
    if (p == 1) tmp_chi_p1(z, lP, lQ);
    else tmp_chi_p(p, tmp_log_factorial(p - 1), tmp_log_factorial(p), tmp_series_terms(p), z, lP, lQ);
}

static long check_chi()
{
    long checked = 0;
    const int ps[] = {1, 2, 3, 17, 64};
    for (int p : ps) {
        const double dp = (double)p, tol = p == 1 ? TOL_1 : TOL_P;
        double &worst = p == 1 ? worst_1 : worst_p;
        std::vector<double> zs = {0.0, 4.9406564584124654e-324, 1e-300, 1e-10, 0.1, 1.0, dp - 1.0, dp - 0.5, dp + 0.5, dp, 50.0, 745.0,
                                  2000.0, 1e6, 1e300,
                                  // both sides of every switch: ln 2 (p = 1), p - 1 (log Q), p (log P)
                                  TMP_LN2, std::nextafter(TMP_LN2, 1.0), std::nextafter(dp - 1.0, 0.0), std::nextafter(dp, 0.0), std::nextafter(dp, 100.0)};
        std::sort(zs.begin(), zs.end());
        double prevP = -INF, prevQ = 0.0, prevz = -1.0;
        for (double z : zs) {
            if (z == prevz) continue;
            double lP = 7.0, lQ = 7.0;
            chi(p, z, &lP, &lQ);
            const LD rP = ref_logP(p, z), rQ = ref_logQ(p, z);
            const double eP = rel(lP, rP), eQ = rel(lQ, rQ);
            worst = std::max(worst, std::max(eP, eQ));
            CHECK(eP <= tol, "p=%d z=%.17g: logP %.17g, reference %.20Lg (%.3g)", p, z, lP, rP, eP);
            CHECK(eQ <= tol, "p=%d z=%.17g: logQ %.17g, reference %.20Lg (%.3g)", p, z, lQ, rQ, eQ);
            CHECK(!std::isnan(lP) && !std::isnan(lQ) && lP <= 0.0 && lQ <= 0.0, "p=%d z=%.17g: %g %g", p, z, lP, lQ);
            CHECK(z <= 0.0 || (std::isfinite(lP) && std::isfinite(lQ)), "p=%d z=%.17g: a tail is not finite: %g %g", p, z, lP, lQ);
            CHECK(std::fabs(logaddexp(lP, lQ)) <= tol, "p=%d z=%.17g: log(P + Q) = %.3g", p, z, logaddexp(lP, lQ));
            // monotone: exactly between points a grid step apart; across a switch (neighbouring doubles) within the bound
            const bool neighbours = prevz > 0.0 && z == std::nextafter(prevz, INF);
            const double slackP = neighbours ? tol * std::max(1.0, std::fabs(lP)) : 0.0, slackQ = neighbours ? tol * std::max(1.0, std::fabs(lQ)) : 0.0;
            CHECK(lP >= prevP - slackP, "p=%d z=%.17g: logP falls from %.17g to %.17g", p, z, prevP, lP);
            CHECK(lQ <= prevQ + slackQ, "p=%d z=%.17g: logQ rises from %.17g to %.17g", p, z, prevQ, lQ);
            prevP = lP; prevQ = lQ; prevz = z;
            checked++;
        }
        double lP = 7.0, lQ = 7.0;
        chi(p, -3.0, &lP, &lQ);
        CHECK(lP == -INF && lQ == 0.0, "p=%d z<0: %g %g", p, lP, lQ);
        chi(p, 0.0, &lP, &lQ);
        CHECK(lP == -INF && lQ == 0.0, "p=%d z=0: %g %g", p, lP, lQ);
        chi(p, 2000.0 * dp, &lP, &lQ);
        CHECK(std::isfinite(lQ) && lQ < -745.0 * dp, "p=%d z=2000p: logQ %g", p, lQ);
        const int J = tmp_series_terms(p);
        CHECK(J >= 10 && J <= 90, "series terms at p=%d: %d", p, J);
    }
    CHECK(tmp_series_terms(TM_PRED_MAX_P) <= 90, "series terms at the largest p: %d", tmp_series_terms(TM_PRED_MAX_P));
    return checked;
}

static long check_gauss()
{
    long checked = 0;
    std::vector<double> rs = {0.0};
    for (double r : {1e-8, 1.0, 5.0, 26.0, 27.0, 40.0, 1e3}) { rs.push_back(r); rs.push_back(-r); }
    rs.push_back(std::nextafter(TMP_GAUSS_SWITCH, 100.0));
    rs.push_back(-std::nextafter(TMP_GAUSS_SWITCH, 100.0));
    std::sort(rs.begin(), rs.end());
    double prevP = -INF, prevQ = 0.0;
    for (double r : rs) {
        double lP = 7.0, lQ = 7.0;
        tmp_gauss(r, &lP, &lQ);
        const LD rP = ref_log_half_erfc(-r), rQ = ref_log_half_erfc(r);
        const double eP = rel(lP, rP), eQ = rel(lQ, rQ);
        worst_g = std::max(worst_g, std::max(eP, eQ));
        CHECK(eP <= TOL_1, "r=%.17g: logP %.17g, reference %.20Lg (%.3g)", r, lP, rP, eP);
        CHECK(eQ <= TOL_1, "r=%.17g: logQ %.17g, reference %.20Lg (%.3g)", r, lQ, rQ, eQ);
        CHECK(std::isfinite(lP) && std::isfinite(lQ) && lP <= 0.0 && lQ <= 0.0, "r=%.17g: %g %g", r, lP, lQ);
        CHECK(std::fabs(logaddexp(lP, lQ)) <= TOL_1, "r=%.17g: log(P + Q) = %.3g", r, logaddexp(lP, lQ));
        const double slackP = TOL_1 * std::max(1.0, std::fabs(lP)), slackQ = TOL_1 * std::max(1.0, std::fabs(lQ));   // (the switch's neighbours are in the list)
        CHECK(lP >= prevP - slackP, "r=%.17g: logP falls from %.17g to %.17g", r, prevP, lP);
        CHECK(lQ <= prevQ + slackQ, "r=%.17g: logQ rises from %.17g to %.17g", r, prevQ, lQ);
        prevP = lP; prevQ = lQ;
        checked++;
    }
    double lP, lQ;
    tmp_gauss(40.0, &lP, &lQ);
    CHECK(std::fabs(lQ + 1604.6) < 1.0 && lP > -1e-300 && lP <= 0.0, "r=40: %g %g", lP, lQ);
    tmp_gauss(-40.0, &lP, &lQ);
    CHECK(std::fabs(lP + 1604.6) < 1.0 && lQ > -1e-300 && lQ <= 0.0, "r=-40: %g %g", lP, lQ);
    return checked;
}

static double fold(const std::vector<double> &x)
{
    double a = 0.0, r = 0.0, c = 0.0;   // the state starts as zeros
    for (double v : x) tmp_lse_step(&a, &r, &c, v);
    CHECK(!std::isnan(a) && !std::isnan(r) && !std::isnan(c), "the state holds a NaN");
    return tmp_lse_result(a, r, c, (long long)x.size());
}

static long check_lse()
{
    const double x = -1234.5;
    CHECK(std::isnan(fold({})), "an empty chain is not NaN");
    CHECK(fold({-INF, -INF}) == -INF, "(-inf, -inf): %g", fold({-INF, -INF}));
    CHECK(fold({-INF}) == -INF, "(-inf): %g", fold({-INF}));
    CHECK(fold({-INF, x}) == x + std::log(0.5), "(-inf, x): %.17g", fold({-INF, x}));
    CHECK(fold({x, -INF}) == x + std::log(0.5), "(x, -inf): %.17g", fold({x, -INF}));
    CHECK(fold({x, x, x, x, x}) == x, "all equal: %.17g", fold({x, x, x, x, x}));
    CHECK(fold({0.0, 0.0, 0.0}) == 0.0, "all zero: %.17g", fold({0.0, 0.0, 0.0}));
    CHECK(fold({-INF, 0.0, -INF, 0.0}) == std::log(0.5), "(-inf, 0, -inf, 0): %.17g", fold({-INF, 0.0, -INF, 0.0}));
    // rising and falling: the maximum follows, and the order changes the last bits at most
    const double up = fold({-2000.0, -1000.0, -3.0}), down = fold({-3.0, -1000.0, -2000.0});
    CHECK(std::fabs(up - (-3.0 + std::log(1.0 / 3.0))) < 1e-15 && std::fabs(down - up) < 1e-15, "rising %.17g falling %.17g", up, down);
    // 70 001 terms near 0, the largest first / last / in the middle: log of their mean against long double, within 4 ulp
    // of 1 (a plain sum loses about sqrt(n) ulp here)
    for (int where = 0; where < 3; where++) {
        std::vector<double> t;
        LD sum = 0.0L;
        for (int k = 0; k < 70001; k++) {
            const double v = -1e-9 * (1.0 + ((k * 7919) % 1000) / 1000.0);
            t.push_back(k == (where == 0 ? 0 : where == 1 ? 70000 : 35000) ? -1e-12 : v);
            sum += expl((LD)t.back());
        }
        const LD want = logl(sum / 70001.0L);
        const double got = fold(t);
        CHECK(fabsl((LD)got - want) <= 4.0 * 0x1p-52, "long sum %d: %.17g against %.20Lg", where, got, want);
    }
    return 13;
}

int main()
{
    const long n = check_chi() + check_gauss() + check_lse();
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok predictive_core_check: %ld cases; worst error p=1 %.2g, p>1 %.2g, gauss %.2g\n", n, worst_1, worst_p, worst_g);
    return 0;
}
