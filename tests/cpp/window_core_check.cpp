// window_core_check -- the per-(sample, window) arithmetic of the windowed predictive check (tamcmc-c-_amd/csrc/
// tamcmc_window.h) on the CPU, with the header's own functions: the partition into windows, the ascending window sum,
// and log P / log Q of the window sum at shapes up to 512 and of the Gaussian form against a long-double brute force.
//   g++ -std=c++17 -O1 -I tamcmc-c-_amd/csrc tests/cpp/window_core_check.cpp -o window_core_check && ./window_core_check
// Prints one `ok` line with the worst error per shape; any failure prints what failed and exits 1.
// (tests/test_summary_window_host.py builds and runs it.)
//
// The brute force: log Q(a, z) is a long-double log-sum-exp of all a terms k log z - log k! - z; log P(a, z) the same over
// the Poisson tail k >= a until it is exhausted, or log(1 - Q) = -Q past z = 4000 where Q < 1e-1000.  Its own error is a
// few long-double ulp of the largest term, 4e3 at shape 512: below 1e-15.
// z per shape a: 1e-300, 1e-3, both sides of a/2, of a - 1 and of a, a + 1, 2a, 4a, 1e4, 1e300, and 300 draws from
// Gamma(a) (minus the sum of a logarithms of uniforms from a fixed splitmix64 stream).
// Bars, relative to max(1, |value|): the power of two at or above twice the worst error this check measured -- the z
// sample is finite, hence the factor -- per shape, in BAR[] below beside the measured value.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "tamcmc_window.h"

typedef long double LD;

static int failures = 0;
#define CHECK(cond, ...)                                                            \
    do {                                                                            \
        if (!(cond)) {                                                              \
            if (failures++ < 20) { fprintf(stderr, "FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
        }                                                                           \
    } while (0)

static const double INF = std::numeric_limits<double>::infinity();

//                              shape, measured worst, bar
static const struct { int a; double measured, bar; } BAR[] = {
    {1, 1.41e-16, 0x1p-51}, {2, 6.63e-16, 0x1p-49}, {3, 7.44e-16, 0x1p-49}, {25, 2.26e-15, 0x1p-47}, {64, 4.64e-15, 0x1p-46},
    {256, 1.67e-14, 0x1p-44}, {511, 3.01e-14, 0x1p-43}, {512, 3.24e-14, 0x1p-43},
};
static const double BAR_GAUSS = 0x1p-50;      // measured 2.92e-16

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static double uniform()                       // splitmix64, in (0, 1)
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return ((double)(z >> 11) + 0.5) * 0x1p-53;
}

static LD lse(const std::vector<LD> &t)
{
    LD m = t[0];
    for (LD v : t) m = v > m ? v : m;
    LD s = 0.0L;
    for (LD v : t) s += expl(v - m);
    return m + logl(s);
}

static LD ref_logQ(int a, double z)
{
    if (z <= 0.0) return 0.0L;
    std::vector<LD> t;
    for (int k = 0; k < a; k++) t.push_back((LD)k * logl((LD)z) - lgammal((LD)k + 1.0L) - (LD)z);
    return lse(t);
}

static LD ref_logP(int a, double z)
{
    if (z <= 0.0) return -(LD)INF;
    if (z > 4000.0) return -expl(ref_logQ(a, z));
    const int kmax = a + (int)(z + 12.0 * std::sqrt(z + 1.0) + 80.0);
    std::vector<LD> t;
    for (int k = a; k <= kmax; k++) t.push_back((LD)k * logl((LD)z) - lgammal((LD)k + 1.0L) - (LD)z);
    return lse(t);
}

// log(erfc(r) / 2) of a long-double argument; past 100 erfcl underflows and the asymptotic series takes over
static LD ref_log_half_erfc(LD x)
{
    if (x < 0.0L) return log1pl(-0.5L * erfcl(-x));
    if (x <= 100.0L) return logl(0.5L * erfcl(x));
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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static long check_shapes(double worst[])
{
    long checked = 0;
    int idx = 0;
    for (const auto &bar : BAR) {
        const int a = bar.a;
        const double da = (double)a;
        // the shape as a window of `a` bins at p = 1 -- and, where it divides, as fewer bins at a larger p: the same numbers
        const TmWinShape sh = tmw_shape(a, 1);
        CHECK(sh.a == a && sh.len == a && sh.nterms == tmp_series_terms(a), "shape %d", a);
        std::vector<double> zs = {1e-300, 1e-3, std::nextafter(da / 2, 0.0), da / 2, std::nextafter(da - 1.0, 0.0), da - 1.0, std::nextafter(da, 0.0), da,
                                  std::nextafter(da, 1e9), da + 1.0, 2 * da, 4 * da, 1e4, 1e300};
        for (int k = 0; k < 300; k++) {
            double g = 0.0;
            for (int j = 0; j < a; j++) g -= std::log(uniform());
            zs.push_back(g);
        }
        double w = 0.0;
        for (double z : zs) {
            double lP = 7.0, lQ = 7.0;
            tmw_chi(sh, 1, z, &lP, &lQ);
            if (z <= 0.0) {                                    // (a - 1 at shape 1, and the double below it)
                CHECK(lP == -INF && lQ == 0.0, "shape %d z=%g: %g %g", a, z, lP, lQ);
                continue;
            }
            const LD rP = ref_logP(a, z), rQ = ref_logQ(a, z);
            const double eP = rel(lP, rP), eQ = rel(lQ, rQ);
            w = std::max(w, std::max(eP, eQ));
            CHECK(eP <= bar.bar, "shape %d z=%.17g: logP %.17g, reference %.20Lg (%.3g)", a, z, lP, rP, eP);
            CHECK(eQ <= bar.bar, "shape %d z=%.17g: logQ %.17g, reference %.20Lg (%.3g)", a, z, lQ, rQ, eQ);
            CHECK(std::isfinite(lP) && std::isfinite(lQ) && lP <= 0.0 && lQ <= 0.0, "shape %d z=%.17g: %g %g", a, z, lP, lQ);
            checked++;
        }
        worst[idx++] = w;
        if (a % 2 == 0 && a > 2) {                             // p = 2 over a / 2 bins: z = 2 S
            const TmWinShape h = tmw_shape(a / 2, 2);
            double lP, lQ, mP, mQ;
            tmw_chi(h, 2, 0.375 * da, &lP, &lQ);
            tmw_chi(sh, 1, 0.75 * da, &mP, &mQ);
            CHECK(h.a == a && same_bits(lP, mP) && same_bits(lQ, mQ), "shape %d as p = 2: %.17g %.17g against %.17g %.17g", a, lP, lQ, mP, mQ);
        }
    }
    CHECK(tmp_series_terms(TM_WIN_MAX_SHAPE) == 216, "series terms at shape 512: %d", tmp_series_terms(TM_WIN_MAX_SHAPE));
    // one bin per window: the per-bin check's own calls, bit for bit
    for (double S : {0.0, -1.0, 1e-300, 0.3, 1.0, 2.5, 40.0, 2000.0}) {
        double lP, lQ, mP, mQ;
        tmw_chi(tmw_shape(1, 1), 1, S, &lP, &lQ);
        tmp_chi_p1(S, &mP, &mQ);
        CHECK(same_bits(lP, mP) && same_bits(lQ, mQ), "W = 1, p = 1, S=%g", S);
        tmw_chi(tmw_shape(1, 4), 4, S, &lP, &lQ);
        tmp_chi_p(4, tmp_log_factorial(3), tmp_log_factorial(4), tmp_series_terms(4), 4.0 * S, &mP, &mQ);
        CHECK(same_bits(lP, mP) && same_bits(lQ, mQ), "W = 1, p = 4, S=%g", S);
    }
    return checked;
}

static long check_gauss(double *worst)
{
    long checked = 0;
    for (int len : {1, 2, 7, 512}) {
        const TmWinShape sh = tmw_shape(len, 1);
        CHECK(sh.c == 1.0 / std::sqrt((double)len) && (len != 1 || sh.c == 1.0), "c at len %d", len);
        const double root = std::sqrt((double)len);
        std::vector<double> Rs = {0.0};
        for (double g : {1e-8, 0.3, 1.0, 5.0, 25.9, 26.1, 40.0, 1e3}) { Rs.push_back(g * root); Rs.push_back(-g * root); }
        for (double R : Rs) {
            double lP = 7.0, lQ = 7.0;
            tmw_gauss(sh, R, &lP, &lQ);
            const LD g = (LD)R / sqrtl((LD)len);
            const LD rP = ref_log_half_erfc(-g), rQ = ref_log_half_erfc(g);
            const double eP = rel(lP, rP), eQ = rel(lQ, rQ);
            *worst = std::max(*worst, std::max(eP, eQ));
            CHECK(eP <= BAR_GAUSS, "len %d R=%.17g: logP %.17g, reference %.20Lg (%.3g)", len, R, lP, rP, eP);
            CHECK(eQ <= BAR_GAUSS, "len %d R=%.17g: logQ %.17g, reference %.20Lg (%.3g)", len, R, lQ, rQ, eQ);
            CHECK(std::isfinite(lP) && std::isfinite(lQ) && lP <= 0.0 && lQ <= 0.0, "len %d R=%.17g: %g %g", len, R, lP, lQ);
            if (len == 1) {
                double mP, mQ;
                tmp_gauss(R, &mP, &mQ);
                CHECK(same_bits(lP, mP) && same_bits(lQ, mQ), "W = 1, R=%g", R);
            }
            checked++;
        }
    }
    return checked;
}

static long check_sum_and_partition()
{
    // ascending: ((1e16 + 1) + 1) - 1e16 = 0 in doubles; any order that adds the two ones first gives 2
    const double q[4] = {1e16, 1.0, 1.0, -1e16};
    CHECK(tmw_sum(q, 4) == 0.0, "the window sum is not ascending: %g", tmw_sum(q, 4));
    CHECK(tmw_sum(q, 3) == 1e16 && tmw_sum(q + 1, 3) == -1e16 + 2.0, "partial sums");
    const double mz = -0.0;
    CHECK(same_bits(tmw_sum(&mz, 1), -0.0) && tmw_sum(q + 1, 1) == 1.0, "a sum of one term is not that term");
    std::vector<double> v(512);
    for (double &t : v) t = -std::log(uniform());
    double s = v[0];
    for (int i = 1; i < 512; i++) s += v[i];
    CHECK(same_bits(tmw_sum(v.data(), 512), s), "512 terms");

    long checked = 5;
    const long long grids[] = {1, 2, 7, 64, 65, 700, 5000};
    const int Ws[] = {1, 2, 3, 7, 64, 100, 512};
    for (long long Nx : grids)
        for (int W : Ws)
            for (int first0 : {0, 1, 3, W - 1, W}) {
                if (first0 < 0 || first0 > W) continue;
                int first = first0, len[3];
                const long long nw = tmw_partition(Nx, W, &first, len);
                CHECK(first >= 1 && first <= W && (first0 == 0 ? first == W : first == first0), "first %d -> %d", first0, first);
                const long long rest = Nx > first ? Nx - first : 0;
                CHECK(nw == 1 + (rest + W - 1) / W, "Nx=%lld W=%d first=%d: %lld windows", Nx, W, first, nw);
                long long next = 0;
                for (long long w = 0; w < nw; w++) {           // disjoint, in order, covering the grid, no window empty
                    const long long b = tmw_begin(w, W, first), e = tmw_end(w, W, first, Nx);
                    CHECK(b == next && e > b && e - b == len[tmw_kind(w, nw)], "Nx=%lld W=%d first=%d window %lld: [%lld, %lld), kind %d of length %d",
                          Nx, W, first, w, b, e, tmw_kind(w, nw), len[tmw_kind(w, nw)]);
                    next = e;
                }
                CHECK(next == Nx, "Nx=%lld W=%d first=%d: the windows end at %lld", Nx, W, first, next);
                checked++;
            }
    return checked;
}

int main()
{
    double worst[sizeof BAR / sizeof BAR[0]] = {}, worst_g = 0.0;
    const long n = check_shapes(worst) + check_gauss(&worst_g) + check_sum_and_partition();
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); }
    printf("%s window_core_check: %ld cases; worst error", failures ? "FAILED" : "ok", n);
    for (size_t k = 0; k < sizeof BAR / sizeof BAR[0]; k++) printf(" a=%d %.3g", BAR[k].a, worst[k]);
    printf(", gauss %.3g\n", worst_g);
    return failures ? 1 : 0;
}
