// modepdf_core_check.cpp -- the arithmetic of tamcmc_modepdf.h on the CPU (plain g++, no GPU, no library):
//   * the class rule and tmp_host_hist against a brute-force count per class (floor instead of the cast, one pass per class)
//     on random columns and ranges, and against integer arithmetic on a dyadic range with a value exactly on every edge:
//     the value on edge b counts in class b, v == hi in the last class; hi == lo (class 0, the rest below / above); a range
//     whose difference overflows and non-finite ranges (tmp_range_ok); +-inf values (below / above); all values equal; a
//     range so narrow that the scale overflows; the plot edges (edge 0 = lo, edge n_bins = hi exactly, dyadic ones exact);
//   * tmp_host_hist2d against the same brute force per axis, its row and column sums against the 1-D counts of the samples
//     inside the range, a pair of a column with itself (the diagonal only);
//   * the window length (k = 1 at mass 1 / n, k = n at mass 1, the clamps), the width order (total: NaN last, smaller
//     width, smaller index; antisymmetric and transitive over a set of widths with NaN, +-inf and ties), and tmp_host_hpd
//     against a three-pass brute force on columns with ties, +-0, +-inf, all values equal, integer columns with many tied
//     widths (the first index wins), k = 1 and k = n; a reduction in any grouping gives the same answer;
//   * the level rule against a brute force over every t, with a level tie, n_in = 0 and mass 1.
// Prints "ok modepdf_core_check ..." and exits 0, or says what failed and exits 1.  May be built with
// -fsanitize=address,undefined and run as it is.
#include "tamcmc_modepdf.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static bool same_bits(const double a, const double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static const double INF = std::numeric_limits<double>::infinity();

// class of v by the rule's words, with floor and the clamp written out: -1 below, -2 above
static long long brute_class(const double v, const double lo, const double hi, const int nb)
{
    if (v < lo) return -1;
    if (v > hi) return -2;
    if (!(hi > lo)) return 0;
    volatile double s = (double)nb / (hi - lo);
    volatile double d = v - lo;
    volatile double u = d * s;
    if (std::isnan(u)) return 0;
    const double f = std::floor(u);
    return f > (double)(nb - 1) ? nb - 1 : (long long)f;
}

static long hist_case(const std::vector<double> &v, const double lo, const double hi, const int nb)
{
    const long long n = (long long)v.size();
    std::vector<int64_t> c((size_t)nb, -7);
    int64_t below = -7, above = -7;
    tmp_host_hist(v.data(), n, lo, hi, nb, c.data(), &below, &above);
    int64_t sum = below + above;
    for (int b = -2; b < nb; b++) {
        int64_t want = 0;
        for (const double x : v) want += brute_class(x, lo, hi, nb) == b;
        const int64_t got = b == -1 ? below : (b == -2 ? above : c[(size_t)b]);
        CHECK(got == want, "hist n=%lld nb=%d [%a, %a] class %d: %lld, want %lld", n, nb, lo, hi, b, (long long)got, (long long)want);
        if (b >= 0) sum += got;
    }
    CHECK(sum == n, "hist n=%lld nb=%d: the counts sum to %lld", n, nb, (long long)sum);
    return nb + 2;
}

static long check_hist(std::mt19937_64 &g)
{
    long checks = 0;
    std::normal_distribution<double> N(0.0, 1.0);
    for (const int n : {1, 2, 3, 64, 257, 1000})
        for (const int nb : {1, 2, 3, 7, 50, 64, 65, 300}) {
            std::vector<double> v((size_t)n);
            for (auto &x : v) x = 3000.0 + 2.5 * N(g);
            const double mn = *std::min_element(v.begin(), v.end()), mx = *std::max_element(v.begin(), v.end());
            checks += hist_case(v, mn, mx, nb);                                       // the default range
            checks += hist_case(v, 2999.0, 3001.5, nb);                              // cuts both tails
            v[0] = INF; v[(size_t)n - 1] = n > 1 ? -INF : INF;
            checks += hist_case(v, 2999.0, 3001.5, nb);                              // +-inf: above, below
            std::fill(v.begin(), v.end(), 7.25);
            checks += hist_case(v, 7.25, 7.25, nb);                                  // all equal: hi == lo, class 0
            checks += hist_case(v, 7.0, 7.5, nb);
            v[0] = 7.0; if (n > 1) v[1] = 7.5;
            checks += hist_case(v, 7.25, 7.25, nb);                                  // hi == lo with values on both sides
        }
    // a dyadic range: [lo, lo + nb w], w a power of two; a value exactly on every edge, one in every class' interior
    for (const int nb : {1, 2, 8, 64, 100, 4096})
        for (const double w : {0.25, 1.0, 8.0})
            for (const double lo : {0.0, -16.0, 1024.0}) {
                const double hi = lo + nb * w;
                std::vector<double> v;
                for (int b = 0; b <= nb; b++) v.push_back(lo + b * w);
                for (int b = 0; b < nb; b++) v.push_back(lo + b * w + 0.5 * w);
                std::vector<int64_t> c((size_t)nb);
                int64_t below, above;
                tmp_host_hist(v.data(), (long long)v.size(), lo, hi, nb, c.data(), &below, &above);
                bool ok = below == 0 && above == 0;
                for (int b = 0; b < nb; b++) ok = ok && c[(size_t)b] == (b == nb - 1 ? 3 : 2);        // edge b, the interior, and v == hi in the last
                CHECK(ok, "dyadic nb=%d w=%g lo=%g", nb, w, lo);
                const double s = tmp_scale(lo, hi, nb);
                for (int b = 0; b <= nb; b++) {
                    CHECK(tmp_class(lo + b * w, lo, hi, s, nb) == (b < nb ? b : nb - 1), "edge %d of %d", b, nb);
                    if ((nb & (nb - 1)) == 0) CHECK(same_bits(tmp_edge(lo, hi, b, nb), lo + b * w), "plot edge %d of %d", b, nb);   // (b / nb exact)
                    checks += 2;
                }
                CHECK(tmp_class(std::nextafter(lo, -INF), lo, hi, s, nb) == TM_PDF_BELOW && tmp_class(std::nextafter(hi, INF), lo, hi, s, nb) == TM_PDF_ABOVE, "outside");
                checks++;
            }
    // plot edges of a range that is no lattice: the first is lo, the last hi exactly
    CHECK(same_bits(tmp_edge(0.1, 0.7, 0, 7), 0.1) && same_bits(tmp_edge(0.1, 0.7, 7, 7), 0.7) && tmp_edge(0.1, 0.7, 3, 7) > 0.1 && tmp_edge(0.1, 0.7, 3, 7) < 0.7, "plot edges");
    // ranges: finite, ordered, a finite difference
    const double big = std::numeric_limits<double>::max();
    CHECK(tmp_range_ok(0.0, 0.0) && tmp_range_ok(-1.0, 2.0) && tmp_range_ok(-0.5 * big, 0.4 * big), "good ranges");
    CHECK(!tmp_range_ok(-big, big) && !tmp_range_ok(1.0, 0.0) && !tmp_range_ok(0.0, INF) && !tmp_range_ok(-INF, 0.0) && !tmp_range_ok(INF, INF) &&
          !tmp_range_ok(NAN, 1.0) && !tmp_range_ok(0.0, NAN), "bad ranges");
    // a range so narrow that the scale overflows: lo in class 0, everything above it in the last class
    {
        const double lo = 0.0, hi = 3 * std::numeric_limits<double>::denorm_min();
        const int nb = 4096;
        const double s = tmp_scale(lo, hi, nb);
        CHECK(std::isinf(s), "the scale overflows");
        CHECK(tmp_class(lo, lo, hi, s, nb) == 0 && tmp_class(hi, lo, hi, s, nb) == nb - 1 && tmp_class(hi / 3, lo, hi, s, nb) == nb - 1, "overflowed scale");
        checks += hist_case({lo, hi, hi / 3, -1.0, 1.0}, lo, hi, nb);
    }
    return checks + 5;
}

static long check_hist2d(std::mt19937_64 &g)
{
    long checks = 0;
    std::normal_distribution<double> N(0.0, 1.0);
    for (const int n : {1, 5, 300})
        for (const int nb : {1, 2, 9, 32}) {
            std::vector<double> x((size_t)n), y((size_t)n);
            for (int t = 0; t < n; t++) { x[(size_t)t] = N(g); y[(size_t)t] = 0.5 * x[(size_t)t] + N(g); }
            if (n > 2) { x[1] = INF; y[2] = -INF; }
            const double lox = -1.5, hix = 1.25, loy = -2.0, hiy = 1.0;
            std::vector<int64_t> c((size_t)nb * (size_t)nb);
            int64_t outside;
            tmp_host_hist2d(x.data(), y.data(), n, lox, hix, loy, hiy, nb, c.data(), &outside);
            int64_t sum = outside, want_out = 0;
            std::vector<int64_t> row((size_t)nb, 0), col((size_t)nb, 0);
            for (int t = 0; t < n; t++) {
                const long long a = brute_class(x[(size_t)t], lox, hix, nb), b = brute_class(y[(size_t)t], loy, hiy, nb);
                if (a < 0 || b < 0) { want_out++; continue; }
                row[(size_t)a]++; col[(size_t)b]++;
            }
            for (int a = 0; a < nb; a++)
                for (int b = 0; b < nb; b++) {
                    int64_t want = 0;
                    for (int t = 0; t < n; t++) want += brute_class(x[(size_t)t], lox, hix, nb) == a && brute_class(y[(size_t)t], loy, hiy, nb) == b;
                    CHECK(c[(size_t)a * nb + b] == want, "hist2d n=%d nb=%d cell (%d, %d)", n, nb, a, b);
                    sum += c[(size_t)a * nb + b]; row[(size_t)a] -= want; col[(size_t)b] -= want;
                    checks++;
                }
            bool ok = outside == want_out && sum == n;
            for (int a = 0; a < nb; a++) ok = ok && row[(size_t)a] == 0 && col[(size_t)a] == 0;
            CHECK(ok, "hist2d n=%d nb=%d: outside, the total, the row and column sums", n, nb);
            // a column with itself: the diagonal only, equal to the 1-D counts
            std::vector<int64_t> h((size_t)nb);
            int64_t below, above;
            tmp_host_hist(x.data(), n, lox, hix, nb, h.data(), &below, &above);
            tmp_host_hist2d(x.data(), x.data(), n, lox, hix, lox, hix, nb, c.data(), &outside);
            ok = outside == below + above;
            for (int a = 0; a < nb; a++)
                for (int b = 0; b < nb; b++) ok = ok && c[(size_t)a * nb + b] == (a == b ? h[(size_t)a] : 0);
            CHECK(ok, "hist2d n=%d nb=%d: a column with itself", n, nb);
            checks += 2;
        }
    return checks;
}

// the interval by three passes over the widths
static void brute_hpd(const std::vector<double> &s, const long long k, long long *start)
{
    const long long n = (long long)s.size();
    bool any = false;
    double best = 0.0;
    for (long long i = 0; i + k <= n; i++) {
        volatile double w = s[(size_t)(i + k - 1)] - s[(size_t)i];
        if (std::isnan(w)) continue;
        if (!any || w < best) { best = w; any = true; }
    }
    *start = 0;
    if (!any) return;                                     // every width NaN: the first index
    for (long long i = 0; i + k <= n; i++) {
        volatile double w = s[(size_t)(i + k - 1)] - s[(size_t)i];
        if (w == best) { *start = i; return; }
    }
}

static long check_hpd(std::mt19937_64 &g)
{
    long checks = 0;
    std::normal_distribution<double> N(0.0, 1.0);
    // the window length
    CHECK(tmp_window(1.0 / 7, 7) == 1 && tmp_window(1.0, 7) == 7 && tmp_window(0.5, 7) == 4 && tmp_window(0.68, 100) == 68 && tmp_window(1e-300, 5) == 1 &&
          tmp_window(0.95, 20000) == 19000 && tmp_window(1.0, 1) == 1, "window lengths");
    for (const long long n : {4LL, 5LL, 100LL, 8193LL}) CHECK(tmp_window(1.0 / (double)n, n) >= 1 && tmp_window(1.0 / (double)n, n) <= 2 && tmp_window(1.0, n) == n, "window at 1 / n");
    CHECK(tmp_mass_ok(1.0) && tmp_mass_ok(1e-300) && !tmp_mass_ok(0.0) && !tmp_mass_ok(-0.5) && !tmp_mass_ok(1.0000001) && !tmp_mass_ok(NAN), "masses");
    // the order: total over widths with NaN, +-inf, ties
    const double W[] = {0.0, 1.0, 1.0, INF, NAN, NAN, 5e-324, 0.0};
    const int nw = 8;
    for (int a = 0; a < nw; a++)
        for (int b = 0; b < nw; b++) {
            const bool ab = tmp_before(W[a], a, W[b], b), ba = tmp_before(W[b], b, W[a], a);
            CHECK(a == b ? (!ab && !ba) : (ab != ba), "order: antisymmetry at (%d, %d)", a, b);
            for (int c = 0; c < nw; c++)
                if (ab && tmp_before(W[b], b, W[c], c)) CHECK(tmp_before(W[a], a, W[c], c), "order: transitivity at (%d, %d, %d)", a, b, c);
            checks++;
        }
    CHECK(tmp_before(INF, 9, NAN, 0) && !tmp_before(NAN, 0, INF, 9) && tmp_before(1.0, 2, 1.0, 3) && tmp_before(0.5, 9, 1.0, 0) && tmp_before(NAN, 1, NAN, 2), "order: the rule");
    for (int kind = 0; kind < 8; kind++)
        for (const int n : {1, 2, 4, 5, 63, 500}) {
            std::vector<double> v((size_t)n);
            switch (kind) {
            case 0: for (auto &x : v) x = 100.0 + N(g); break;
            case 1: for (auto &x : v) x = std::floor(3.0 * N(g)); break;                            // integers: many tied widths
            case 2: for (size_t i = 0; i < v.size(); i++) v[i] = (i & 1) ? 0.0 : -0.0; break;         // +-0: one value, returned as +0
            case 3: for (auto &x : v) x = 7.25; break;                                              // all equal: start 0, width 0
            case 4: for (auto &x : v) x = std::fabs(N(g)); break;                                   // one-sided
            case 5: for (size_t i = 0; i < v.size(); i++) v[i] = i % 3 == 0 ? INF : (i % 3 == 1 ? -INF : N(g)); break;   // inf - inf widths
            case 6: for (auto &x : v) x = INF; break;                                               // every width NaN
            default: for (size_t i = 0; i < v.size(); i++) v[i] = (double)(i / 2); break;           // every value twice
            }
            const std::vector<uint64_t> keys = tmp_host_sorted(v.data(), n);
            std::vector<double> s((size_t)n);
            for (int t = 0; t < n; t++) s[(size_t)t] = tmq_unkey(keys[(size_t)t]);
            std::vector<double> ref = v;
            for (auto &x : ref) x = x + 0.0;
            std::sort(ref.begin(), ref.end());
            bool ok = true;
            for (int t = 0; t < n; t++) ok = ok && same_bits(s[(size_t)t], ref[(size_t)t]);
            CHECK(ok, "kind %d n=%d: the sorted keys are the sorted values, -0 as +0", kind, n);
            for (const long long k : {1LL, 2LL, (long long)tmp_window(0.5, n), (long long)tmp_window(0.68, n), (long long)n - 1, (long long)n}) {
                if (k < 1 || k > n) continue;
                int64_t start;
                double lo, hi;
                tmp_host_hpd(keys.data(), n, k, &start, &lo, &hi);
                long long want;
                brute_hpd(s, k, &want);
                CHECK(start == want && same_bits(lo, s[(size_t)want]) && same_bits(hi, s[(size_t)(want + k - 1)]), "kind %d n=%d k=%lld: start %lld, want %lld",
                      kind, n, k, (long long)start, want);
                if (k == n) CHECK(start == 0 && same_bits(lo, s[0]) && same_bits(hi, s[(size_t)n - 1]), "k = n is min ... max");
                if (kind == 3) CHECK(start == 0 && lo == 7.25 && hi == 7.25, "all equal");
                // the kernel's shape: strided owners that all start from i = 0, reduced in pairs from the far end
                for (const int T : {1, 3, 64, 256}) {
                    std::vector<double> bw((size_t)T, tmp_width(keys.data(), 0, k));
                    std::vector<long long> bi((size_t)T, 0);
                    for (int tid = 0; tid < T; tid++)
                        for (long long i = tid; i + k <= n; i += T) {
                            const double w = tmp_width(keys.data(), i, k);
                            if (tmp_before(w, i, bw[(size_t)tid], bi[(size_t)tid])) { bw[(size_t)tid] = w; bi[(size_t)tid] = i; }
                        }
                    for (int d = T; d > 1; d = (d + 1) / 2)
                        for (int tid = 0; tid + (d + 1) / 2 < d; tid++) {
                            const int o = tid + (d + 1) / 2;
                            if (tmp_before(bw[(size_t)o], bi[(size_t)o], bw[(size_t)tid], bi[(size_t)tid])) { bw[(size_t)tid] = bw[(size_t)o]; bi[(size_t)tid] = bi[(size_t)o]; }
                        }
                    CHECK(bi[0] == want, "kind %d n=%d k=%lld: %d owners give start %lld, want %lld", kind, n, k, T, bi[0], want);
                }
                checks += 5;
            }
        }
    return checks;
}

static int64_t brute_level(const std::vector<int64_t> &c, const int64_t n_in, const double mass)
{
    if (n_in <= 0) return 0;
    const int64_t need = (int64_t)std::ceil(mass * (double)n_in);
    for (int64_t t = *std::max_element(c.begin(), c.end()); t >= 1; t--) {
        int64_t sum = 0;
        for (const int64_t x : c) sum += x >= t ? x : 0;
        if (sum >= need) return t;
    }
    return 0;
}

static long check_level(std::mt19937_64 &g)
{
    long checks = 0;
    std::vector<std::vector<int64_t>> cases = {{0, 0, 0, 0}, {5}, {3, 3, 3, 1}, {10, 0, 0, 0}, {4, 4, 2, 2, 1, 1, 0}, {1, 1, 1, 1, 1, 1, 1, 1}};
    for (int r = 0; r < 20; r++) {
        std::vector<int64_t> c(64);
        for (auto &x : c) x = (int64_t)(g() % 12);
        cases.push_back(c);
    }
    for (const auto &c : cases) {
        int64_t n_in = 0;
        for (const int64_t x : c) n_in += x;
        const std::vector<int64_t> desc = tmp_sorted_counts(c.data(), c.size());
        int64_t prev = -1;
        for (const double m : {1e-9, 0.3, 0.5, 0.68, 0.95, 1.0}) {
            const int64_t got = tmp_level(desc, n_in, m), want = brute_level(c, n_in, m);
            CHECK(got == want, "level mass %g: %lld, want %lld", m, (long long)got, (long long)want);
            if (prev >= 0) CHECK(got <= prev, "levels do not increase with the mass");
            prev = got;
            checks++;
        }
    }
    // the tie: {3, 3, 3, 1}, n_in = 10: 0.3 needs 3 samples and 0.9 needs 9, both level 3; 0.95 needs 10: level 1
    const std::vector<int64_t> tie = {3, 3, 3, 1}, d = tmp_sorted_counts(tie.data(), 4);
    CHECK(tmp_level(d, 10, 0.3) == 3 && tmp_level(d, 10, 0.9) == 3 && tmp_level(d, 10, 0.95) == 1 && tmp_level(d, 10, 1.0) == 1 && tmp_level(d, 0, 0.5) == 0, "the level tie");
    return checks + 1;
}

int main()
{
    std::mt19937_64 g(20240611);
    const long h = check_hist(g), p = check_hist2d(g), q = check_hpd(g), l = check_level(g);
    CHECK(tmp_hpd_col_bytes(8192, 2) == 8192 * 8 + 4 + 48, "bytes of a column");
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok modepdf_core_check: %ld histogram, %ld pair, %ld interval, %ld level checks\n", h, p, q, l);
    return 0;
}
