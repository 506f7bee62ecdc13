// moderank_core_check.cpp -- the arithmetic of tamcmc_moderank.h on the CPU (plain g++, no GPU, no library):
//   * the sort kernel's walk -- tiles of TM_MR_TILE keys, the stages inside a tile and the wide stages on the whole column,
//     comparator by comparator and thread by thread -- against std::sort of the keys: n = 4 ... 130, both sides of every
//     power of two up to 4096, every 97th n up to 5000, 5000, and both sides of TM_MR_TILE, 2 TM_MR_TILE and 4 TM_MR_TILE (one, two and three wide
//     stages); columns with ties, +-0, all values equal, and key ranges of 0, 1, 31, 32, 33 and 64 bits;
//   * rank2 by the two binary searches against the counts of the definition; its sum n (n + 1);
//   * z: antisymmetric bit for bit, +0 at rank2 = n + 1, strictly increasing over distinct rank2, and within
//     10 2^-50 q / phi(z) + 4 2^-52 |z| of the exact value, checked in long double through erfcl as |Q(z) - q| <= phi(z) bound;
//   * median, fold, indicators, the NaN-skipping minimum and maximum, the totals, the byte count of a column.
// Prints "ok moderank_core_check ..." and exits 0, or says what failed and exits 1.  May be built with
// -fsanitize=address,undefined and run as it is.
#define TMR_HOST_FEED
#include "tamcmc_moderank.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static bool same_bits(const double a, const double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// a column of n values of one kind
static std::vector<double> column(const int kind, const long long n, std::mt19937_64 &g)
{
    std::vector<double> v((size_t)n);
    std::normal_distribution<double> N(0.0, 1.0);
    const uint64_t k1 = tmq_key(1.0);
    auto spread = [&](const uint64_t R) { for (auto &x : v) x = tmq_unkey(k1 + (R == ~(uint64_t)0 ? g() : g() % (R + 1))); };
    switch (kind) {
    case 0: for (auto &x : v) x = 3000.0 + N(g); break;                                   // distinct
    case 1: for (auto &x : v) x = std::floor(4.0 * N(g)); break;                          // massive ties, -0 never, +0 often
    case 2: for (size_t i = 0; i < v.size(); i++) v[i] = (g() & 1) ? 0.0 : -0.0; break;     // +-0: one key
    case 3: for (auto &x : v) x = 7.25; break;                                            // all equal: 0 bits
    case 4: spread(1); break;                                                             // 1 bit
    case 5: spread(((uint64_t)1 << 31) - 1); break;                                       // 31 bits
    case 6: spread(((uint64_t)1 << 32) - 1); break;                                       // 32 bits
    case 7: spread(((uint64_t)1 << 33) - 1); break;                                       // 33 bits
    case 8: for (auto &x : v) x = ((g() & 1) ? 1.0 : -1.0) * std::exp(200.0 * N(g)); v[0] = -1e300; v[1] = 1e300; break;   // 64 bits
    default: for (size_t i = 0; i < v.size(); i++) v[i] = (i % 3 == 0) ? -0.0 : ((i % 3 == 1) ? 0.0 : N(g)); break;       // zeros among values
    }
    return v;
}
static const int want_bits[] = {-1, -1, 0, 0, 1, 31, 32, 33, 64, -1};

static long check_column(const std::vector<double> &v, const int kind, const bool ranks)
{
    const long long n = (long long)v.size(), P = tmr_padded(n);
    CHECK(P >= n && P >= 2 && (P & (P - 1)) == 0 && (P == 2 || P / 2 < n), "padded(%lld) = %lld", n, P);
    std::vector<uint64_t> keys((size_t)P, ~(uint64_t)0), want((size_t)n);
    for (long long t = 0; t < n; t++) keys[(size_t)t] = want[(size_t)t] = tmq_key(v[(size_t)t]);
    std::sort(want.begin(), want.end());
    if (want_bits[kind] >= 0 && n >= 64) CHECK(tmq_bit_length(want.back() - want.front()) == want_bits[kind], "kind %d: %d bits", kind, tmq_bit_length(want.back() - want.front()));
    tmr_host_sort(keys.data(), P, TM_MR_SORT_THREADS);
    bool ok = true;
    for (long long t = 0; t < n; t++) ok = ok && keys[(size_t)t] == want[(size_t)t];
    for (long long t = n; t < P; t++) ok = ok && keys[(size_t)t] == ~(uint64_t)0;
    CHECK(ok, "sort: kind %d n %lld", kind, n);
    if (!ranks) return 1;
    long long sum = 0;
    for (long long t = 0; t < n; t++) {
        const uint64_t key = tmq_key(v[(size_t)t]);
        long long lb, ub;
        tmr_bounds(keys.data(), n, key, &lb, &ub);
        const long long wl = std::lower_bound(want.begin(), want.end(), key) - want.begin(), wu = std::upper_bound(want.begin(), want.end(), key) - want.begin();
        CHECK(lb == wl && ub == wu, "bounds: kind %d n %lld t %lld: %lld %lld, want %lld %lld", kind, n, t, lb, ub, wl, wu);
        if (n <= 130) {
            long long less = 0, leq = 0;
            for (long long s = 0; s < n; s++) { less += tmq_key(v[(size_t)s]) < key; leq += tmq_key(v[(size_t)s]) <= key; }
            CHECK(lb == less && ub == leq, "counts: kind %d n %lld t %lld", kind, n, t);
        }
        const long long r2 = tmr_rank2(keys.data(), n, key);
        CHECK(r2 == lb + ub + 1 && r2 >= 2 && r2 <= 2 * n, "rank2 %lld", r2);
        sum += r2;
    }
    CHECK(sum == n * (n + 1), "kind %d n %lld: sum of rank2 %lld", kind, n, sum);
    // median, fold, indicators on this column
    const double med = tmr_median(keys.data(), n);
    std::vector<double> s(v);
    for (auto &x : s) x = x + 0.0;
    std::sort(s.begin(), s.end());
    CHECK(same_bits(med, 0.5 * s[(size_t)((n - 1) / 2)] + 0.5 * s[(size_t)(n / 2)]), "median kind %d n %lld", kind, n);
    if (kind == 3) CHECK(tmr_rank2(keys.data(), n, tmq_key(v[0])) == n + 1 && same_bits(tmr_z(n + 1, n), 0.0) && same_bits(tmr_fold(v[0], med), 0.0), "constant column");
    return 1;
}

static long check_z(const long long n, const long long step)
{
    const long long D = 8 * n + 2;
    double prev = -INFINITY;
    long cnt = 0;
    for (long long r2 = 2; r2 <= 2 * n; r2 += (r2 < 400 || r2 > 2 * n - 400 || (r2 > n - 200 && r2 < n + 200)) ? 1 : step) {
        const double z = tmr_z(r2, n), zm = tmr_z(2 * (n + 1) - r2, n);
        CHECK(same_bits(z, -zm) || (r2 == n + 1 && same_bits(z, 0.0) && same_bits(zm, 0.0)), "antisymmetry n %lld rank2 %lld: %a %a", n, r2, z, zm);
        CHECK(z > prev, "monotone n %lld rank2 %lld: %a after %a", n, r2, z, prev);
        prev = z;
        if (r2 == n + 1) CHECK(same_bits(z, 0.0), "+0 at the middle, n %lld", n);
        const long long a = 4 * r2 - 3, m = a < D - a ? a : D - a;
        if (m != D - m) {
            const long double q = (long double)m / (long double)D, g = fabsl((long double)z);
            const long double Q = 0.5L * erfcl(g * 0.70710678118654752440084436210485L), phi = 0.39894228040143267793994605993438L * expl(-0.5L * g * g);
            const long double bound = 10.0L * ldexpl(1.0L, -50) * q / phi + 4.0L * ldexpl(1.0L, -52) * g;
            CHECK(fabsl(Q - q) <= phi * bound, "accuracy n %lld rank2 %lld: |Q - q| %Lg, allowed %Lg", n, r2, fabsl(Q - q), phi * bound);
            CHECK((a < D - a) == (z < 0.0), "sign n %lld rank2 %lld", n, r2);
        }
        cnt++;
    }
    return cnt;
}

int main()
{
    static_assert((TM_MR_TILE & (TM_MR_TILE - 1)) == 0 && TM_MR_TILE >= 2 && TM_MR_LDS_BYTES == 65536 && TM_MR_LDS_BYTES <= 160 * 1024, "sort kernel LDS");
    static_assert(TM_MR_NOUT == 8 && TM_MR_NSERIES == 4 && sizeof(TmrTotals) == 88, "ABI");
    std::mt19937_64 g(20260421);
    long cols = 0, zs = 0;
    std::vector<long long> sizes;
    for (long long n = 4; n <= 130; n++) sizes.push_back(n);
    for (long long p = 256; p <= 4096; p <<= 1) { sizes.push_back(p - 1); sizes.push_back(p); sizes.push_back(p + 1); }
    sizes.push_back(5000);
    for (long long n = 131; n < 5000; n += 97) sizes.push_back(n);
    for (long long n : sizes)
        for (int kind = 0; kind < 10; kind++) cols += check_column(column(kind, n, g), kind, true);
    for (long long p = TM_MR_TILE; p <= 4 * TM_MR_TILE; p <<= 1)
        for (long long n : {p - 1, p, p + 1})
            for (int kind : {0, 1, 8}) cols += check_column(column(kind, n, g), kind, n == p + 1 && kind == 1);
    for (long long n : {4LL, 5LL, 63LL, 64LL, 65LL, 1023LL, 1024LL, 2049LL, 4000LL}) zs += check_z(n, 1);
    zs += check_z(70001, 97);
    zs += check_z(((long long)1 << 31) - 1, 1000003LL * 4099);
    // g at the ends of its domain and around the switch of its start
    for (double q : {1e-300, 1e-12, 0.02424999, 0.02425, 0.02425001, 0.25, 0.4999999, 0.49999999999999994}) {
        const long double g1 = tmr_g(q), Q = 0.5L * erfcl(g1 * 0.70710678118654752440084436210485L), phi = 0.39894228040143267793994605993438L * expl(-0.5L * g1 * g1);
        CHECK(g1 > 0 && fabsl(Q - (long double)q) <= phi * (10.0L * ldexpl(1.0L, -50) * q / phi + 4.0L * ldexpl(1.0L, -52) * g1), "g(%g) = %Lg", q, g1);
    }
    // the NaN-skipping pair rules and the totals
    const double nan = NAN;
    CHECK(tmr_min_skip(3.0, 2.0) == 2.0 && tmr_min_skip(nan, 2.0) == 2.0 && tmr_min_skip(3.0, nan) == 3.0 && std::isnan(tmr_min_skip(nan, nan)), "min_skip");
    CHECK(tmr_max_skip(3.0, 2.0) == 3.0 && tmr_max_skip(nan, 2.0) == 2.0 && tmr_max_skip(3.0, nan) == 3.0 && std::isnan(tmr_max_skip(nan, nan)), "max_skip");
    {
        const double eb[5] = {nan, 50.0, 20.0, 20.0, 70.0}, et[5] = {nan, 9.0, nan, 8.0, 8.0}, rh[5] = {nan, 1.02, 1.2, 1.2, 1.0};
        const int32_t cut[5] = {0, 16, 4, 16, 2}, sel[5] = {9, 7, 5, 3, 1};
        const double a0[5] = {0.0, 1.0, 2.0, 3.0, 0.0};
        const TmrTotals t = tmr_totals(5, sel, 100, 15, eb, et, rh, cut, a0);
        CHECK(t.n_used == 100 && t.lag == 15 && t.min_ess_bulk == 20.0 && t.col_min_ess_bulk == 5 && t.min_ess_tail == 8.0 && t.col_min_ess_tail == 3 &&
              t.max_rhat == 1.2 && t.col_max_rhat == 5 && t.n_truncated == 2 && t.n_constant == 2 && t.n_rhat_high == 3, "totals");
        const TmrTotals u = tmr_totals(1, nullptr, 100, 15, eb, et, rh, cut, a0);
        CHECK(std::isnan(u.min_ess_bulk) && std::isnan(u.min_ess_tail) && std::isnan(u.max_rhat) && u.col_min_ess_bulk == -1 && u.col_min_ess_tail == -1 &&
              u.col_max_rhat == -1 && u.n_constant == 1 && u.n_truncated == 0 && u.n_rhat_high == 0, "totals of NaN");
    }
    CHECK(tmr_col_bytes(1100, 255) == 16 * 2048 + 32 * (1100 + 255 + 5) + 44 && tmr_col_bytes(4, 3) == 16 * 4 + 32 * 12 + 44, "col bytes");
    CHECK(same_bits(tmr_indicator(-0.0, 0.0), 1.0) && same_bits(tmr_indicator(1.0, 0.0), 0.0) && same_bits(tmr_fold(-3.0, 1.0), 4.0), "indicator, fold");
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok moderank_core_check: %ld columns sorted and ranked, %ld z values\n", cols, zs);
    return 0;
}
