// quantile_core_check -- the per-bin arithmetic of the quantile selection (tamcmc-c-_amd/csrc/tamcmc_quantile.h) on the
// CPU, with the header's own functions: the key map, and whole multi-pass selections against a sort.
//   g++ -std=c++17 -O1 -I tamcmc-c-_amd/csrc tests/cpp/quantile_core_check.cpp -o quantile_core_check && ./quantile_core_check
// Prints one `ok` line; any failure prints what failed and exits 1.  (tests/test_summary_quantiles_host.py builds and runs
// it; with -fsanitize=address,undefined it is the check that no shift is by 64 or more.)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "tamcmc_quantile.h"

static int failures = 0;
#define CHECK(cond, ...)                                                            \
    do {                                                                            \
        if (!(cond)) {                                                              \
            if (failures++ < 20) { fprintf(stderr, "FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
        }                                                                           \
    } while (0)

static uint64_t bits_of(double v) { uint64_t u; memcpy(&u, &v, sizeof(u)); return u; }

static long check_keys()
{
    const double inf = std::numeric_limits<double>::infinity(), den = std::numeric_limits<double>::denorm_min();
    // sorted; -0 and +0 are neighbours and must get one key
    const double v[] = {-inf, -1.7976931348623157e308, -2.0000000000000004, -2.0, -1.9999999999999998, -1.0, -2.2250738585072014e-308, -den,
                        -0.0, 0.0, den, 2.2250738585072014e-308, 0.5, 1.0, 1.9999999999999998, 2.0, 2.0000000000000004,
                        4.0 - 8.881784197001252e-16, 4.0, 1.7976931348623157e308, inf};
    const size_t n = sizeof(v) / sizeof(v[0]);
    long checked = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t k = tmq_key(v[i]);
        const double back = tmq_unkey(k);
        CHECK(back == v[i], "round trip of %a gives %a", v[i], back);
        if (v[i] != 0.0) CHECK(bits_of(back) == bits_of(v[i]), "round trip bits of %a", v[i]);
        else CHECK(bits_of(back) == 0, "the inverse of key(+-0) must be +0");
        if (i + 1 < n) {
            const uint64_t k1 = tmq_key(v[i + 1]);
            if (v[i] == v[i + 1]) CHECK(k == k1, "-0 and +0 must share a key");
            else CHECK(k < k1, "key not strictly monotone between %a and %a", v[i], v[i + 1]);
        }
        checked++;
    }
    // neighbours in key space are neighbours as doubles
    CHECK(tmq_unkey(tmq_key(2.0) - 1) == 1.9999999999999998 && tmq_unkey(tmq_key(2.0) + 1) == 2.0000000000000004, "neighbours of 2.0");
    // (the key that the bits of -0 would map to is never produced: -0 is folded into +0 first)
    CHECK(tmq_key(0.0) - tmq_key(-den) == 2 && tmq_key(den) - tmq_key(0.0) == 1, "neighbours of 0");
    CHECK(tmq_bit_length(0) == 0 && tmq_bit_length(1) == 1 && tmq_bit_length(255) == 8 && tmq_bit_length(256) == 9 &&
              tmq_bit_length(~(uint64_t)0) == 64, "bit_length");
    CHECK(tmq_rank(0.0, 37) == 0 && tmq_rank(1.0, 37) == 36 && tmq_rank(0.5, 37) == 18 && tmq_rank(0.5, 2) == 0 && tmq_rank(0.16, 37) == 5 &&
              tmq_rank(0.5, 1) == 0, "rank rule");
    return checked;
}

// One column, every rank, bits 1 ... 6: the histogram is filled and narrowed with the header's functions.  Every pass's
// bracket must contain the sorted answer and the final prefix must equal it.
static long check_column(const char *name, const std::vector<double> &col)
{
    const size_t n = col.size();
    std::vector<uint64_t> keys(n);
    for (size_t s = 0; s < n; s++) keys[s] = tmq_key(col[s]);
    std::vector<uint64_t> sorted = keys;
    std::sort(sorted.begin(), sorted.end());
    const uint64_t kmin = sorted.front(), R = sorted.back() - kmin;
    const int u0 = tmq_bit_length(R);
    long selections = 0;
    for (int bits = 1; bits <= TM_Q_MAXBITS; bits++)
        for (size_t k = 0; k < n; k++) {
            uint64_t prefix = 0, below = 0;
            int u = u0, passes = 0;
            uint32_t hist[1 << TM_Q_MAXBITS] = {};
            const uint64_t want = sorted[k] - kmin;
            uint64_t lo, hi, plo = 0, phi = R;
            tmq_bracket(prefix, u, R, &lo, &hi);
            CHECK(lo == 0 && hi == R, "%s: the first bracket must be the envelope", name);
            while (u > 0) {
                const int d = tmq_digits(u, bits);
                for (size_t s = 0; s < n; s++) {
                    const uint64_t D = keys[s] - kmin;
                    unsigned cell;
                    if (D <= R && tmq_match(D, prefix, u, d, &cell)) hist[cell]++;
                }
                tmq_narrow(&prefix, &below, (uint64_t)k, hist, 1, d);
                u -= d;
                passes++;
                tmq_bracket(prefix, u, R, &lo, &hi);
                CHECK(lo <= want && want <= hi, "%s bits %d rank %zu pass %d: the bracket lost the answer", name, bits, k, passes);
                CHECK(lo >= plo && hi <= phi, "%s bits %d rank %zu pass %d: the bracket grew", name, bits, k, passes);
                plo = lo; phi = hi;
                for (int c = 0; c < (1 << TM_Q_MAXBITS); c++) CHECK(hist[c] == 0, "%s: narrow left a cell uncleared", name);
            }
            CHECK(passes == (u0 + bits - 1) / bits, "%s bits %d: %d passes for %d bits", name, bits, passes, u0);
            CHECK(prefix == want && lo == want && hi == want, "%s bits %d rank %zu: final prefix is not the order statistic", name, bits, k);
            CHECK(tmq_key(tmq_unkey(kmin + prefix)) == sorted[k], "%s bits %d rank %zu: value", name, bits, k);
            selections++;
        }
    return selections;
}

// tmq_narrow<uint32_t> on cells that hold 65 535, 65 536 and 4 294 967 295 counts -- past the 16-bit LDS counters of the
// histogram kernel and at the end of the global uint32 cells -- with the wanted rank first and last in such a cell.  The
// cumulative counts are uint64: three full cells sum to 3 (2^32 - 1), which a 32-bit running sum would wrap.
static long check_big_cells()
{
    long cases = 0;
    const uint64_t bigs[] = {65535u, 65536u, 4294967295u};
    for (const uint64_t big : bigs)
        for (int d = 1; d <= TM_Q_MAXBITS; d++) {
            const unsigned ncell = 1u << d;
            // the big cell at c0, a few small ones around it, and (where there is room) big cells under it too
            for (const unsigned c0 : {0u, ncell / 2, ncell - 1})
                for (int full_below = 0; full_below < 2; full_below++) {
                    std::vector<uint32_t> cells(ncell);
                    for (unsigned c = 0; c < ncell; c++) cells[c] = (c % 3 == 0) ? 0u : (c % 3 == 1 ? 1u : 7u);
                    if (full_below)
                        for (unsigned c = 0; c < c0 && c < 3; c++) cells[c] = (uint32_t)big;
                    cells[c0] = (uint32_t)big;
                    uint64_t under = 0;
                    for (unsigned c = 0; c < c0; c++) under += cells[c];
                    if (full_below && c0 >= 2) CHECK(big < 4294967295u || under > 0xFFFFFFFFull, "the cells under the big one must pass 2^32");
                    const uint64_t below0 = 12345678901ull, prefix0 = 5;
                    for (const uint64_t within : {(uint64_t)0, big - 1}) {            // first and last rank of the big cell
                        std::vector<uint32_t> h = cells;
                        uint64_t prefix = prefix0, below = below0;
                        tmq_narrow<uint32_t>(&prefix, &below, below0 + under + within, h.data(), 1, d);
                        CHECK(prefix == ((prefix0 << d) | c0), "big %llu d %d cell %u rank +%llu: digit %llu", (unsigned long long)big, d, c0,
                              (unsigned long long)within, (unsigned long long)(prefix & (ncell - 1)));
                        CHECK(below == below0 + under, "big %llu d %d cell %u rank +%llu: below off by %lld", (unsigned long long)big, d, c0,
                              (unsigned long long)within, (long long)(below - below0 - under));
                        for (unsigned c = 0; c < ncell; c++) CHECK(h[c] == 0, "narrow left a cell uncleared");
                        cases++;
                    }
                    // the rank just past the big cell belongs to the next cell that holds anything (or, none left, the top cell)
                    {
                        std::vector<uint32_t> h = cells;
                        uint64_t prefix = prefix0, below = below0;
                        tmq_narrow<uint32_t>(&prefix, &below, below0 + under + big, h.data(), 1, d);
                        unsigned next = c0 + 1;
                        uint64_t u2 = under + big;
                        while (next < ncell && cells[next] == 0) next++;
                        if (next < ncell) {
                            CHECK(prefix == ((prefix0 << d) | next) && below == below0 + u2, "big %llu d %d cell %u: the rank past it", (unsigned long long)big, d, c0);
                        } else {
                            CHECK(prefix == ((prefix0 << d) | (ncell - 1)) && below == below0, "big %llu d %d cell %u: a rank no cell holds", (unsigned long long)big, d, c0);
                        }
                        cases++;
                    }
                }
        }
    return cases;
}

int main()
{
    const long nkeys = check_keys();
    const long nbig = check_big_cells();
    const double inf = std::numeric_limits<double>::infinity(), den = std::numeric_limits<double>::denorm_min();
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto uniform = [&]() {                                    // xorshift64*: [0, 1)
        rng ^= rng >> 12; rng ^= rng << 25; rng ^= rng >> 27;
        return (double)((rng * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
    };
    long sel = 0;
    for (size_t n : {(size_t)1, (size_t)2, (size_t)50, (size_t)300}) {
        std::vector<double> c(n);
        for (auto &v : c) v = 1.0 + 3.0 * uniform();                       // random, positive, across 2.0
        sel += check_column("random", c);
        for (auto &v : c) v = (double)(int)(4.0 * uniform());              // heavy ties
        sel += check_column("ties", c);
        for (auto &v : c) v = 0.1;                                         // all equal: 0 passes
        sel += check_column("equal", c);
        for (auto &v : c) v = (uniform() - 0.5) * std::exp(40.0 * (uniform() - 0.5));      // mixed sign, many binades
        sel += check_column("mixed-sign", c);
    }
    sel += check_column("special", {-inf, -3.5, -den, -0.0, 0.0, 0.0, den, 1.9999999999999998, 2.0, 2.0, inf});
    sel += check_column("zeros", {0.0, -0.0, -0.0, 0.0});
    sel += check_column("straddle-2", {1.9999999999999998, 2.0000000000000004});
    sel += check_column("full-range", {-inf, inf});                        // R needs all 64 bits
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok quantile_core_check: %ld key values, %ld selections, %ld narrowings of cells of 65535 ... 2^32 - 1 counts\n", nkeys, sel, nbig);
    return 0;
}
