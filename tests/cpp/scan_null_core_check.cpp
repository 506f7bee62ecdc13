// scan_null_core_check.cpp -- the generator, the combine rule and the calibration of tamcmc_scan_null.h on the CPU, plain g++
// (-std=c++17 -O1 -ffp-contract=off; `make scan-null-core-check CHECKFLAGS=-fsanitize=address,undefined` for a sanitizer
// build): the three published Philox4x32-10 known answers, the uniform mapping at its two ends, the variate's use of the
// calls, the tile-combine rule on hand-made partials with ties, and the calibration counts on hand-made and random m with
// ties against a brute-force restatement, with the invariants ceil(j / K) <= c <= j (without ties) and joint line <=
// per-width line.  Prints one line, "ok scan_null_core_check ...", or what failed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "tamcmc_scan_null.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static bool philox_is(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    uint32_t w[4];
    tmn_philox(c0, c1, c2, c3, k0, k1, w);
    return w[0] == a && w[1] == b && w[2] == c && w[3] == d;
}

// the definition, count by count
struct Brute {
    long long R;
    int K;
    std::vector<std::vector<double>> m;      // [k][r]
    std::vector<long long> vmin;
    explicit Brute(const std::vector<std::vector<double>> &m_) : R((long long)m_[0].size()), K((int)m_.size()), m(m_), vmin((size_t)R)
    {
        for (long long r = 0; r < R; r++) {
            long long v = R;
            for (int k = 0; k < K; k++) {
                long long c = 0;
                for (long long q = 0; q < R; q++) c += m[k][(size_t)q] <= m[k][(size_t)r] ? 1 : 0;
                v = c < v ? c : v;
            }
            vmin[(size_t)r] = v;
        }
    }
    long long n_le(int k, double v) const { long long n = 0; for (double x : m[k]) n += x <= v ? 1 : 0; return n; }
    long long vmin_le(long long n) const { long long c = 0; for (long long x : vmin) c += x <= n ? 1 : 0; return c; }
    // the i-th smallest (1-based) by counting: the smallest x with #{<= x} >= i
    double smallest(int k, long long i) const
    {
        double best = INFINITY;
        for (double x : m[k]) if (n_le(k, x) >= i && x < best) best = x;
        return best;
    }
    long long smallest_vmin(long long i) const
    {
        long long best = R + 1;
        for (long long x : vmin) if (vmin_le(x) >= i && x < best) best = x;
        return best;
    }
};

static void check_calibration(const std::vector<std::vector<double>> &m, const bool ties)
{
    const int K = (int)m.size();
    const long long R = (long long)m[0].size();
    TmNullCalib c;
    c.build(K, R, m.data());
    const Brute b(m);
    for (const double alpha : {0.01, 0.05, 0.1, 0.5, 0.99}) {
        const double jd = floor(alpha * (double)(R + 1));
        const long long j = c.rank(alpha);
        CHECK(j == (jd >= 1.0 && jd <= (double)R ? (long long)jd : 0));
        if (j < 1) continue;
        const long long cj = c.line_rank(j, true);
        CHECK(cj == b.smallest_vmin(j));
        CHECK(cj >= 1 && cj <= R);
        if (!ties) CHECK((j + K - 1) / K <= cj && cj <= j);
        for (int k = 0; k < K; k++) {
            CHECK(c.line(k, j, false) == b.smallest(k, j));
            CHECK(c.line(k, j, true) == b.smallest(k, cj));
            CHECK(c.line(k, j, true) <= c.line(k, j, false));
        }
    }
    CHECK(c.rank(0.0) == 0 && c.rank(-1.0) == 0 && c.rank(1.0) == 0 && c.rank(NAN) == 0 && c.rank(0.5 / (double)(R + 1)) == 0);
    for (int k = 0; k < K; k++) {
        std::vector<double> probe(m[k]);
        probe.push_back(-INFINITY); probe.push_back(INFINITY); probe.push_back(m[k][0] - 0.5); probe.push_back(m[k][0] + 1e-9);
        for (const double v : probe) {
            double pw, pj;
            c.pvalue(k, v, &pw, &pj);
            const long long n = b.n_le(k, v);
            CHECK(pw == (double)(1 + n) / (double)(R + 1));
            CHECK(pj == (double)(1 + b.vmin_le(n)) / (double)(R + 1));
            CHECK(pj >= pw && pj <= 1.0 && pw >= 1.0 / (double)(R + 1));
        }
    }
}

int main()
{
    // 1. known answers (Random123's kat_vectors: philox4x32 10)
    CHECK(philox_is(0, 0, 0, 0, 0, 0, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u));
    CHECK(philox_is(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu));
    CHECK(philox_is(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u));

    // 2. the uniform: exact, strictly inside (0, 1), the low 12 bits of the second word unused
    CHECK(tmn_uniform(0u, 0u) == 0x1p-53 && tmn_uniform(0u, 0u) > 0.0);
    CHECK(tmn_uniform(0xFFFFFFFFu, 0xFFFFFFFFu) == 1.0 - 0x1p-53 && tmn_uniform(0xFFFFFFFFu, 0xFFFFFFFFu) < 1.0);
    CHECK(tmn_uniform(0u, 0xFFFu) == tmn_uniform(0u, 0u) && tmn_uniform(0u, 0x1000u) == 0x1p-52 + 0x1p-53);
    CHECK(tmn_uniform(0x80000000u, 0u) == 0.5 + 0x1p-53 && tmn_uniform(1u, 0u) == 0x1p-32 + 0x1p-53);
    {
        // counter = (bin, t, replicate low, replicate high), key = (seed low, seed high)
        const uint64_t seed = 0x299f31d0a4093822ull, rep = 0x0370734413198a2eull;
        double ue, uo;
        tmn_uniforms(seed, rep, 0x243f6a88u, 0x85a308d3u, &ue, &uo);
        CHECK(ue == tmn_uniform(0xd16cfe09u, 0x94fdccebu) && uo == tmn_uniform(0x5001e420u, 0x24126ea1u));
    }

    // 3. the variate: p terms from ceil(p / 2) calls in ascending k, one division; the Gaussian from call 0
    {
        const uint64_t seed = 3, rep = ((uint64_t)1 << 32) - 1;
        for (const int p : {1, 2, 3, 4, 7, 64}) {
            double z = 0.0;
            for (int k = 0; k < p; k++) {
                double ue, uo;
                tmn_uniforms(seed, rep, 11u, (uint32_t)(k >> 1), &ue, &uo);
                const double e = -log(k & 1 ? uo : ue);
                z = k == 0 ? e : z + e;
            }
            CHECK(tmn_variate(false, p, seed, rep, 11u) == z / (double)p);
        }
        double ue, uo;
        tmn_uniforms(seed, rep, 11u, 0u, &ue, &uo);
        CHECK(tmn_variate(true, 5, seed, rep, 11u) == sqrt(-log(ue)) * tmn_cospi(2.0 * uo));
        CHECK(tmn_variate(false, 1, seed, rep, 11u) != tmn_variate(false, 1, seed, rep + 1, 11u));
        CHECK(tmn_variate(false, 1, seed, rep, 11u) != tmn_variate(false, 1, seed, rep, 12u));
        CHECK(tmn_variate(false, 1, seed, rep, 11u) != tmn_variate(false, 1, seed + ((uint64_t)1 << 32), rep, 11u));
    }

    // 4. the combine rule: ties go to the lower position, a tile without a window (-1) never wins, in any order
    {
        CHECK(tmn_takes(true, 2.0, 5, 1.0, 3) && !tmn_takes(true, 1.0, 5, 2.0, 3) && !tmn_takes(true, 2.0, 5, 2.0, 3) && tmn_takes(true, 2.0, 2, 2.0, 3));
        CHECK(tmn_takes(false, 1.0, 5, 2.0, 3) && !tmn_takes(false, 2.0, 5, 1.0, 3) && !tmn_takes(false, 2.0, 5, 2.0, 3) && tmn_takes(false, 2.0, 2, 2.0, 3));
        CHECK(!tmn_takes(true, INFINITY, -1, 0.0, 3) && tmn_takes(true, -5.0, 7, -INFINITY, -1) && !tmn_takes(false, -INFINITY, -1, 0.0, 3));
        // three (width, side) columns interleaved with stride 3; column 0: a maximum with a tie, 1: a minimum with a tie and
        // an empty tile, 2: only the first tile has a window
        const double val[] = {1.0, 4.0, 9.0,   7.0, 2.0, -INFINITY,   7.0, 2.0, -INFINITY,   3.0, INFINITY, -INFINITY};
        const long long pos[] = {10, 11, 12,   2050, 2051, -1,   4100, 4101, -1,   6200, -1, -1};
        double v; long long at;
        tmn_combine(true, 4, 3, val + 0, pos + 0, &v, &at);  CHECK(v == 7.0 && at == 2050);
        tmn_combine(false, 4, 3, val + 1, pos + 1, &v, &at); CHECK(v == 2.0 && at == 2051);
        tmn_combine(true, 4, 3, val + 2, pos + 2, &v, &at);  CHECK(v == 9.0 && at == 12);
        tmn_combine(true, 1, 3, val + 0, pos + 0, &v, &at);  CHECK(v == 1.0 && at == 10);
        // the same partials handed over in the opposite order still give the lower position
        const double rval[] = {7.0, 7.0, 1.0};
        const long long rpos[] = {4100, 2050, 10};
        tmn_combine(true, 3, 1, rval, rpos, &v, &at);        CHECK(v == 7.0 && at == 2050);
    }

    // 5. layout arithmetic
    CHECK(tmn_tiles(2, 1) == 1 && tmn_tiles(2048, 1) == 1 && tmn_tiles(2049, 1) == 2 && tmn_tiles(2049, 2) == 1 && tmn_tiles(100000, 10) == 49);
    CHECK(tmn_chunk(1, 1) == TM_NULL_CHUNK_MAX && tmn_chunk(49, 8) == TM_NULL_CHUNK_MAX && tmn_chunk(1 << 20, 8) == 1 && tmn_chunk(1 << 16, 1) == 32);
    CHECK(TM_NULL_LDS_BYTES == 21248);
    for (const long long tiles : {1LL, 49LL, 1000LL, 1LL << 16, 1LL << 20})
        for (const int K : {1, 8}) {
            const long long c = tmn_chunk(tiles, K);
            CHECK(c >= 1 && (c == 1 || (c * tiles * K * 32 <= TM_NULL_PARTIAL_BYTES && c * tiles * TM_NULL_THREADS <= (1LL << 30))));
        }

    // the memory term 64 MiB / (32 K tiles) = 2^21 / (K tiles) at its edge with the cap of 4096: K tiles = 512, 513, and 520
    // (K = 8, 65 tiles: Nx = 131 073 with a narrowest width of 1)
    CHECK(tmn_chunk(64, 8) == 4096 && tmn_chunk(512, 1) == 4096 && tmn_chunk(513, 1) == 4088 && tmn_chunk(171, 3) == 4088 && tmn_chunk(65, 8) == 4032);
    CHECK(tmn_tiles(131072, 1) == 64 && tmn_tiles(131073, 1) == 65 && tmn_tiles(131073, 2) == 64);
    for (int K = 1; K <= 8; K++)
        for (long long tiles = 1; tiles <= 5000; tiles++) {
            const long long c = tmn_chunk(tiles, K);
            CHECK(c >= 1 && c <= TM_NULL_CHUNK_MAX && (c == TM_NULL_CHUNK_MAX) == (K * tiles <= 512));
            CHECK(c == 1 || 2 * K * tiles * 16 * c <= TM_NULL_PARTIAL_BYTES);
            CHECK(c == TM_NULL_CHUNK_MAX || 2 * K * tiles * 16 * (c + 1) > TM_NULL_PARTIAL_BYTES);        // (the 2^30-thread term is the larger one here)
        }

    // 6. the calibration by hand: R = 4, K = 2
    {
        //            r:   0     1     2     3
        const std::vector<std::vector<double>> m = {{-5.0, -1.0, -3.0, -2.0}, {-1.0, -6.0, -2.0, -2.0}};
        // cnt[.][0] = 1 4 2 3; cnt[.][1] = 4 1 3 3 (the tie counts both); vmin = 1 1 2 3
        TmNullCalib c;
        c.build(2, 4, m.data());
        CHECK(c.vmin == (std::vector<long long>{1, 1, 2, 3}));
        CHECK(c.rank(0.2) == 1 && c.rank(0.4) == 2 && c.rank(0.19) == 0 && c.rank(0.8) == 4 && c.rank(1.0) == 0);
        CHECK(c.line(0, 1, false) == -5.0 && c.line(0, 2, false) == -3.0 && c.line(1, 2, false) == -2.0 && c.line(1, 3, false) == -2.0);
        CHECK(c.line_rank(1, true) == 1 && c.line_rank(2, true) == 1 && c.line_rank(3, true) == 2 && c.line_rank(4, true) == 3);
        CHECK(c.line(0, 3, true) == -3.0 && c.line(1, 4, true) == -2.0);
        double pw, pj;
        c.pvalue(0, -3.0, &pw, &pj); CHECK(pw == 3.0 / 5.0 && pj == 4.0 / 5.0);        // n = 2: vmin <= 2 three times
        c.pvalue(1, -2.0, &pw, &pj); CHECK(pw == 4.0 / 5.0 && pj == 5.0 / 5.0);        // n = 3
        c.pvalue(1, -7.0, &pw, &pj); CHECK(pw == 1.0 / 5.0 && pj == 1.0 / 5.0);        // below everything
        check_calibration(m, true);
    }
    // random m: continuous (no ties), and on a coarse lattice (many ties)
    std::mt19937_64 gen(12345);
    std::uniform_real_distribution<double> U(-20.0, 0.0);
    for (const int K : {1, 3, 8})
        for (const long long R : {1LL, 2LL, 99LL, 200LL}) {
            std::vector<std::vector<double>> m((size_t)K, std::vector<double>((size_t)R)), lattice = m;
            for (int k = 0; k < K; k++)
                for (long long r = 0; r < R; r++) {
                    m[(size_t)k][(size_t)r] = U(gen) + (k > 0 ? 0.5 * m[0][(size_t)r] : 0.0);      // correlated widths
                    lattice[(size_t)k][(size_t)r] = floor(U(gen) / 4.0);
                }
            check_calibration(m, false);
            check_calibration(lattice, true);
        }

    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("ok scan_null_core_check: Philox known answers, uniforms, variates, combine rule, calibration counts and invariants\n");
    return 0;
}
