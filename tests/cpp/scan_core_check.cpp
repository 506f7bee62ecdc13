// scan_core_check.cpp -- the host arithmetic of tamcmc_scan.h on the CPU, plain g++ (-std=c++17 -O1 -ffp-contract=off; `make
// scan-core-check CHECKFLAGS=-fsanitize=address,undefined` for a sanitizer build): position counts and layout, the chunk
// size at its four regimes, the default line, the region finder against a brute force, and the prefix sums of one ascending
// walk against tmw_sum at every width.  Prints one line, "ok scan_core_check ...", or what failed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "tamcmc_scan.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

// the definition, position by position: is j below, and does a run start / end here
static std::vector<TmScanRegion> brute(const std::vector<double> &v, const std::vector<double> &mr, const int W, const double line)
{
    const long long n = (long long)v.size();
    auto below = [&](long long j) { return j >= 0 && j < n && v[(size_t)j] < line; };
    std::vector<TmScanRegion> out;
    for (long long j = 0; j < n; j++) {
        if (!below(j) || below(j - 1)) continue;
        long long e = j;
        while (below(e + 1)) e++;
        long long at = j;
        for (long long i = j; i <= e; i++)
            if (v[(size_t)i] < v[(size_t)at]) at = i;      // strict: the first position of the minimum
        TmScanRegion r;
        r.pos_first = j; r.pos_last = e; r.bin_first = j; r.bin_last = e + W - 1; r.pos_min = at;
        r.min_log = v[(size_t)at]; r.mean_resid_at_min = mr[(size_t)at];
        out.push_back(r);
    }
    return out;
}

static bool same(const TmScanRegion &a, const TmScanRegion &b)
{
    return a.pos_first == b.pos_first && a.pos_last == b.pos_last && a.bin_first == b.bin_first && a.bin_last == b.bin_last &&
           a.pos_min == b.pos_min && a.min_log == b.min_log && a.mean_resid_at_min == b.mean_resid_at_min;
}

// tmsc_regions with room for all, with max_regions 0 and 1, against the brute force; returns the count
static long long check_regions(const std::vector<double> &v, const int W, const double line)
{
    std::vector<double> mr(v.size());
    for (size_t i = 0; i < v.size(); i++) mr[i] = 1000.0 + (double)i;
    const std::vector<TmScanRegion> want = brute(v, mr, W, line);
    const long long n = (long long)v.size();
    std::vector<TmScanRegion> got(v.size() + 1);
    const long long count = tmsc_regions(v.data(), mr.data(), n, W, line, (long long)got.size(), got.data());
    CHECK(count == (long long)want.size());
    for (long long i = 0; i < count && i < (long long)want.size(); i++) CHECK(same(got[(size_t)i], want[(size_t)i]));
    CHECK(tmsc_regions(v.data(), mr.data(), n, W, line, 0, nullptr) == count);
    TmScanRegion one;
    one.pos_first = -7;
    CHECK(tmsc_regions(v.data(), mr.data(), n, W, line, 1, &one) == count);
    if (count >= 1) CHECK(same(one, want[0]));
    else CHECK(one.pos_first == -7);
    return count;
}

int main()
{
    const double nan = std::nan("");

    // position counts and layout
    CHECK(tmsc_positions(700, 1) == 700 && tmsc_positions(700, 20) == 681 && tmsc_positions(700, 700) == 1 && tmsc_positions(2, 2) == 1);
    {
        const int32_t W[4] = {1, 2, 7, 64};
        long long off[4];
        CHECK(tmsc_layout(65, 4, W, off) == 65 + 64 + 59 + 2 && off[0] == 0 && off[1] == 65 && off[2] == 129 && off[3] == 188);
        CHECK(tmsc_layout(65, 1, W + 2, off) == 59 && off[0] == 0);
    }

    // chunk size: one sample, a block below the cap, the 4096 cap, the 256 MiB cap
    CHECK(tmsc_chunk(1, 59) == 1);
    CHECK(tmsc_chunk(64, 59) == 64);
    CHECK(tmsc_chunk(5000, 59) == 4096 && tmsc_chunk(70001, 59) == 4096 && tmsc_chunk(4096, 59) == 4096 && tmsc_chunk(4095, 59) == 4095);
    {
        const int32_t W[8] = {1, 2, 4, 8, 16, 32, 64, 128};
        long long off[8];
        const long long total = tmsc_layout(100000, 8, W, off);
        CHECK(total == 8 * 100001LL - 255);
        const long long c = tmsc_chunk(64, total);
        CHECK(c == 13 && 24 * total * c <= TM_SCAN_SCRATCH_BYTES && 24 * total * (c + 1) > TM_SCAN_SCRATCH_BYTES);
        CHECK(tmsc_chunk(5, total) == 5);
        CHECK(tmsc_chunk(64, TM_SCAN_SCRATCH_BYTES) == 1);       // one sample alone is past the cap: still one
    }
    // the edges of the memory term fit = 256 MiB / (24 total): the last total at which a block of 64 is one chunk, the
    // first with fit = 1 and the first with fit = 0 (still one sample); the scratch [3][C][total] stays within the cap
    // wherever C > 1
    CHECK(tmsc_chunk(64, 174762) == 64 && tmsc_chunk(64, 174763) == 63 && tmsc_chunk(63, 174763) == 63 && tmsc_chunk(4096, 2730) == 4096 && tmsc_chunk(4096, 2731) == 4095);
    CHECK(tmsc_chunk(64, 5592405) == 2 && tmsc_chunk(64, 5592406) == 1 && tmsc_chunk(1, 5592405) == 1);
    CHECK(tmsc_chunk(64, 11184810) == 1 && tmsc_chunk(64, 11184811) == 1 && TM_SCAN_SCRATCH_BYTES / (24 * 11184810LL) == 1 && TM_SCAN_SCRATCH_BYTES / (24 * 11184811LL) == 0);
    for (const long long B : {1LL, 2LL, 63LL, 64LL, 2600LL, 4096LL, 70001LL})
        for (long long total = 1; total <= 12000000; total += total < 5000 ? 1 : 4999) {
            const long long c = tmsc_chunk(B, total);
            CHECK(c >= 1 && c <= B && c <= TM_SCAN_CHUNK_MAX && (c == 1 || 24 * total * c <= TM_SCAN_SCRATCH_BYTES));
            CHECK(c == B || c == TM_SCAN_CHUNK_MAX || c == 1 || 24 * total * (c + 1) > TM_SCAN_SCRATCH_BYTES);
        }

    // the default line
    CHECK(tmsc_default_line(20, 700) == std::log(0.01 * 20.0 / 700.0) && std::fabs(tmsc_default_line(20, 700) - (-8.1605)) < 1e-4);
    CHECK(tmsc_default_line(1, 100000) < tmsc_default_line(512, 100000) && tmsc_default_line(512, 512) == std::log(0.01));

    // the region finder: hand-made cases
    const double line = -3.0;
    CHECK(check_regions({}, 5, line) == 0);
    CHECK(check_regions({-1.0, -2.0, -3.0, 0.0, nan}, 5, line) == 0);                       // none below (-3 is not below -3)
    CHECK(check_regions({-4.0, -5.0, -6.0, -3.5}, 5, line) == 1);                           // all below
    CHECK(check_regions({-4.0, -1.0, -1.0, -4.0}, 5, line) == 2);                           // a run at each end
    CHECK(check_regions({-1.0, -4.0, -5.0, -2.0, -6.0, -4.0, -1.0}, 3, line) == 2);         // adjacent runs split by one value
    CHECK(check_regions({-1.0, -4.0, -5.0, nan, -6.0, -4.0, -1.0}, 3, line) == 2);          // ... by a NaN
    CHECK(check_regions({-1.0, -5.0, -4.0, -5.0, -5.0, -1.0}, 2, line) == 1);               // ties at the minimum
    {
        const std::vector<double> v = {-1.0, -5.0, -4.0, -5.0, -5.0, -1.0, -9.0};
        const std::vector<double> mr = {0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0};
        TmScanRegion r[2];
        CHECK(tmsc_regions(v.data(), mr.data(), 7, 4, line, 2, r) == 2);
        CHECK(r[0].pos_first == 1 && r[0].pos_last == 4 && r[0].bin_first == 1 && r[0].bin_last == 7 && r[0].pos_min == 1 && r[0].min_log == -5.0 &&
              r[0].mean_resid_at_min == 1.0);
        CHECK(r[1].pos_first == 6 && r[1].pos_last == 6 && r[1].bin_last == 9 && r[1].pos_min == 6 && r[1].min_log == -9.0 && r[1].mean_resid_at_min == 6.0);
    }
    // ... and random arrays with NaNs, few distinct values so that ties and adjacent runs are common
    std::mt19937_64 rng(12345);
    long long runs = 0;
    for (int rep = 0; rep < 2000; rep++) {
        const size_t n = 1 + (size_t)(rng() % 40);
        std::vector<double> v(n);
        for (size_t i = 0; i < n; i++) {
            const unsigned u = (unsigned)(rng() % 10);
            v[i] = u == 0 ? nan : (u == 1 ? -(double)INFINITY : -0.5 * (double)(rng() % 12));
        }
        runs += check_regions(v, 1 + (int)(rng() % 512), rep % 3 == 0 ? -1e-300 : -(double)(1 + rep % 5));
    }
    CHECK(runs > 2000);

    // the prefixes of ONE ascending sum are tmw_sum's bits at every width
    {
        std::uniform_real_distribution<double> U(0.0, 4.0);
        std::vector<double> q(1200);
        for (double &x : q) x = U(rng) * std::exp(8.0 * (U(rng) - 2.0));
        const int32_t W[8] = {1, 2, 3, 7, 20, 64, 100, 512};
        for (size_t j = 0; j + 512 <= q.size(); j += 37) {
            double sum = q[j];
            int terms = 1;
            for (int k = 0; k < 8; k++) {
                for (; terms < W[k]; terms++) sum += q[j + (size_t)terms];
                CHECK(sum == tmw_sum(q.data() + j, W[k]));
            }
        }
    }

    if (failures) return 1;
    std::printf("ok scan_core_check: layout, chunk sizes, default line, %lld regions against the brute force, prefix sums\n", runs);
    return 0;
}
