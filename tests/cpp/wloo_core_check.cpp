// wloo_core_check -- tamcmc_wloo.h on the CPU (plain g++), against long double and against the header's own statements:
//   the window sum     tmw_sum, which the sums kernel calls on l, adds in ascending bin order starting from the first term,
//                      in plain double: bit for bit the explicit loop, a sum of one term is that term, and the result lies
//                      within len 2^-53 sum|l| of the
//                      long-double sum; the same through the route the sums kernel takes, tms_like per bin and then the sum,
//                      for chi(2,2p) at p = 1, 2, 3 and chi_square
//   window geometry    for every W of the suites, every first in 0 ... W and grids on both sides of every edge: the windows
//                      of tmw_begin / tmw_end are non-empty, disjoint, ascending and cover [0, Nx); their number and their
//                      three lengths are tmw_partition's; the first, the full and the last window have tmw_kind 0, 1, 2; a grid
//                      shorter than `first` is one window
//   the byte counts    twl_begin_bytes and twl_pit_bytes are the expressions include/tamcmc_accel.h documents, and the
//                      pieces the host carves out of the two state allocations fit them exactly
// Prints one line, `ok wloo_core_check ...`, and returns 0; otherwise says what failed and returns 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "tamcmc_wloo.h"

static long fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; if (fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static bool same_bits(const double a, const double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static long check_sums()
{
    std::mt19937_64 rng(20261);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    long cases = 0;
    const int lens[] = {1, 2, 3, 5, 7, 20, 63, 64, 65, 511, 512};
    for (const int len : lens)
        for (int rep = 0; rep < 20; rep++) {
            std::vector<double> l((size_t)len);
            long double want = 0.0L, mag = 0.0L;
            // magnitudes over twelve decades and both signs: an order other than the stated one would show
            for (int i = 0; i < len; i++) {
                l[(size_t)i] = (U(rng) < 0.5 ? -1.0 : 1.0) * std::pow(10.0, 12.0 * U(rng) - 6.0);
                want += (long double)l[(size_t)i];
                mag += fabsl((long double)l[(size_t)i]);
            }
            double loop = l[0];
            for (int i = 1; i < len; i++) loop += l[(size_t)i];
            const double got = tmw_sum(l.data(), len);
            CHECK(same_bits(got, loop), "len %d: tmw_sum is not the ascending loop", len);
            if (len == 1) CHECK(same_bits(got, l[0]), "a sum of one term is not that term");
            CHECK(fabsl((long double)got - want) <= (long double)len * 0x1p-53L * mag, "len %d: %.17g against %.21Lg", len, got, want);
            cases++;
        }
    // the kernel's route: l per bin by tms_like, then the sum; against long double from the same y, M
    for (const int len : lens)
        for (int cfg = 0; cfg < 4; cfg++) {
            const bool gauss = cfg == 3;
            const double p = gauss ? 1.0 : (double)(cfg + 1);
            std::vector<double> l((size_t)len);
            long double want = 0.0L, mag = 0.0L;
            for (int i = 0; i < len; i++) {
                const double M = 0.5 + 20.0 * U(rng), y = M * -std::log(1.0 - U(rng)), isig2 = 1.0 / (0.01 + U(rng));
                l[(size_t)i] = tms_like(gauss, y, M, isig2, p);
                const long double t = gauss ? -(((long double)y - M) * ((long double)y - M)) * (long double)isig2
                                            : -(long double)p * ((long double)y / M + logl((long double)M));
                want += t;
                mag += fabsl(t);
            }
            const double got = tmw_sum(l.data(), len);
            // every term within 4 ulp of its long-double value, and the sum's own len 2^-53
            CHECK(fabsl((long double)got - want) <= ((long double)len + 8.0L) * 0x1p-53L * mag, "route len %d cfg %d: %.17g against %.21Lg", len, cfg, got, want);
            cases++;
        }
    return cases;
}

static long check_geometry()
{
    long cases = 0;
    const int Ws[] = {1, 2, 3, 5, 7, 20, 64, 511, 512};
    for (const int W : Ws)
        for (int first = 0; first <= W; first++) {
            if (W > 64 && first > 3 && first < W - 2 && first != W / 2) continue;      // the large widths: the ends and the middle
            const int f = first == 0 ? W : first;
            std::vector<long long> grids;
            for (long long k = 0; k <= 3; k++)
                for (long long d = -1; d <= 1; d++) grids.push_back((long long)f + k * W + d);
            grids.push_back(1); grids.push_back(2); grids.push_back(700); grids.push_back(1100);
            for (const long long Nx : grids) {
                if (Nx < 1) continue;
                int fr = first, len[3];
                const long long nw = tmw_partition(Nx, W, &fr, len);
                CHECK(fr == f, "W %d first %d: resolved to %d", W, first, fr);
                CHECK(nw >= 1 && nw == 1 + ((Nx > f ? Nx - f : 0) + W - 1) / W, "W %d first %d Nx %lld: %lld windows", W, first, Nx, nw);
                if (Nx <= f) CHECK(nw == 1 && len[0] == Nx, "W %d first %d Nx %lld: a grid no longer than first is one window", W, first, Nx);
                long long at = 0;
                for (long long w = 0; w < nw; w++) {
                    const long long b = tmw_begin(w, W, fr), e = tmw_end(w, W, fr, Nx);
                    CHECK(b == at && e > b && e <= Nx, "W %d first %d Nx %lld: window %lld is [%lld, %lld) after %lld", W, first, Nx, w, b, e, at);
                    const int kind = tmw_kind(w, nw);
                    CHECK(kind == (w == 0 ? 0 : (w == nw - 1 ? 2 : 1)), "kind of window %lld of %lld", w, nw);
                    CHECK(e - b == len[kind], "W %d first %d Nx %lld: window %lld holds %lld bins, its kind %d", W, first, Nx, w, e - b, len[kind]);
                    if (kind == 1) CHECK(e - b == W, "a window between the first and the last is not full");
                    at = e;
                }
                CHECK(at == Nx, "W %d first %d Nx %lld: the windows end at %lld", W, first, Nx, at);
                if (nw == 1) CHECK(len[2] == len[0], "one window: the last length is the first");
                cases++;
            }
        }
    return cases;
}

static long check_bytes()
{
    long cases = 0;
    const size_t nws[] = {1, 2, 13, 35, 350, 100000}, Ms[] = {1, 4, 8, 64, 794, 2048}, Bs[] = {1, 7, 64, 4096};
    for (const size_t nw : nws)
        for (const size_t M : Ms)
            for (const size_t B : Bs) {
                CHECK(twl_begin_bytes(nw, M, B) == 8 * (M + 1) * nw + 52 * nw + 32 + 8 * B * nw, "wloo_begin: nw %zu M %zu B %zu", nw, M, B);
                CHECK(twl_pit_bytes(nw, M, B) == 8 * M * nw + 116 * nw + 36 + 16 * B * nw, "wloo_pit_begin: nw %zu M %zu B %zu", nw, M, B);
                cases++;
            }
    for (const size_t nw : nws) {
        // the host's carve-up: body[3] | elpd | khat | cutoff doubles, four counts, tail_len
        const size_t state = (3 + 1 + 1 + 1) * nw * sizeof(double) + 4 * sizeof(long long) + nw * sizeof(int32_t);
        CHECK(state == twl_state_bytes(nw) && state == 52 * nw + 32, "state of %zu windows", nw);
        // sums[TM_LOOPIT_NSTATE] | xmax | c doubles, four counts, first slot, the flag
        const size_t pit = ((size_t)TM_LOOPIT_NSTATE + 2) * nw * sizeof(double) + 4 * sizeof(long long) + nw * sizeof(int32_t) + sizeof(int32_t);
        CHECK(pit == twl_pit_state_bytes(nw) && pit == 116 * nw + 36, "sub-mode state of %zu windows", nw);
        CHECK((((3 + 1 + 1 + 1) * nw * sizeof(double)) % alignof(long long)) == 0, "the counts are aligned");
    }
    CHECK(TM_LOOPIT_NSTATE == 12, "twelve state words");
    CHECK(tml_tail_M(466033) == TM_LOO_MAX_TAIL && tml_tail_M(466034) > TM_LOO_MAX_TAIL, "the longest chain");
    return cases;
}

int main()
{
    const long a = check_sums(), b = check_geometry(), c = check_bytes();
    if (fails) { printf("%ld checks failed\n", fails); return 1; }
    printf("ok wloo_core_check: %ld sums, %ld partitions, %ld byte counts\n", a, b, c);
    return 0;
}
