// bandess_core_check -- the integer arithmetic of tamcmc_bandess.h on the CPU (plain g++, `make bandess-core-check`): the packing,
// the ring, the head, the lag groups and the centred lag products, fed through TmbHostSeries in pieces of random sizes (pieces of
// 0 and of 1 included, rejected samples among them), against brute-force integer sums; E_k at the largest n against __int128;
// the comparison at signed zeros, infinities and NaN.  Prints one line, `ok bandess_core_check ...`, or the first mismatch.
#define TMB_HOST_FEED
#include "tamcmc_bandess.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

static long long checks = 0;

static int miss(const char *what, long long a, long long b, long long c, long long got, long long want)
{
    printf("MISMATCH %s (%lld, %lld, %lld): got %lld, want %lld\n", what, a, b, c, got, want);
    return 1;
}

// one series of n bits at lag limit L, fed as the values 1.0 (bit set) and 2.0 against the threshold 1.5
static int one_series(const std::vector<int> &b, const int L, std::mt19937 &rng, const int kind)
{
    const long long n = (long long)b.size();
    // brute force
    std::vector<long long> C((size_t)L + 1, 0), H((size_t)L + 1, 0), T((size_t)L + 1, 0), E((size_t)L + 1, 0);
    long long N = 0;
    for (long long t = 0; t < n; t++) N += b[(size_t)t];
    for (int k = 0; k <= L; k++) {
        for (long long t = k; t < n; t++) C[(size_t)k] += b[(size_t)t] * b[(size_t)(t - k)];
        for (long long t = 0; t < k; t++) H[(size_t)k] += b[(size_t)t];
        for (long long t = n - k; t < n; t++) T[(size_t)k] += b[(size_t)t];
        // n^2 sum (b_t - N/n)(b_{t-k} - N/n) = sum (n b_t - N)(n b_{t-k} - N), term by term
        for (long long t = k; t < n; t++) E[(size_t)k] += (n * b[(size_t)t] - N) * (n * b[(size_t)(t - k)] - N);
    }
    // the pushed stream: the accepted values with rejected samples sprinkled in (their values would set every bit)
    std::vector<double> v;
    std::vector<unsigned char> ok;
    const int rej_mode = (int)(rng() % 4);                  // 0: none, 1: a few, 2: runs of 64 ... 130, 3: every other
    for (long long t = 0; t < n; t++) {
        if (rej_mode == 1 && rng() % 7 == 0) { v.push_back(0.0); ok.push_back(0); }
        if (rej_mode == 2 && rng() % 40 == 0) for (unsigned r = 64 + rng() % 67; r > 0; r--) { v.push_back(0.0); ok.push_back(0); }
        if (rej_mode == 3) { v.push_back(0.0); ok.push_back(0); }
        v.push_back(b[(size_t)t] ? 1.0 : 2.0);
        ok.push_back(1);
    }
    if (rej_mode == 2) for (int r = 0; r < 70; r++) { v.push_back(0.0); ok.push_back(0); }
    TmbHostSeries s(L, 1.5);
    const long long m = (long long)v.size();
    for (long long at = 0; at < m;) {
        const unsigned pick = rng() % 8;
        long long piece = pick == 0 ? 0 : pick == 1 ? 1 : pick == 2 ? 64 : pick == 3 ? (long long)(rng() % (unsigned)(L + 2)) : (long long)(rng() % 200);
        if (piece > m - at) piece = m - at;
        s.push(v.data() + at, rej_mode ? ok.data() + at : nullptr, piece);
        at += piece;
    }
    if (s.t != n) return miss("accepted", n, L, kind, s.t, n);
    std::vector<long long> gotE((size_t)L + 1);
    std::vector<double> gotA((size_t)L + 1);
    s.centred(gotE.data());
    s.centred(gotA.data());
    for (int k = 0; k <= L; k++) {
        if ((long long)s.C[(size_t)k] != C[(size_t)k]) return miss("C_k", n, L, k, s.C[(size_t)k], C[(size_t)k]);
        if (tmb_E(n, k, N, C[(size_t)k], H[(size_t)k], T[(size_t)k]) != E[(size_t)k])
            return miss("tmb_E", n, L, k, tmb_E(n, k, N, C[(size_t)k], H[(size_t)k], T[(size_t)k]), E[(size_t)k]);
        if (gotE[(size_t)k] != E[(size_t)k]) return miss("E_k", n, L, k, gotE[(size_t)k], E[(size_t)k]);
        if (gotA[(size_t)k] != (double)E[(size_t)k]) return miss("A_k", n, L, k, (long long)gotA[(size_t)k], E[(size_t)k]);
        checks += 4;
    }
    if (gotE[0] != n * N * (n - N)) return miss("E_0", n, L, 0, gotE[0], n * N * (n - N));
    // the finish on these doubles: a constant series is NaN, NaN, 0; any other has a finite tau no smaller than the floor
    const double floor_ = 1.0 / std::log10((double)n);
    const TmeFinish f = tme_finish(gotA.data(), 1, L, (double)n, floor_);
    if (N == 0 || N == n) {
        if (!(std::isnan(f.tau) && std::isnan(f.ess) && f.cut == 0)) return miss("constant series", n, L, kind, f.cut, 0);
    } else if (!(f.tau >= floor_ && f.ess == (double)n / f.tau && f.cut >= 0 && f.cut <= L + 1 && f.cut % 2 == 0)) {
        return miss("finish", n, L, kind, f.cut, -1);
    }
    checks++;
    return 0;
}

int main()
{
    std::mt19937 rng(20240611u);
    static const int Ls[] = {1, 3, 63, 65, 127, 129};
    for (int n = 4; n <= 200; n++)
        for (const int L : Ls) {
            if (L > n - 1) continue;
            if (tme_lag_limit(L, n) != L) { printf("MISMATCH lag limit (%d, %d)\n", L, n); return 1; }
            for (int kind = 0; kind < 7; kind++) {
                std::vector<int> b((size_t)n, 0);
                for (int t = 0; t < n; t++)
                    b[(size_t)t] = kind == 0 ? (int)(rng() & 1) : kind == 1 ? (int)(rng() % 10 == 0) : kind == 2 ? 0 : kind == 3 ? 1 : kind == 4 ? (t & 1) :
                                   kind == 5 ? (t == 0) : (t == n - 1);
                if (one_series(b, L, rng, kind)) return 1;
            }
        }
    // longer series across several ring wraps at the largest lag limits
    for (const int L : {255, 1023}) {
        std::vector<int> b(3000);
        for (int &x : b) x = (int)(rng() % 3 == 0);
        if (one_series(b, L, rng, 7)) return 1;
    }
    // E_k at the largest n against 128-bit arithmetic: N = 1, n / 2, n - 1 with extreme heads and tails, every term's largest value
    {
        const long long n = TM_BANDESS_MAX_N - 1;
        for (const long long N : {1LL, n / 2, n - 1})
            for (const long long k : {0LL, 1LL, 1023LL})
                for (const long long C : {0LL, N > k ? N - k : 0LL, N})
                    for (const long long H : {0LL, k < N ? k : N})
                        for (const long long T : {0LL, k < N ? k : N}) {
                            const __int128 w = (__int128)n * n * C - (__int128)n * N * (2 * N - H - T) + (__int128)(n - k) * N * N;
                            const long long g = tmb_E(n, k, N, C, H, T);
                            if ((__int128)g != w) return miss("E_k at n = 2^20 - 1", N, k, C, g, (long long)w);
                            const __int128 lim = (__int128)1 << 62;
                            if (!(w < lim && w > -lim)) return miss("|E_k| < 2^62", N, k, C, g, 0);
                            checks++;
                        }
    }
    // the comparison: IEEE <=
    {
        const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
        struct { double v, thr; unsigned want; } cases[] = {
            {-0.0, 0.0, 1}, {0.0, -0.0, 1}, {1.0, inf, 1}, {inf, inf, 1}, {-inf, -inf, 1}, {1.0, -inf, 0}, {inf, 1e308, 0},
            {1.0, nan, 0}, {nan, 1.0, 0}, {nan, nan, 0}, {-inf, nan, 0}, {1.0, 1.0, 1}, {std::nextafter(1.0, 2.0), 1.0, 0}};
        for (const auto &c : cases) {
            if (tmb_le(c.v, c.thr) != c.want) { printf("MISMATCH tmb_le(%g, %g)\n", c.v, c.thr); return 1; }
            checks++;
        }
        // a NaN threshold gives 0 throughout; +inf gives 1 throughout
        const double v[5] = {-1.0, 0.0, 3.0, inf, -inf};
        TmbHostSeries sn(3, nan), si(3, inf);
        sn.push(v, nullptr, 5);
        si.push(v, nullptr, 5);
        if (sn.C[0] != 0 || si.C[0] != 5) { printf("MISMATCH NaN / inf thresholds\n"); return 1; }
    }
    // the helpers at their edges
    if (tmb_low(0) != 0 || tmb_low(64) != ~(uint64_t)0 || tmb_low(63) != (~(uint64_t)0 >> 1) || tmb_funnel(1, 2, 0) != 1 ||
        tmb_funnel(0, 1, 63) != 2 || tmb_ring_words(1) != 3 || tmb_ring_words(64) != 3 || tmb_ring_words(65) != 4 || tmb_ring_words(1023) != 18 ||
        tmb_head_words(1) != 1 || tmb_head_words(1023) != 16) {
        printf("MISMATCH helpers\n");
        return 1;
    }
    printf("ok bandess_core_check: %lld checks\n", checks);
    return 0;
}
