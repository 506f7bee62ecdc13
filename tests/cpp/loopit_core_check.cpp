// loopit_core_check -- tamcmc_loopit.h on the CPU (plain g++, one lane), against a long-double brute force:
//   the tie-mean rule   runs of 1, 2, 7 and "all equal" in a tail, and a tie with the cutoff (which is body and must not
//                       join a run), through the route the prepare kernel takes: top set -> sort -> tml_finalize -> tlp_tie_lw
//   the clamped search  columns of 1, 2, 63, 64, 65 (and 2047, 2048) slots: every stored value is found at the first slot
//                       of its run, values below, between and above are not, and no probe leaves [1, M]
//   the four sums       tlp_add over a sequence with -inf terms against sums of long-double exponentials
// Prints one line, `ok loopit_core_check ...`, and returns 0; otherwise says what failed and returns 1.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "tamcmc_loopit.h"

static long fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; if (fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct OneLane {
    int lane() const { return 0; }
    int lanes() const { return 1; }
    double sum(double v) const { return v; }
    void sync() const {}
};

// what the prepare kernel computes for one bin: the sorted candidates, and lw per sorted slot
struct Prepared {
    std::vector<double> s, lw, zt;
    double xmax, c, root;
    int nb, L;
};

static Prepared prepare(const std::vector<double> &xs)
{
    const long long n = (long long)xs.size();
    const int cap = (int)tml_tail_M(n) + 1;
    std::vector<double> heap((size_t)cap), t((size_t)cap), theta(TM_LOO_MAX_THETA), ell(TM_LOO_MAX_THETA);
    double root = 0.0, a = 0.0, r = 0.0, c = 0.0;
    for (long long k = 0; k < n; k++) tml_top_push(heap.data(), 1, cap, k, xs[(size_t)k], &root, &a, &r, &c);
    const int cnt = n < cap ? (int)n : cap;
    Prepared p;
    p.s.assign(heap.begin() + 1, heap.begin() + cnt);
    std::sort(p.s.begin(), p.s.end());
    OneLane w;
    const int ncand = cnt - 1;
    const TmlBin b = tml_finalize(w, p.s.data(), ncand, heap[0], n >= cap, n, a, r - c, t.data(), theta.data(), ell.data());
    p.L = b.tail_len; p.nb = ncand - p.L; p.root = heap[0];
    p.xmax = ncand > 0 ? p.s[(size_t)ncand - 1] : heap[0];
    p.c = n >= cap ? fmax(heap[0] - p.xmax, log(DBL_MIN)) : (double)INFINITY;
    p.zt.assign(t.begin(), t.begin() + p.L);
    p.lw.resize((size_t)ncand);
    for (int j = 0; j < ncand; j++)
        p.lw[(size_t)j] = j < p.nb ? p.s[(size_t)j] - p.xmax : tlp_tie_lw(p.s.data() + p.nb, t.data(), p.L, j - p.nb);
    return p;
}

static double ulps(const double got, const long double want)
{
    if (std::isnan(got) || std::isnan((double)want)) return std::isnan(got) && std::isnan((double)want) ? 0.0 : 1e300;
    if ((long double)got == want) return 0.0;
    const double scale = std::fmax(1.0, std::fabs((double)want));
    return (double)(fabsl((long double)got - want) / ((long double)scale * 0x1p-52L));
}

// xs: the samples of one bin; every tail slot's lw against the long-double mean over its run
static double check_ties(const std::vector<double> &xs, const char *what, const int want_longest_run)
{
    const Prepared p = prepare(xs);
    double worst = 0.0;
    int longest = 0;
    for (int j = 0; j < p.L; j++) {
        const double x = p.s[(size_t)(p.nb + j)];
        CHECK(x - p.xmax > p.c, "%s: tail slot %d is not above the cutoff", what, j);
        int a = j, b = j;
        while (a > 0 && p.s[(size_t)(p.nb + a - 1)] == x) a--;
        while (b + 1 < p.L && p.s[(size_t)(p.nb + b + 1)] == x) b++;
        longest = std::max(longest, b - a + 1);
        long double sum = 0.0L;
        for (int i = a; i <= b; i++) sum += expl((long double)p.zt[(size_t)i]);
        const long double want = a == b ? (long double)p.zt[(size_t)j] : logl(sum / (long double)(b - a + 1));
        const double u = ulps(p.lw[(size_t)(p.nb + j)], want);
        worst = std::max(worst, u);
        if (a == b) CHECK(tlp_same_bits(p.lw[(size_t)(p.nb + j)], p.zt[(size_t)j]), "%s: a run of 1 must keep zt's bits", what);
        else CHECK(tlp_same_bits(p.lw[(size_t)(p.nb + j)], p.lw[(size_t)(p.nb + a)]), "%s: the members of a run differ", what);
    }
    for (int j = 0; j < p.nb; j++) {
        CHECK(!(p.s[(size_t)j] - p.xmax > p.c), "%s: body slot %d is above the cutoff", what, j);
        CHECK(tlp_same_bits(p.lw[(size_t)j], p.s[(size_t)j] - p.xmax), "%s: a body slot's weight is z", what);
    }
    CHECK(worst <= 4.0, "%s: tie-mean off by %.3g ulp", what, worst);
    CHECK(want_longest_run < 0 || longest == want_longest_run, "%s: longest run %d, expected %d", what, longest, want_longest_run);
    return worst;
}

static double check_tie_rule()
{
    std::mt19937_64 g(1234);
    std::normal_distribution<double> N(0.0, 1.0);
    double worst = 0.0;
    const int n = 400;                                         // M = 60
    std::vector<double> base((size_t)n);
    for (auto &v : base) v = 3.0 + N(g);
    std::vector<double> sorted = base;
    std::sort(sorted.begin(), sorted.end());
    worst = std::max(worst, check_ties(base, "distinct", 1));
    auto with_run = [&](const int len, const int rank_from_top) {          // the value at that rank, len times in all
        std::vector<double> xs = base;
        const double v = sorted[(size_t)(n - 1 - rank_from_top)];
        int put = 1;
        for (size_t k = 0; k < xs.size() && put < len; k++)
            if (xs[k] < sorted[(size_t)(n - 70)]) { xs[k] = v; put++; }      // body samples become copies of the tail value
        return xs;
    };
    worst = std::max(worst, check_ties(with_run(2, 10), "run of 2", 2));
    worst = std::max(worst, check_ties(with_run(7, 20), "run of 7", 7));
    worst = std::max(worst, check_ties(with_run(2, 0), "run of 2 at the maximum", 2));
    {
        std::vector<double> xs((size_t)n, 1.25);                // all equal: every candidate ties with the cutoff, L = 0
        const Prepared p = prepare(xs);
        CHECK(p.L == 0 && p.nb == 60, "all equal: L = %d, nb = %d", p.L, p.nb);
        worst = std::max(worst, check_ties(xs, "all equal", 0));
    }
    {
        std::vector<double> xs = base;                          // the whole tail one value above a distinct body
        for (auto &v : xs) if (v > sorted[(size_t)(n - 61)]) v = 9.0;
        const Prepared p = prepare(xs);
        CHECK(p.L == 60, "tail all equal: L = %d", p.L);
        worst = std::max(worst, check_ties(xs, "tail all equal", 60));
    }
    {
        // a tie with the cutoff: the (M+1)-th largest value five times, three of them among the candidates.  They are body.
        std::vector<double> xs = base;
        const double cut = sorted[(size_t)(n - 61)];
        int put = 0;
        for (auto &v : xs) if (v > cut && v <= sorted[(size_t)(n - 58)]) { v = cut; put++; }
        for (size_t k = 0; k < xs.size() && put < 4; k++) if (xs[k] < sorted[10]) { xs[k] = cut; put++; }
        const Prepared p = prepare(xs);
        CHECK(p.root == cut && p.nb >= 3 && p.L == 60 - p.nb, "tie with the cutoff: root %.17g cut %.17g nb %d L %d", p.root, cut, p.nb, p.L);
        for (int j = 0; j < p.nb; j++) CHECK(p.s[(size_t)j] == cut, "tie with the cutoff: body slot %d", j);
        worst = std::max(worst, check_ties(xs, "tie with the cutoff", -1));
    }
    {
        std::vector<double> xs;                                 // every row twice, as a chain with rejected proposals has them
        for (auto v : base) { xs.push_back(v); xs.push_back(v); }
        worst = std::max(worst, check_ties(xs, "every sample twice", 2));
        for (int nn : {1, 4, 20, 21, 26}) {                    // short chains: raw weights up to n = 20, the first fit at 21
            std::vector<double> y(base.begin(), base.begin() + nn);
            worst = std::max(worst, check_ties(y, "short", -1));
        }
    }
    return worst;
}

static long check_search()
{
    long done = 0;
    std::mt19937_64 g(99);
    std::uniform_real_distribution<double> U(-5.0, 5.0);
    for (int M : {1, 2, 3, 63, 64, 65, 2047, 2048}) {
        const int T = tlp_trips(M);
        CHECK(((long long)1 << T) >= (long long)M + 1 && (T == 0 || ((long long)1 << (T - 1)) < (long long)M + 1), "trips(%d) = %d", M, T);
        for (int variant = 0; variant < 3; variant++) {
            std::vector<double> col((size_t)M + 1);             // slot 0 is the root: never read
            col[0] = NAN;
            for (int k = 1; k <= M; k++) col[(size_t)k] = variant == 2 ? 1.5 : U(g);
            std::sort(col.begin() + 1, col.end());
            if (variant == 1) for (int k = 2; k <= M; k += 3) col[(size_t)k] = col[(size_t)k - 1];      // runs of 2
            std::vector<double> probes(col.begin() + 1, col.end());
            probes.push_back(-6.0); probes.push_back(6.0); probes.push_back(-INFINITY); probes.push_back(INFINITY); probes.push_back(NAN);
            for (int k = 1; k < M; k++) if (col[(size_t)k] < col[(size_t)k + 1]) probes.push_back(0.5 * (col[(size_t)k] + col[(size_t)k + 1]));
            probes.push_back(-0.0); probes.push_back(0.0);
            for (const double x : probes) {
                // the steps one by one, as the kernel takes them: no probe leaves the column
                int pos = 0;
                for (int t = T - 1; t >= 0; t--) {
                    const int i = tlp_probe(pos, 1 << t, M);
                    CHECK(i >= 1 && i <= M, "M = %d: probe %d", M, i);
                    pos = tlp_advance(pos, 1 << t, M, col[(size_t)i], x);
                    CHECK(pos >= 0 && pos <= M, "M = %d: pos %d", M, pos);
                }
                const int slot = tlp_slot(pos, M);
                bool found = false;
                const int slot2 = tlp_find(col.data(), 1, M, T, x, &found);
                CHECK(slot == slot2 && slot >= 1 && slot <= M, "M = %d: slot %d / %d", M, slot, slot2);
                const int lb = (int)(std::lower_bound(col.begin() + 1, col.end(), x) - col.begin());     // M + 1: above all
                const int want = std::isnan(x) ? 1 : std::min(lb, M);
                CHECK(slot == want, "M = %d x = %.17g: slot %d, lower bound %d", M, x, slot, want);
                bool stored = false;
                for (int k = 1; k <= M; k++) stored = stored || tlp_same_bits(col[(size_t)k], x);
                // (+0 and -0 compare equal and differ in bits: the one that is not stored is reported as not found)
                const bool reachable = stored && !(x == 0.0 && !tlp_same_bits(col[(size_t)slot], x));
                CHECK(found == reachable, "M = %d x = %.17g: found %d, stored %d", M, x, (int)found, (int)stored);
                done++;
            }
        }
    }
    return done;
}

static double check_sums()
{
    std::mt19937_64 g(7);
    std::normal_distribution<double> N(0.0, 1.0);
    double worst = 0.0;
    for (int trial = 0; trial < 6; trial++) {
        const int n = trial == 0 ? 1 : 500 * trial;
        TlpSums s{};
        long double W = 0.0L, A = 0.0L, B = 0.0L, W2 = 0.0L;
        bool anyA = false;
        for (int k = 0; k < n; k++) {
            const double lw = (trial & 1 ? -40.0 : -3.0) * std::fabs(N(g)), z = std::fabs(3.0 * N(g));
            double lP, lQ;
            if (k % 7 == 3) tmp_chi_p1(0.0, &lP, &lQ);          // a datum of 0: logP = -inf, skipped
            else tmp_chi_p1(z * (trial == 5 ? 200.0 : 1.0), &lP, &lQ);
            tlp_add(&s, lw, lP, lQ);
            W += expl((long double)lw); W2 += expl(2.0L * (long double)lw);
            if (lP != -INFINITY) { A += expl((long double)lw + (long double)lP); anyA = true; }
            B += expl((long double)lw + (long double)lQ);
        }
        const double lW = tlp_lse(s.wa, s.wr, s.wc), lA = tlp_lse(s.aa, s.ar, s.ac), lB = tlp_lse(s.ba, s.br, s.bc), lW2 = tlp_lse(s.qa, s.qr, s.qc);
        worst = std::max(worst, ulps(lW, logl(W)));
        worst = std::max(worst, ulps(lW2, logl(W2)));
        worst = std::max(worst, ulps(lB, logl(B)));
        if (anyA) worst = std::max(worst, ulps(lA, logl(A)));
        else CHECK(lA == -INFINITY, "a sum without a finite term must be -inf");
        const long double ess = W * W / W2;
        CHECK(ess >= 1.0L - 1e-12L && ess <= (long double)n * (1.0L + 1e-12L), "ess %.6Lg outside 1 ... %d", ess, n);
        worst = std::max(worst, ulps(std::exp(2.0 * lW - lW2), ess) / std::fmax(1.0, (double)ess));
        // the tails sum to the weights: exp(lA - lW) + exp(lB - lW) = 1
        CHECK(std::fabs(std::exp(lA - lW) + std::exp(lB - lW) - 1.0) < 1e-13, "tails do not sum to 1: %.3g", std::exp(lA - lW) + std::exp(lB - lW) - 1.0);
    }
    CHECK(worst <= 16.0, "sums off by %.3g ulp of max(1, |value|)", worst);
    {
        TlpSums s{};                                            // nothing but -inf: every sum empty
        tlp_add(&s, -INFINITY, 0.0, 0.0);
        CHECK(s.wr == 0.0 && tlp_lse(s.wa, s.wr, s.wc) == -INFINITY, "a weight of -inf must add nothing");
    }
    return worst;
}

int main()
{
    const double tie = check_tie_rule();
    const long searched = check_search();
    const double sums = check_sums();
    if (fails) { printf("loopit_core_check: %ld failures\n", fails); return 1; }
    printf("ok loopit_core_check: tie-mean within %.2f ulp, %ld searches, sums within %.2f ulp\n", tie, searched, sums);
    return 0;
}
