// modetable_core_check -- tamcmc_modetable.h on the CPU (plain g++):
//   the column layout  tm_mt_layout / tm_mt_mult_first / tm_mt_ncols against tables written out by hand for ids 2, 8, 13
//                      (global, lmax 1, 2, 3) and 11 (local; once with an empty degree): every multiplet's (order, l, params
//                      index of its frequency, first column) and the number of columns; the kinds, m and the -1 entries of every
//                      column; 277 columns for the benchmark layout
//   the selection      tm_mt_select, the passes the quantile kernel runs, against std::sort for every rank of columns with
//                      ties, +-inf, +-0, denormals, one value, all values equal, and a stride; every bits-per-pass 1 ... 8
//   the fold           tm_mt_fold_one: equal values give a sum of squared deviations of exactly 0, and the mean, minimum and
//                      maximum of the value; random values stay within n 2^-52 mean|v| of the long-double mean
//   the byte counts    the expressions include/tamcmc_accel.h documents
// Prints one line, `ok modetable_core_check ...`, and returns 0; otherwise says what failed and returns 1.  With the
// arguments `layout <id> <Nmax> <lmax> <Nfl0> ... <Nfl3>` it prints the header's layout of that plength instead.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "tamcmc_modetable.h"

static long fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; if (fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Mult { int n, l, idx_f, first; };

static TmLayout make_layout(int id, int family, int Nmax, int lmax, const int Nfl[4])
{
    TmLayout L{};
    L.model_case = id; L.family = family; L.Nmax = Nmax; L.lmax = lmax;
    int nf = 0;
    for (int l = 0; l < 4; l++) { L.Nfl[l] = Nfl[l]; nf += Nfl[l]; }
    L.off_f[0] = Nmax + lmax;
    for (int l = 1; l < 4; l++) L.off_f[l] = L.off_f[l - 1] + Nfl[l - 1];
    L.n_mult = family == TM_FAM_GLOBAL ? Nmax * (lmax + 1) : nf;
    return L;
}

static long check_layout(const char *tag, const TmLayout &L, const std::vector<Mult> &want, int want_cols)
{
    CHECK(L.n_mult == (int)want.size(), "%s: n_mult %d", tag, L.n_mult);
    CHECK(tm_mt_ncols(L) == want_cols && tm_mt_layout(L, nullptr) == want_cols, "%s: n_cols %d, expected %d", tag, tm_mt_ncols(L), want_cols);
    std::vector<TmMtCol> c((size_t)want_cols + 1, TmMtCol{-7, -7, -7, -7, -7, -7});
    tm_mt_layout(L, c.data());
    CHECK(c[(size_t)want_cols].kind == -7, "%s: wrote past the last column", tag);
    for (int k = 0; k < 4; k++)
        CHECK(c[k].kind == k && c[k].mult == -1 && c[k].order == -1 && c[k].l == -1 && c[k].m == 0 && c[k].param_index == -1, "%s: chain column %d", tag, k);
    long seen = 4;
    for (size_t j = 0; j < want.size(); j++) {
        const Mult &w = want[j];
        int n, l;
        tm_mt_mult_nl(L, (int)j, &n, &l);
        CHECK(n == w.n && l == w.l, "%s: multiplet %zu is (%d, %d)", tag, j, n, l);
        CHECK(tm_mt_mult_first(L, (int)j) == w.first && (long)w.first == seen, "%s: multiplet %zu starts at %d", tag, j, tm_mt_mult_first(L, (int)j));
        const TmMtCol *o = c.data() + w.first;
        for (int k = 0; k < 7; k++)
            CHECK(o[k].kind == 4 + k && o[k].mult == (int)j && o[k].order == w.n && o[k].l == w.l && o[k].m == 0 &&
                  o[k].param_index == (k == 0 ? w.idx_f : -1), "%s: multiplet %zu column %d", tag, j, k);
        for (int k = 0; k < 2 * w.l + 1; k++) {
            const TmMtCol &a = o[7 + k], &b = o[7 + 2 * w.l + 1 + k];
            CHECK(a.kind == TM_MT_NU_M && b.kind == TM_MT_H_M && a.m == k - w.l && b.m == k - w.l && a.mult == (int)j && b.mult == (int)j &&
                  a.order == w.n && b.order == w.n && a.l == w.l && b.l == w.l && a.param_index == -1 && b.param_index == -1,
                  "%s: multiplet %zu component %d", tag, j, k);
        }
        seen += 7 + 2 * (2 * w.l + 1);
    }
    CHECK(seen == want_cols, "%s: the multiplets hold %ld columns", tag, seen);
    return (long)want.size();
}

static long check_layouts()
{
    long n = 0;
    { const int f[4] = {2, 2, 0, 0};          // id 2, Nmax 2, lmax 1: params = 2 heights, 1 visibility, then the frequencies
      n += check_layout("id2", make_layout(2, TM_FAM_GLOBAL, 2, 1, f), {{0, 0, 3, 4}, {0, 1, 5, 13}, {1, 0, 4, 26}, {1, 1, 6, 35}}, 48); }
    { const int f[4] = {2, 2, 2, 0};          // id 8, Nmax 2, lmax 2
      n += check_layout("id8", make_layout(8, TM_FAM_GLOBAL, 2, 2, f),
                        {{0, 0, 4, 4}, {0, 1, 6, 13}, {0, 2, 8, 26}, {1, 0, 5, 43}, {1, 1, 7, 52}, {1, 2, 9, 65}}, 82); }
    { const int f[4] = {2, 2, 2, 2};          // id 13, Nmax 2, lmax 3
      n += check_layout("id13", make_layout(13, TM_FAM_GLOBAL, 2, 3, f),
                        {{0, 0, 5, 4}, {0, 1, 7, 13}, {0, 2, 9, 26}, {0, 3, 11, 43}, {1, 0, 6, 64}, {1, 1, 8, 73}, {1, 2, 10, 86}, {1, 3, 12, 103}}, 124); }
    { const int f[4] = {2, 2, 2, 2};          // id 11, eight heights, two modes of every degree: degree by degree
      n += check_layout("id11", make_layout(11, TM_FAM_LOCAL, 8, 0, f),
                        {{0, 0, 8, 4}, {1, 0, 9, 13}, {0, 1, 10, 22}, {1, 1, 11, 35}, {0, 2, 12, 48}, {1, 2, 13, 65}, {0, 3, 14, 82}, {1, 3, 15, 103}}, 124); }
    { const int f[4] = {1, 0, 2, 0};          // id 11 with no l = 1 and no l = 3 mode
      n += check_layout("id11-gaps", make_layout(11, TM_FAM_LOCAL, 3, 0, f), {{0, 0, 3, 4}, {0, 2, 4, 13}, {1, 2, 5, 30}}, 47); }
    { const int f[4] = {7, 7, 7, 0};          // the benchmark layout
      CHECK(tm_mt_ncols(make_layout(2, TM_FAM_GLOBAL, 7, 2, f)) == 277, "benchmark layout: %d columns", tm_mt_ncols(make_layout(2, TM_FAM_GLOBAL, 7, 2, f))); }
    { const int f[4] = {64, 64, 64, 64};      // TM_MAXMULT multiplets
      const TmLayout L = make_layout(2, TM_FAM_GLOBAL, 64, 3, f);
      CHECK(L.n_mult == TM_MAXMULT && tm_mt_ncols(L) == 4 + 64 * 60, "256 multiplets: %d columns", tm_mt_ncols(L)); }
    return n;
}

static bool same_value(double a, double b) { return tmq_key(a) == tmq_key(b); }   // bit for bit, -0 and +0 one value

static long check_select_column(const char *tag, const std::vector<double> &v, size_t stride)
{
    const long long n = (long long)(v.size() / stride);
    std::vector<double> s;
    for (long long i = 0; i < n; i++) s.push_back(v[(size_t)i * stride]);
    std::sort(s.begin(), s.end());
    long cases = 0;
    for (int bits = 1; bits <= TM_MT_QBITS; bits++)
        for (long long k = 0; k < n; k++) {
            const double got = tm_mt_select(v.data(), stride, n, s.front(), s.back(), (uint64_t)k, bits);
            CHECK(same_value(got, s[(size_t)k]), "%s: bits %d rank %lld of %lld: %.17g, expected %.17g", tag, bits, k, n, got, s[(size_t)k]);
            cases++;
        }
    return cases;
}

static long check_select()
{
    const double inf = std::numeric_limits<double>::infinity(), den = std::numeric_limits<double>::denorm_min();
    std::mt19937_64 rng(20264);
    std::normal_distribution<double> N(0.0, 1.0);
    long cases = 0;
    cases += check_select_column("one value", {3.25}, 1);
    cases += check_select_column("all equal", std::vector<double>(37, -1.5), 1);
    cases += check_select_column("zeros", {0.0, -0.0, 0.0, -0.0, 1.0, -1.0}, 1);
    cases += check_select_column("infinities", {inf, -inf, 0.0, 1.0, inf, -inf, -0.0, 2.0, den, -den}, 1);
    cases += check_select_column("neighbours", {1.0, std::nextafter(1.0, 2.0), std::nextafter(1.0, 0.0), 1.0, 2.0, std::nextafter(2.0, 1.0)}, 1);
    std::vector<double> v(301);
    for (double &t : v) t = std::floor(4.0 * N(rng)) / 4.0;           // heavy ties, both signs
    cases += check_select_column("ties", v, 1);
    for (double &t : v) t = 3000.0 + N(rng);
    cases += check_select_column("frequencies", v, 1);
    cases += check_select_column("stride", v, 7);
    for (double &t : v) t = std::exp(30.0 * N(rng)) * (N(rng) < 0 ? -1.0 : 1.0);
    cases += check_select_column("decades", v, 1);
    // the rank rule at the ends
    CHECK(tmq_rank(0.0, 5) == 0 && tmq_rank(1.0, 5) == 4 && tmq_rank(1e-9, 5) == 0 && tmq_rank(0.5, 5) == 2 && tmq_rank(0.5, 4) == 1, "tmq_rank");
    return cases;
}

static long check_fold()
{
    std::mt19937_64 rng(20265);
    std::normal_distribution<double> N(0.0, 1.0);
    long cases = 0;
    for (const double v : {3017.25, -0.1, 0.0, 1e-300, 1e300}) {
        double mean = 0.0, M2 = 0.0, mn = 0.0, mx = 0.0;
        for (long long n = 1; n <= 50; n++) tm_mt_fold_one(mean, M2, mn, mx, n, v);
        CHECK(mean == v && M2 == 0.0 && mn == v && mx == v, "equal values %g: mean %g M2 %g", v, mean, M2);
        cases++;
    }
    for (const int n : {1, 2, 3, 37, 1000}) {
        double mean = 0.0, M2 = 0.0, mn = 0.0, mx = 0.0;
        long double sum = 0.0L, mag = 0.0L, lo = 0, hi = 0;
        for (long long k = 1; k <= n; k++) {
            const double v = 3000.0 + 5.0 * N(rng);
            tm_mt_fold_one(mean, M2, mn, mx, k, v);
            sum += v; mag += std::fabs(v);
            lo = (k == 1 || v < lo) ? v : lo; hi = (k == 1 || v > hi) ? v : hi;
        }
        CHECK(std::fabs((long double)mean - sum / n) <= n * 0x1p-52L * (mag / n), "mean of %d", n);
        CHECK(mn == (double)lo && mx == (double)hi && M2 >= 0.0, "envelope of %d", n);
        cases++;
    }
    return cases;
}

static long check_bytes()
{
    CHECK(tm_mt_table_bytes(1000, 277) == (size_t)8 * 1000 * 277, "table bytes");
    CHECK(tm_mt_block(277) == 4096 && tm_mt_block(4 + 64 * 60) == (int)((1u << 23) / (4 + 64 * 60)) && tm_mt_block(48) == 4096, "block");
    CHECK(tm_mt_block_bytes(4096, 56, 277) == (size_t)8 * 4096 * (56 + 277 + 1), "block bytes");
    CHECK(tm_mt_state_bytes(277) == (size_t)128 * 277 + 64, "state bytes");
    return 4;
}

// `modetable_core_check layout <id> <Nmax> <lmax> <Nfl0> <Nfl1> <Nfl2> <Nfl3>`: the header's layout of that plength, one
// line per column (kind mult order l m param_index), for tests/test_modetable_host.py to hold against its restatement
static int print_layout(char *argv[])
{
    const int id = atoi(argv[2]), Nmax = atoi(argv[3]), lmax = atoi(argv[4]);
    const int f[4] = {atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8])};
    const TmLayout L = make_layout(id, (id == 11 || id == 14) ? TM_FAM_LOCAL : TM_FAM_GLOBAL, Nmax, lmax, f);
    if (L.n_mult < 1 || L.n_mult > TM_MAXMULT) return 2;
    std::vector<TmMtCol> c((size_t)tm_mt_layout(L, nullptr));
    tm_mt_layout(L, c.data());
    for (const TmMtCol &k : c) printf("%d %d %d %d %d %d\n", k.kind, k.mult, k.order, k.l, k.m, k.param_index);
    return 0;
}

int main(int argc, char *argv[])
{
    if (argc == 9 && std::strcmp(argv[1], "layout") == 0) return print_layout(argv);
    const long a = check_layouts(), b = check_select(), c = check_fold(), d = check_bytes();
    if (fails) { printf("modetable_core_check: %ld failures\n", fails); return 1; }
    printf("ok modetable_core_check: %ld multiplets laid out, %ld selections, %ld folds, %ld byte counts\n", a, b, c, d);
    return 0;
}
