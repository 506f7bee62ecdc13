// seismic_core_check.cpp -- the plan and the arithmetic of tamcmc_seismic.h on the CPU (plain g++, no GPU, no library):
//   * plans of the global layouts lmax = 0 ... 3 with Nmax = 3, 4, 5, of lmax = 3 with Nmax = 12 and lmax = 0 with Nmax = 70, and
//     of the local layout Nfl = (4, 3, 4, 2), from rows on nu = Dnu (n + l / 2 + eps) - l (l + 1) D0: the number of columns of
//     every kind against its closed form, the columns' order, every source a freq (or amplitude) column of the right mode,
//     the CSR arrays consistent, n_base, dnu_ref and eps_ref;
//   * assignment on a hand-built ladder: an l = 1 mode shifted to |u - k| = 0.34 (assigned) and to 0.36 (not), a duplicate
//     order (both unassigned), a radial gap refused, two radial modes refused, a NaN radial frequency refused;
//   * least-squares coefficients: sum c_i = 0, sum c_i k_i = 1, sum a_i = 1, sum a_i k_i = 0 to their rounding, ladders with gaps;
//   * the evaluator against long double on random rows, the single-subtraction columns bit for bit, nu_max's weights, a zero
//     denominator (+-inf), 0 / 0 (NaN), an offset, the constant-one source.
// Prints "ok seismic_core_check ..." and exits 0, or says what failed and exits 1.  With the arguments `plan <Nmax> <lmax>`
// it prints the header's plan of that global layout instead (print_plan below).  May be built with
// -fsanitize=address,undefined and run as it is.
#include "tamcmc_seismic.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static bool same_bits(const double a, const double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static TmLayout make_layout(int family, int Nmax, int lmax, const int Nfl[4])
{
    TmLayout L{};
    L.model_case = family == TM_FAM_GLOBAL ? 2 : 11; L.family = family; L.Nmax = Nmax; L.lmax = lmax;
    int nf = 0;
    for (int l = 0; l < 4; l++) { L.Nfl[l] = Nfl[l]; nf += Nfl[l]; }
    L.off_f[0] = Nmax + lmax;
    for (int l = 1; l < 4; l++) L.off_f[l] = L.off_f[l - 1] + Nfl[l - 1];
    L.n_mult = family == TM_FAM_GLOBAL ? Nmax * (lmax + 1) : nf;
    return L;
}

struct Table {
    std::vector<TmMtCol> cols;
    std::vector<double> row;
    int fcol(int l, int n) const
    {
        for (size_t c = 0; c < cols.size(); c++)
            if (cols[c].kind == TM_MT_FREQ && cols[c].l == l && cols[c].order == n) return (int)c;
        return -1;
    }
};

// a row on the asymptotic pattern: order n of degree l is radial index n of its block, n0 the absolute order of index 0
static Table asymptotic(const TmLayout &L, double dnu, double eps, double D0, int n0)
{
    Table T;
    T.cols.resize((size_t)tm_mt_layout(L, nullptr));
    tm_mt_layout(L, T.cols.data());
    T.row.assign(T.cols.size(), 0.0);
    for (size_t c = 0; c < T.cols.size(); c++) {
        const TmMtCol &k = T.cols[c];
        if (k.kind == TM_MT_FREQ) T.row[c] = dnu * ((double)(n0 + k.order) + 0.5 * k.l + eps) - (double)(k.l * (k.l + 1)) * D0;
        else if (k.kind == TM_MT_AMPLITUDE) T.row[c] = 1.0 + 0.25 * k.order;
        else T.row[c] = 0.5 + (double)c;
    }
    return T;
}

static int count_kind(const TmSeisPlan &P, int kind, int l = -2)
{
    int n = 0;
    for (const TmMtCol &c : P.cols) n += c.kind == kind && (l == -2 || c.l == l);
    return n;
}

static long check_plan(const char *tag, const TmLayout &L, const int N[4])
{
    const double dnu = 103.25, eps = 1.37, D0 = 1.1;
    const int n0 = 14;
    const Table T = asymptotic(L, dnu, eps, D0, n0);
    TmSeisPlan P;
    const int rc = tm_seis_plan(T.cols.data(), (int)T.cols.size(), T.row.data(), P);
    CHECK(rc == 0, "%s: plan refused", tag);
    if (rc != 0) return 0;
    CHECK(P.n_radial == N[0] && P.n_unassigned == 0, "%s: n_radial %d unassigned %d", tag, P.n_radial, P.n_unassigned);
    CHECK(P.n_base == n0 && fabs(P.dnu_ref - dnu) < 1e-9 && fabs(P.eps_ref - eps) < 1e-9, "%s: n_base %lld dnu %.17g eps %.17g", tag, P.n_base, P.dnu_ref, P.eps_ref);
    auto pairs = [](int a) { return a > 1 ? a - 1 : 0; };
    auto both = [&](int la, int lb, int shift) {     // orders n with (n, la) and (n - shift, lb) present
        int n = 0;
        for (int k = 0; k < N[la]; k++) n += k - shift >= 0 && k - shift < N[lb];
        return n;
    };
    int fits = 0, dn = 0, d2 = 0;
    for (int l = 0; l < 4; l++) { fits += N[l] >= 2; dn += pairs(N[l]); d2 += N[l] > 2 ? N[l] - 2 : 0; }
    CHECK(count_kind(P, TM_SEIS_DNU_FIT) == fits && count_kind(P, TM_SEIS_EPSILON) == 1 && count_kind(P, TM_SEIS_NUMAX) == 1, "%s: fits", tag);
    CHECK(count_kind(P, TM_SEIS_DNU_NL) == dn && count_kind(P, TM_SEIS_D2NU) == d2, "%s: dnu_nl %d d2nu %d", tag, count_kind(P, TM_SEIS_DNU_NL), count_kind(P, TM_SEIS_D2NU));
    const int w02 = both(0, 2, 1), w13 = both(1, 3, 1);
    int w01 = 0, w10 = 0, r02 = 0, r13 = 0;
    for (int k = 0; k < 80; k++) {
        const bool h0m = k - 1 >= 0 && k - 1 < N[0], h0 = k < N[0], h0p = k + 1 < N[0], h1m = k - 1 >= 0 && k - 1 < N[1], h1 = k < N[1], h1p = k + 1 < N[1];
        w01 += h0m && h1m && h0 && h1 && h0p;
        w10 += h1m && h0 && h1 && h0p && h1p;
        r02 += h0 && k - 1 >= 0 && k - 1 < N[2] && h1 && h1m;
        r13 += h1 && k - 1 >= 0 && k - 1 < N[3] && h0p && h0;
    }
    CHECK(count_kind(P, TM_SEIS_D02) == w02 && count_kind(P, TM_SEIS_D13) == w13 && count_kind(P, TM_SEIS_D01) == w01 && count_kind(P, TM_SEIS_D10) == w10,
          "%s: d02 %d d13 %d d01 %d d10 %d", tag, count_kind(P, TM_SEIS_D02), count_kind(P, TM_SEIS_D13), count_kind(P, TM_SEIS_D01), count_kind(P, TM_SEIS_D10));
    CHECK(count_kind(P, TM_SEIS_R02) == r02 && count_kind(P, TM_SEIS_R01) == w01 && count_kind(P, TM_SEIS_R13) == r13 && count_kind(P, TM_SEIS_R10) == w10, "%s: ratios", tag);
    // order of the kinds, then l, then n; CSR; sources
    const int ni = P.n_index();
    CHECK((int)P.first.size() == ni + 1 && (int)P.n_num.size() == ni && (int)P.offset.size() == ni && P.first[0] == 0 && P.first[(size_t)ni] == P.n_terms(), "%s: csr", tag);
    CHECK(P.wsrc.size() == P.src.size() && P.coef.size() == P.src.size(), "%s: term arrays", tag);
    for (int j = 0; j < ni; j++) {
        const TmMtCol &c = P.cols[(size_t)j];
        if (j > 0) {
            const TmMtCol &b = P.cols[(size_t)j - 1];
            const bool per_l = c.kind == TM_SEIS_DNU_FIT || c.kind == TM_SEIS_DNU_NL || c.kind == TM_SEIS_D2NU;
            CHECK(b.kind < c.kind || (b.kind == c.kind && (per_l ? (b.l < c.l || (b.l == c.l && b.order < c.order)) : b.order < c.order)), "%s: order at %d", tag, j);
        }
        CHECK(c.mult == -1 && c.m == 0 && c.param_index == -1, "%s: col %d", tag, j);
        const int t0 = P.first[(size_t)j], t2 = P.first[(size_t)j + 1], t1 = t0 + P.n_num[(size_t)j];
        CHECK(t0 < t1 && t1 <= t2, "%s: range of %d", tag, j);
        for (int t = t0; t < t2; t++) {
            const int s = P.src[(size_t)t], w = P.wsrc[(size_t)t];
            CHECK(s == TM_SEIS_ONE || (s >= 0 && s < (int)T.cols.size() && T.cols[(size_t)s].kind == TM_MT_FREQ), "%s: src of %d", tag, j);
            CHECK(w == -1 || (w >= 0 && w < (int)T.cols.size() && T.cols[(size_t)w].kind == TM_MT_AMPLITUDE && T.cols[(size_t)w].l == 0), "%s: wsrc of %d", tag, j);
            CHECK((w >= 0) == (c.kind == TM_SEIS_NUMAX) && (s == TM_SEIS_ONE) == (c.kind == TM_SEIS_NUMAX && t >= t1), "%s: weights of %d", tag, j);
        }
        // the value on the exact pattern
        const double v = tm_seis_eval(T.row.data(), P.src.data(), P.wsrc.data(), P.coef.data(), t0, t1, t2, P.offset[(size_t)j]);
        double want = NAN;
        const int k = c.order - (int)P.n_base;
        switch (c.kind) {
        case TM_SEIS_DNU_FIT: case TM_SEIS_DNU_NL: want = dnu; break;
        case TM_SEIS_EPSILON: want = eps; break;
        case TM_SEIS_D2NU: want = 0.0; break;
        case TM_SEIS_D02: want = 6.0 * D0; break;
        case TM_SEIS_D13: want = 10.0 * D0; break;
        case TM_SEIS_D01: want = 2.0 * D0; break;
        case TM_SEIS_D10: want = 2.0 * D0; break;
        case TM_SEIS_R02: want = 6.0 * D0 / dnu; break;
        case TM_SEIS_R13: want = 10.0 * D0 / dnu; break;
        case TM_SEIS_R01: want = 2.0 * D0 / dnu; break;
        case TM_SEIS_R10: want = 2.0 * D0 / dnu; break;
        default: break;
        }
        if (c.kind != TM_SEIS_NUMAX) CHECK(fabs(v - want) < 1e-8, "%s: col %d kind %d value %.17g want %.17g", tag, j, c.kind, v, want);
        if (c.kind == TM_SEIS_D02) {
            const int a = T.fcol(0, k), b = T.fcol(2, k - 1);
            CHECK(a >= 0 && b >= 0 && P.src[(size_t)t0] == a && P.src[(size_t)t0 + 1] == b && same_bits(v, T.row[(size_t)a] - T.row[(size_t)b]), "%s: d02 at %d", tag, j);
        }
        if (c.kind == TM_SEIS_DNU_NL) {
            const int a = T.fcol(c.l, k), b = T.fcol(c.l, k - 1);
            CHECK(a >= 0 && b >= 0 && same_bits(v, T.row[(size_t)a] - T.row[(size_t)b]), "%s: dnu_nl at %d", tag, j);
        }
        if (c.kind == TM_SEIS_NUMAX) {
            long double nu = 0.0L, den = 0.0L;
            for (int n = 0; n < N[0]; n++) { const int f = T.fcol(0, n); const long double A = T.row[(size_t)f + 3]; nu += (long double)T.row[(size_t)f] * A * A; den += A * A; }
            CHECK(fabsl((long double)v - nu / den) < 1e-9L, "%s: numax %.17g", tag, v);
        }
    }
    return ni;
}

static void check_ls()
{
    const std::vector<std::vector<long long>> ladders = {{0, 1}, {0, 1, 2}, {-1, 0, 1, 2, 3}, {0, 2, 3, 7}, {3, 4, 9, 10, 11, 30}};
    std::vector<std::vector<long long>> all = ladders;
    std::vector<long long> longl;
    for (int i = 0; i < 70; i++) longl.push_back(i);
    all.push_back(longl);
    for (const auto &k : all) {
        std::vector<double> c, a;
        tm_seis_ls(k, c, a);
        long double sc = 0, sck = 0, sa = 0, sak = 0, mag = 0;
        for (size_t i = 0; i < k.size(); i++) {
            sc += c[i]; sck += (long double)c[i] * k[i]; sa += a[i]; sak += (long double)a[i] * k[i];
            mag += fabsl((long double)c[i] * k[i]) + fabsl((long double)a[i] * k[i]) + fabsl((long double)a[i]);
        }
        const long double tol = 8.0L * 2.220446049250313e-16L * (1.0L + mag);
        CHECK(fabsl(sc) <= tol && fabsl(sck - 1.0L) <= tol && fabsl(sa - 1.0L) <= tol && fabsl(sak) <= tol, "ls of %zu orders: %Lg %Lg %Lg %Lg", k.size(), sc, sck - 1.0L, sa - 1.0L, sak);
    }
}

static void check_assignment()
{
    const int f[4] = {6, 6, 0, 0};
    const TmLayout L = make_layout(TM_FAM_GLOBAL, 6, 1, f);
    const double dnu = 100.0, eps = 1.2;
    Table T = asymptotic(L, dnu, eps, 0.0, 10);
    TmSeisPlan P;
    CHECK(tm_seis_plan(T.cols.data(), (int)T.cols.size(), T.row.data(), P) == 0 && P.n_unassigned == 0, "clean ladder");
    const int full = P.n_index();
    const int c12 = T.fcol(1, 2);
    // the fitted line is the exact ladder here (six radial modes on it): u of (l = 1, n = 2) is 2 + shift / dnu
    Table S = T;
    S.row[(size_t)c12] = T.row[(size_t)c12] + 0.34 * dnu;
    CHECK(tm_seis_plan(S.cols.data(), (int)S.cols.size(), S.row.data(), P) == 0 && P.n_unassigned == 0 && P.n_index() == full, "0.34: unassigned %d", P.n_unassigned);
    S.row[(size_t)c12] = T.row[(size_t)c12] - 0.34 * dnu;
    CHECK(tm_seis_plan(S.cols.data(), (int)S.cols.size(), S.row.data(), P) == 0 && P.n_unassigned == 0, "-0.34: unassigned %d", P.n_unassigned);
    S.row[(size_t)c12] = T.row[(size_t)c12] + 0.36 * dnu;
    CHECK(tm_seis_plan(S.cols.data(), (int)S.cols.size(), S.row.data(), P) == 0 && P.n_unassigned == 1 && P.n_index() < full, "0.36: unassigned %d", P.n_unassigned);
    for (int t = 0; t < P.n_terms(); t++) CHECK(P.src[(size_t)t] != c12, "0.36: the unassigned mode is a source");
    S.row[(size_t)c12] = T.row[(size_t)c12] - 0.36 * dnu;
    CHECK(tm_seis_plan(S.cols.data(), (int)S.cols.size(), S.row.data(), P) == 0 && P.n_unassigned == 1, "-0.36: unassigned %d", P.n_unassigned);
    // a duplicate order: (1, 2) moved next to (1, 3); both are unassigned
    S.row[(size_t)c12] = T.row[(size_t)T.fcol(1, 3)] - 0.1 * dnu;
    CHECK(tm_seis_plan(S.cols.data(), (int)S.cols.size(), S.row.data(), P) == 0 && P.n_unassigned == 2, "duplicate: unassigned %d", P.n_unassigned);
    for (int t = 0; t < P.n_terms(); t++) CHECK(P.src[(size_t)t] != c12 && P.src[(size_t)t] != T.fcol(1, 3), "duplicate: an unassigned mode is a source");
    // a mode a million orders off the ladder (on the pattern, so assigned): three more orders to look at, not a range to walk;
    // it stays in its degree's fit and leaves the separations that needed order 2
    S = T;
    S.row[(size_t)c12] = T.row[(size_t)c12] + 1.0e6 * dnu;
    CHECK(tm_seis_plan(S.cols.data(), (int)S.cols.size(), S.row.data(), P) == 0 && P.n_unassigned == 0 && P.n_index() < full, "far mode: %d columns", P.n_index());
    for (int j = 0; j < P.n_index(); j++)
        for (int t = P.first[(size_t)j]; t < P.first[(size_t)j + 1]; t++)
            CHECK(P.src[(size_t)t] != c12 || P.cols[(size_t)j].kind == TM_SEIS_DNU_FIT, "far mode: a source of column %d", j);
    // a radial gap: the upper three radial modes one order up
    S = T;
    for (int n = 3; n < 6; n++) S.row[(size_t)T.fcol(0, n)] += dnu;
    CHECK(tm_seis_plan(S.cols.data(), (int)S.cols.size(), S.row.data(), P) == 1, "radial gap accepted");
    S = T;
    S.row[(size_t)T.fcol(0, 1)] = NAN;
    CHECK(tm_seis_plan(S.cols.data(), (int)S.cols.size(), S.row.data(), P) == 1, "NaN radial accepted");
    // radial modes stored out of order are sorted by frequency
    S = T;
    std::swap(S.row[(size_t)T.fcol(0, 1)], S.row[(size_t)T.fcol(0, 4)]);
    CHECK(tm_seis_plan(S.cols.data(), (int)S.cols.size(), S.row.data(), P) == 0 && P.n_index() == full, "unsorted radial modes");
    // a ridge whose first order would be 1e12: orders are 32-bit, refused
    S = T;
    for (size_t c = 0; c < S.cols.size(); c++) if (S.cols[c].kind == TM_MT_FREQ) S.row[c] += 1.0e14;
    CHECK(tm_seis_plan(S.cols.data(), (int)S.cols.size(), S.row.data(), P) == 1, "n_base of 1e12 accepted");
    const int g[4] = {2, 2, 0, 0};
    const TmLayout L2 = make_layout(TM_FAM_GLOBAL, 2, 1, g);
    const Table T2 = asymptotic(L2, dnu, eps, 0.0, 10);
    CHECK(tm_seis_plan(T2.cols.data(), (int)T2.cols.size(), T2.row.data(), P) == 1, "two radial modes accepted");
}

static void check_evaluator()
{
    const int f[4] = {9, 9, 9, 9};
    const TmLayout L = make_layout(TM_FAM_GLOBAL, 9, 3, f);
    Table T = asymptotic(L, 135.1, 1.45, 1.5, 12);
    TmSeisPlan P;
    CHECK(tm_seis_plan(T.cols.data(), (int)T.cols.size(), T.row.data(), P) == 0, "evaluator: plan");
    std::mt19937_64 g(20241);
    std::normal_distribution<double> N(0.0, 1.0);
    double worst = 0.0;
    for (int rep = 0; rep < 200; rep++) {
        std::vector<double> x = T.row;
        for (size_t c = 0; c < x.size(); c++)
            if (T.cols[c].kind == TM_MT_FREQ) x[c] += 0.8 * N(g); else if (T.cols[c].kind == TM_MT_AMPLITUDE) x[c] = fabs(2.0 + N(g));
        for (int j = 0; j < P.n_index(); j++) {
            const int t0 = P.first[(size_t)j], t2 = P.first[(size_t)j + 1], t1 = t0 + P.n_num[(size_t)j];
            const double v = tm_seis_eval(x.data(), P.src.data(), P.wsrc.data(), P.coef.data(), t0, t1, t2, P.offset[(size_t)j]);
            long double s[2] = {0.0L, 0.0L}, m[2] = {0.0L, 0.0L};
            for (int t = t0; t < t2; t++) {
                long double term = (long double)P.coef[(size_t)t] * (P.src[(size_t)t] >= 0 ? (long double)x[(size_t)P.src[(size_t)t]] : 1.0L);
                long double wt = 1.0L;
                if (P.wsrc[(size_t)t] >= 0) { const long double w = x[(size_t)P.wsrc[(size_t)t]]; term *= w * w; wt = P.src[(size_t)t] >= 0 ? 3.0L : 2.0L; }
                s[t >= t1] += term; m[t >= t1] += wt * fabsl(term);
            }
            long double want = s[0], sens = m[0];
            if (t2 > t1) { want = s[0] / s[1]; sens = m[0] / fabsl(s[1]) + fabsl(s[0]) * m[1] / (s[1] * s[1]); }
            want -= (long double)P.offset[(size_t)j];
            const long double bound = 10.0L * 0x1p-50L * sens;
            const double ratio = (double)(fabsl((long double)v - want) / bound);
            worst = ratio > worst ? ratio : worst;
            CHECK(ratio <= 1.0, "evaluator: col %d kind %d off by %.3g of the bound", j, P.cols[(size_t)j].kind, ratio);
        }
    }
    std::printf("ok seismic_core_check evaluator worst error / bound %.3g ", worst);
    // hand-made columns: a zero denominator, 0 / 0, offset 0
    const double x[4] = {3.0, 3.0, -0.0, 5.0};
    const int32_t src[4] = {0, 1, 3, 2}, wsrc[4] = {-1, -1, -1, -1};
    const double coef[4] = {1.0, -1.0, 1.0, 1.0};
    CHECK(same_bits(tm_seis_eval(x, src, wsrc, coef, 3, 4, 4, 0.0), 0.0) && same_bits(tm_seis_eval(x, src, wsrc, coef, 0, 2, 2, 0.0), 0.0), "sums from +0.0");
    const int32_t s2[4] = {3, 0, 1, 0};                       // 5 / (3 - 3), (3 - 3) / (3 - 3)
    const double c2[4] = {1.0, 1.0, -1.0, 1.0};
    CHECK(std::isinf(tm_seis_eval(x, s2, wsrc, c2, 0, 1, 3, 0.0)), "inf");
    const double cm[3] = {-1.0, 1.0, -1.0};
    CHECK(tm_seis_eval(x, s2, wsrc, cm, 0, 1, 3, 0.0) == -INFINITY || tm_seis_eval(x, s2, wsrc, cm, 0, 1, 3, 0.0) == INFINITY, "signed inf");
    const int32_t s3[4] = {0, 1, 0, 1};
    const double c3[4] = {1.0, -1.0, 1.0, -1.0};
    CHECK(std::isnan(tm_seis_eval(x, s3, wsrc, c3, 0, 2, 4, 0.0)), "0 / 0");
    CHECK(same_bits(tm_seis_eval(x, s3, wsrc, c3, 0, 2, 2, 1.5), -1.5), "offset");
    const int32_t one[1] = {TM_SEIS_ONE}, w3[1] = {3};
    const double c1[1] = {1.0};
    CHECK(same_bits(tm_seis_eval(x, one, w3, c1, 0, 1, 1, 0.0), 25.0), "the constant-one source");
}

// `seismic_core_check plan <Nmax> <lmax>`: the header's plan of the global layout on the ladder dnu = 100, eps = 1.2, D0 = 1,
// first order 10 -- one line per index column, `kind order l n_num n_den offset`, then per term ` src wsrc coef`, the doubles
// as hexadecimal floats -- for the comparison with tests/seismic_reference.py
static int print_plan(int Nmax, int lmax)
{
    int f[4] = {0, 0, 0, 0};
    for (int l = 0; l <= lmax && l < 4; l++) f[l] = Nmax;
    const TmLayout L = make_layout(TM_FAM_GLOBAL, Nmax, lmax, f);
    if (Nmax < 1 || lmax < 0 || lmax > 3 || L.n_mult > TM_MAXMULT) return 2;
    const Table T = asymptotic(L, 100.0, 1.2, 1.0, 10);
    TmSeisPlan P;
    if (tm_seis_plan(T.cols.data(), (int)T.cols.size(), T.row.data(), P) != 0) { std::printf("refused\n"); return 0; }
    std::printf("info %d %d %d %lld %a %a\n", P.n_index(), P.n_radial, P.n_unassigned, P.n_base, P.dnu_ref, P.eps_ref);
    for (int j = 0; j < P.n_index(); j++) {
        const TmMtCol &c = P.cols[(size_t)j];
        const int t0 = P.first[(size_t)j], t2 = P.first[(size_t)j + 1];
        std::printf("%d %d %d %d %d %a", c.kind, c.order, c.l, P.n_num[(size_t)j], t2 - t0 - P.n_num[(size_t)j], P.offset[(size_t)j]);
        for (int t = t0; t < t2; t++) std::printf(" %d %d %a", P.src[(size_t)t], P.wsrc[(size_t)t], P.coef[(size_t)t]);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && std::strcmp(argv[1], "plan") == 0) return print_plan(std::atoi(argv[2]), std::atoi(argv[3]));
    long cols = 0;
    int plans = 0;
    for (int lmax = 0; lmax <= 3; lmax++)
        for (int Nmax = 3; Nmax <= 5; Nmax++) {
            int f[4] = {0, 0, 0, 0};
            for (int l = 0; l <= lmax; l++) f[l] = Nmax;
            char tag[64];
            std::snprintf(tag, sizeof tag, "global lmax %d Nmax %d", lmax, Nmax);
            cols += check_plan(tag, make_layout(TM_FAM_GLOBAL, Nmax, lmax, f), f);
            plans++;
        }
    { const int f[4] = {12, 12, 12, 12}; const long n = check_plan("global lmax 3 Nmax 12", make_layout(TM_FAM_GLOBAL, 12, 3, f), f); CHECK(n > 64, "Nmax 12: %ld index columns", n); cols += n; plans++; }
    { const int f[4] = {70, 0, 0, 0}; cols += check_plan("global lmax 0 Nmax 70", make_layout(TM_FAM_GLOBAL, 70, 0, f), f); plans++; }
    { const int f[4] = {4, 3, 4, 2}; cols += check_plan("local 4 3 4 2", make_layout(TM_FAM_LOCAL, 0, 3, f), f); plans++; }
    check_ls();
    check_assignment();
    check_evaluator();
    if (failures) { std::printf("\n%d failures\n", failures); return 1; }
    std::printf("plans %d index columns %ld\n", plans, cols);
    return 0;
}
