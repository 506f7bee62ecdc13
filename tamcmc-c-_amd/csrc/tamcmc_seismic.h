// tamcmc_seismic.h -- the seismic indices of the posterior mode table (tamcmc_modetable_indices_* in
// include/tamcmc_accel_seismic.h): per stored sample the large separation and the offset of the radial ridge, nu_max, the
// per-order separations and second differences, the small separations d02, d13, d01, d10 and the frequency ratios r02, r01,
// r13, r10 of Roxburgh & Vorontsov (2003), appended to the table as further columns so that every statistic and
// diagnostic the table has for its own columns serves them too.
//
// Everything below is plain C++17: the kernel (tamcmc_seismic.hip), the host side of the C ABI (tamcmc_seismic_api.cpp)
// and the stand-alone check (tests/cpp/seismic_core_check.cpp, built with g++) call the same functions.
//
// An index column is a fixed expression of the base columns x[] of the same row,
//     value = num / den - offset,
// num and den ordered lists of terms.  A term is coef * x[src]; with a weight column wsrc >= 0 it is
// (coef * x[src]) * (x[wsrc] * x[wsrc]).  src = TM_SEIS_ONE (-1) is the constant-one pseudo-source: x[src] reads 1.0 (the
// denominator of nu_max is a sum of A_k^2 alone: coef 1, src TM_SEIS_ONE, wsrc the amplitude).  An empty den: no division.
// offset = 0: no subtraction.  tm_seis_eval states the arithmetic once: acc = 0.0; per term in order t = coef * x[src],
// t = t * (w * w) if weighted, acc = acc + t; then one division, then one subtraction.  Only + - * /, never contracted
// (the kernel's file sets the pragma, the host builds pass -ffp-contract=off), so the device, g++ and numpy float64 give
// the same bits.  The order of addition is part of the result: a fit of any length is one serial loop.
//
// The plan (tm_seis_plan) is built once from a reference row, a derived row of the table's base columns:
//   radial modes   the l = 0 freq columns sorted by reference frequency (ties: column order); ladder index k = 0, 1, ...
//                  is the position.  Fewer than 3: refused.  The unweighted straight line through (k, nu_ref) -- slope
//                  b_ref = sum c_i nu_i, intercept a_ref = sum a_i nu_i with the least-squares coefficients below -- must
//                  have a positive finite slope and no residual above 0.25 b_ref (a missing order): refused otherwise.
//                  n_base = floor(a_ref / b_ref - 0.5), refused at |n_base| >= 1e9 (orders are 32-bit); the absolute order
//                  is n = n_base + k, so the reference row's epsilon = a_ref / b_ref - n_base lies in [0.5, 1.5).
//   l >= 1         u = (nu_ref - a_ref) / b_ref - l / 2, k = rint(u).  The mode is assigned order k iff |u - k| <= 0.35
//                  and no other mode of the same degree has the same rint(u) (then every one of them is unassigned).
//                  Unassigned modes (mixed modes, modes far off the asymptotic pattern) are counted and take part in no
//                  column; a column that would need an unassigned or absent mode is not created.
//   least squares  for the assigned orders k_1 < ... < k_T of a degree, every sum in that order in double:
//                  kbar = (sum k_i) / T, S = sum (k_i - kbar)^2, c_i = (k_i - kbar) / S, a_i = 1 / T - kbar * c_i.
//   columns, in this order (kind; per what; expression), nu_{n,l} the freq column of the mode of degree l and order n:
//     DNU_FIT   degree l with T >= 2 assigned modes   sum c_i nu_{k_i,l}
//     EPSILON   chain                                  (sum a_i nu_{k_i,0}) / (sum c_i nu_{k_i,0}) - n_base
//     NUMAX     chain                                  (sum nu_k A_k^2) / (sum A_k^2) over the radial modes, A the amplitude column
//     DNU_NL    (l, n), l ascending then n             nu_{n,l} - nu_{n-1,l}
//     D2NU      (l, n)                                 nu_{n+1,l} - 2 nu_{n,l} + nu_{n-1,l}
//     D02       n                                      nu_{n,0} - nu_{n-1,2}
//     D13       n                                      nu_{n,1} - nu_{n-1,3}
//     D01       n     0.125 nu_{n-1,0} - 0.5 nu_{n-1,1} + 0.75 nu_{n,0} - 0.5 nu_{n,1} + 0.125 nu_{n+1,0}
//     D10       n    -0.125 nu_{n-1,1} + 0.5 nu_{n,0} - 0.75 nu_{n,1} + 0.5 nu_{n+1,0} - 0.125 nu_{n+1,1}
//     R02, R01  n     the numerators of D02 and D01 over nu_{n,1} - nu_{n-1,1}
//     R13, R10  n     the numerators of D13 and D10 over nu_{n+1,0} - nu_{n,0}
//   Terms stand in the order written.  TmMtCol of an index column: mult = -1, order = the absolute n (-1 for DNU_FIT,
//   EPSILON, NUMAX), l = the degree (DNU_FIT, DNU_NL, D2NU), the first degree of the pair (D02 and R02: 0, D13 and R13: 1,
//   D01 and R01: 0, D10 and R10: 1), -1 for EPSILON and NUMAX; m = 0, param_index = -1.
#pragma once
#include <math.h>
#include <stdint.h>

#include "tamcmc_modetable.h"

enum {                            // TAMCMC_MODETABLE_* of include/tamcmc_accel_seismic.h, after TM_MT_H_M
    TM_SEIS_DNU_FIT = TM_MT_NKINDS, TM_SEIS_EPSILON, TM_SEIS_NUMAX, TM_SEIS_DNU_NL, TM_SEIS_D2NU,
    TM_SEIS_D02, TM_SEIS_D13, TM_SEIS_D01, TM_SEIS_D10, TM_SEIS_R02, TM_SEIS_R01, TM_SEIS_R13, TM_SEIS_R10,
    TM_SEIS_NKINDS
};
#define TM_SEIS_ONE (-1)          // src of a term: the constant 1.0
#define TM_SEIS_THREADS 64        // indices kernel: one wave per sample, lanes loop over the index columns
#define TM_SEIS_MARGIN 0.35       // |u - rint(u)| of an assigned mode of degree >= 1, at most
#define TM_SEIS_GAP 0.25          // residual of a radial mode over b_ref, at most
#define TM_SEIS_LDS_MAX (60 * 1024)   // bytes of base columns the kernel stages per sample, at most

// One index column: terms [t0, t1) are num, [t1, t2) den.
TM_HD inline double tm_seis_sum(const double *x, const int32_t *src, const int32_t *wsrc, const double *coef, const int t0, const int t1)
{
    double acc = 0.0;
    for (int t = t0; t < t1; t++) {
        const int s = src[t], ws = wsrc[t];
        double v = coef[t] * (s >= 0 ? x[s] : 1.0);
        if (ws >= 0) { const double w = x[ws]; v = v * (w * w); }
        acc = acc + v;
    }
    return acc;
}
TM_HD inline double tm_seis_eval(const double *x, const int32_t *src, const int32_t *wsrc, const double *coef, const int t0, const int t1,
                                 const int t2, const double offset)
{
    double v = tm_seis_sum(x, src, wsrc, coef, t0, t1);
    if (t2 > t1) v = v / tm_seis_sum(x, src, wsrc, coef, t1, t2);
    if (offset != 0.0) v = v - offset;
    return v;
}

// ---- launch arguments (tamcmc_seismic.hip) ----
struct TmSeisArgs {
    double *rows;                 // [B][n_cols]: base columns read, index columns written
    int32_t *status;              // [B] the derive kernel's; TAMCMC_CHAIN_OK becomes TAMCMC_CHAIN_NAN when an index column is a NaN
    const int32_t *first;         // [n_index + 1] first term of a column (CSR)
    const int32_t *n_num;         // [n_index] terms of num; the rest of the column's range is den
    const int32_t *src, *wsrc;    // [n_terms]
    const double *coef;           // [n_terms]
    const double *offset;         // [n_index]
    int32_t B, n_cols, n_base_cols, n_index;
};
int tm_launch_seismic(const TmSeisArgs &a, void *stream);      // returns a hipError_t

// ---- the plan (host) ----
#include <algorithm>
#include <vector>

struct TmSeisPlan {
    int n_base_cols = 0, n_radial = 0, n_unassigned = 0;
    long long n_base = 0;
    double dnu_ref = 0.0, eps_ref = 0.0, a_ref = 0.0;
    std::vector<TmMtCol> cols;                  // the index columns
    std::vector<int32_t> first, n_num;          // [n_index + 1], [n_index]
    std::vector<int32_t> src, wsrc;
    std::vector<double> coef, offset;
    int n_index() const { return (int)cols.size(); }
    int n_terms() const { return (int)src.size(); }
};

// least-squares coefficients of the orders k[0] < ... < k[T-1]: slope c, intercept a
inline void tm_seis_ls(const std::vector<long long> &k, std::vector<double> &c, std::vector<double> &a)
{
    const size_t T = k.size();
    double sk = 0.0;
    for (size_t i = 0; i < T; i++) sk = sk + (double)k[i];
    const double kbar = sk / (double)T;
    double S = 0.0;
    for (size_t i = 0; i < T; i++) { const double d = (double)k[i] - kbar; S = S + d * d; }
    c.resize(T); a.resize(T);
    for (size_t i = 0; i < T; i++) {
        c[i] = ((double)k[i] - kbar) / S;
        a[i] = 1.0 / (double)T - kbar * c[i];
    }
}

struct TmSeisMode { long long k; int fcol, acol; };     // order on the ladder, freq column, amplitude column

// The assignment: modes[l] = the assigned modes of degree l in ascending k.  Returns 0, or 1 (refused).
inline int tm_seis_assign(const TmMtCol *base, const int n_base_cols, const double *ref, std::vector<TmSeisMode> modes[4], TmSeisPlan &P)
{
    std::vector<int> fc[4];
    for (int c = 0; c < n_base_cols; c++)
        if (base[c].kind == TM_MT_FREQ && base[c].l >= 0 && base[c].l <= 3) fc[base[c].l].push_back(c);
    std::vector<int> &r = fc[0];
    std::stable_sort(r.begin(), r.end(), [&](int i, int j) { return ref[i] < ref[j]; });
    const size_t T = r.size();
    if (T < 3) return 1;
    std::vector<long long> k(T);
    for (size_t i = 0; i < T; i++) { k[i] = (long long)i; if (!(ref[r[i]] == ref[r[i]])) return 1; }
    std::vector<double> c, a;
    tm_seis_ls(k, c, a);
    double b_ref = 0.0, a_ref = 0.0;
    for (size_t i = 0; i < T; i++) b_ref = b_ref + c[i] * ref[r[i]];
    for (size_t i = 0; i < T; i++) a_ref = a_ref + a[i] * ref[r[i]];
    if (!(b_ref > 0.0) || !(b_ref < INFINITY) || !(fabs(a_ref) < INFINITY)) return 1;
    for (size_t i = 0; i < T; i++)
        if (!(fabs(ref[r[i]] - (a_ref + b_ref * (double)i)) <= TM_SEIS_GAP * b_ref)) return 1;
    const double nb = floor(a_ref / b_ref - 0.5);
    if (!(fabs(nb) < 1e9)) return 1;                 // with |k| < 1e9 below, n_base + k is an int32 (TmMtCol::order)
    P.n_radial = (int)T; P.n_base = (long long)nb; P.dnu_ref = b_ref; P.a_ref = a_ref; P.eps_ref = a_ref / b_ref - nb;
    P.n_unassigned = 0;
    modes[0].clear();
    for (size_t i = 0; i < T; i++) modes[0].push_back(TmSeisMode{(long long)i, r[i], r[i] + (TM_MT_AMPLITUDE - TM_MT_FREQ)});
    for (int l = 1; l <= 3; l++) {
        modes[l].clear();
        const size_t n = fc[l].size();
        std::vector<double> u(n), kk(n);
        for (size_t i = 0; i < n; i++) {
            u[i] = (ref[fc[l][i]] - a_ref) / b_ref - (double)l / 2.0;
            kk[i] = rint(u[i]);
        }
        for (size_t i = 0; i < n; i++) {
            bool ok = fabs(u[i] - kk[i]) <= TM_SEIS_MARGIN && fabs(kk[i]) < 1e9;     // (a NaN fails)
            for (size_t j = 0; j < n && ok; j++) ok = j == i || kk[j] != kk[i];
            if (ok) modes[l].push_back(TmSeisMode{(long long)kk[i], fc[l][i], fc[l][i] + (TM_MT_AMPLITUDE - TM_MT_FREQ)});
            else P.n_unassigned++;
        }
        std::sort(modes[l].begin(), modes[l].end(), [](const TmSeisMode &x, const TmSeisMode &y) { return x.k < y.k; });
    }
    return 0;
}

// The plan of a table whose base columns are base[0 ... n_base_cols - 1], from the reference row ref[0 ... n_base_cols - 1].
// Returns 0, or 1 (refused: fewer than 3 radial modes, a radial gap, a reference row that is not finite).
inline int tm_seis_plan(const TmMtCol *base, const int n_base_cols, const double *ref, TmSeisPlan &P)
{
    P = TmSeisPlan();
    P.n_base_cols = n_base_cols;
    std::vector<TmSeisMode> modes[4];
    if (tm_seis_assign(base, n_base_cols, ref, modes, P) != 0) return 1;
    auto find = [&](int l, long long k) -> int {             // the freq column of (l, k), or -1
        for (const TmSeisMode &m : modes[l]) if (m.k == k) return m.fcol;
        return -1;
    };
    struct Term { int src, wsrc; double coef; };
    auto add = [&](int kind, long long k, int l, const std::vector<Term> &num, const std::vector<Term> &den, double offset) {
        for (const Term &t : num) if (t.src < TM_SEIS_ONE || t.src >= n_base_cols) return;       // (a mode that is absent: no column)
        for (const Term &t : den) if (t.src < TM_SEIS_ONE || t.src >= n_base_cols) return;
        if (P.first.empty()) P.first.push_back(0);
        for (const Term &t : num) { P.src.push_back(t.src); P.wsrc.push_back(t.wsrc); P.coef.push_back(t.coef); }
        for (const Term &t : den) { P.src.push_back(t.src); P.wsrc.push_back(t.wsrc); P.coef.push_back(t.coef); }
        P.n_num.push_back((int32_t)num.size());
        P.first.push_back((int32_t)P.src.size());
        P.offset.push_back(offset);
        const bool ordered = kind != TM_SEIS_DNU_FIT && kind != TM_SEIS_EPSILON && kind != TM_SEIS_NUMAX;
        P.cols.push_back(TmMtCol{kind, -1, ordered ? (int32_t)(P.n_base + k) : -1, l, 0, -1});
    };
    const int ABSENT = -2;
    auto nu = [&](int l, long long k, double coef) { const int c = find(l, k); return Term{c < 0 ? ABSENT : c, -1, coef}; };
    const std::vector<Term> none;

    std::vector<double> c0, a0;
    for (int l = 0; l <= 3; l++) {
        const size_t T = modes[l].size();
        if (T < 2) continue;
        std::vector<long long> k(T);
        for (size_t i = 0; i < T; i++) k[i] = modes[l][i].k;
        std::vector<double> c, a;
        tm_seis_ls(k, c, a);
        std::vector<Term> num;
        for (size_t i = 0; i < T; i++) num.push_back(Term{modes[l][i].fcol, -1, c[i]});
        add(TM_SEIS_DNU_FIT, 0, l, num, none, 0.0);
        if (l == 0) { c0 = c; a0 = a; }
    }
    {
        std::vector<Term> num, den;
        for (size_t i = 0; i < modes[0].size(); i++) {
            num.push_back(Term{modes[0][i].fcol, -1, a0[i]});
            den.push_back(Term{modes[0][i].fcol, -1, c0[i]});
        }
        add(TM_SEIS_EPSILON, 0, -1, num, den, (double)P.n_base);
        num.clear(); den.clear();
        for (const TmSeisMode &m : modes[0]) {
            num.push_back(Term{m.fcol, m.acol, 1.0});
            den.push_back(Term{TM_SEIS_ONE, m.acol, 1.0});
        }
        add(TM_SEIS_NUMAX, 0, -1, num, den, 0.0);
    }
    // the orders a column can belong to, ascending: every assigned order and its two neighbours (a mode far off the
    // ladder is one more order, not a range to walk)
    std::vector<long long> orders;
    for (int l = 0; l <= 3; l++)
        for (const TmSeisMode &m : modes[l]) { orders.push_back(m.k - 1); orders.push_back(m.k); orders.push_back(m.k + 1); }
    std::sort(orders.begin(), orders.end());
    orders.erase(std::unique(orders.begin(), orders.end()), orders.end());
    for (int l = 0; l <= 3; l++)
        for (const long long k : orders) add(TM_SEIS_DNU_NL, k, l, {nu(l, k, 1.0), nu(l, k - 1, -1.0)}, none, 0.0);
    for (int l = 0; l <= 3; l++)
        for (const long long k : orders) add(TM_SEIS_D2NU, k, l, {nu(l, k + 1, 1.0), nu(l, k, -2.0), nu(l, k - 1, 1.0)}, none, 0.0);
    auto n02 = [&](long long k) { return std::vector<Term>{nu(0, k, 1.0), nu(2, k - 1, -1.0)}; };
    auto n13 = [&](long long k) { return std::vector<Term>{nu(1, k, 1.0), nu(3, k - 1, -1.0)}; };
    auto n01 = [&](long long k) { return std::vector<Term>{nu(0, k - 1, 0.125), nu(1, k - 1, -0.5), nu(0, k, 0.75), nu(1, k, -0.5), nu(0, k + 1, 0.125)}; };
    auto n10 = [&](long long k) { return std::vector<Term>{nu(1, k - 1, -0.125), nu(0, k, 0.5), nu(1, k, -0.75), nu(0, k + 1, 0.5), nu(1, k + 1, -0.125)}; };
    auto dl1 = [&](long long k) { return std::vector<Term>{nu(1, k, 1.0), nu(1, k - 1, -1.0)}; };
    auto dl0 = [&](long long k) { return std::vector<Term>{nu(0, k + 1, 1.0), nu(0, k, -1.0)}; };
    for (const long long k : orders) add(TM_SEIS_D02, k, 0, n02(k), none, 0.0);
    for (const long long k : orders) add(TM_SEIS_D13, k, 1, n13(k), none, 0.0);
    for (const long long k : orders) add(TM_SEIS_D01, k, 0, n01(k), none, 0.0);
    for (const long long k : orders) add(TM_SEIS_D10, k, 1, n10(k), none, 0.0);
    for (const long long k : orders) add(TM_SEIS_R02, k, 0, n02(k), dl1(k), 0.0);
    for (const long long k : orders) add(TM_SEIS_R01, k, 0, n01(k), dl1(k), 0.0);
    for (const long long k : orders) add(TM_SEIS_R13, k, 1, n13(k), dl0(k), 0.0);
    for (const long long k : orders) add(TM_SEIS_R10, k, 1, n10(k), dl0(k), 0.0);
    if (P.first.empty()) P.first.push_back(0);
    return 0;
}
