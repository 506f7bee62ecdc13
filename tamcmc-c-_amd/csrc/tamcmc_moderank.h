// tamcmc_moderank.h -- rank-normalised diagnostics of the posterior mode table's columns (tamcmc_moderank_* in
// include/tamcmc_accel.h): bulk and tail effective sample size and the rank-normalised and folded split R-hat of Vehtari,
// Gelman, Simpson, Carpenter and Buerkner (2021), from the accepted rows the table keeps on the device, column-major.
//
// Everything below is plain C++17: the kernels (tamcmc_moderank.hip), the host side (tamcmc_moderank_api.cpp) and the
// stand-alone check (tests/cpp/moderank_core_check.cpp, built with g++) call these same functions.  The kernels' file
// includes this header under `#pragma clang fp contract(off)`; g++ builds it with -ffp-contract=off.
//
//   n        accepted rows, n >= 4; v_t = column c of the t-th accepted row; order is that of tmq_key (tamcmc_quantile.h)
//   rank2_t  = #{s : v_s < v_t} + #{s : v_s <= v_t} + 1: twice the average rank, an integer in [2, 2n]        tmr_bounds
//   z_t      a = 4 rank2_t - 3, D = 8 n + 2, b = D - a;  a < b: -g(a / D);  a > b: +g(b / D);  a = b: +0.0     tmr_z
//            g(q) = -Phi^-1(q), 0 < q < 1/2 (Blom's (r - 3/8) / (n + 1/4), the smaller tail inverted)          tmr_g
//   fold     med = 0.5 s_[(n-1)/2] + 0.5 s_[n/2] of the sorted column; f_t = |v_t - med|; zf_t = z of f's ranks   tmr_median, tmr_fold
//   tails    i05_t = (v_t <= Q05), i95_t = (v_t <= Q95) as 0.0 / 1.0, Q the order statistic of rank tmq_rank(0.05 | 0.95, n)
//   means    of each of the four series by tme_welford in t order, one owner per series
//   then the series table goes through tamcmc_modediag.h's lag and finish kernels as it is.
//
// Sort kernel's walk.  One workgroup of TM_MR_SORT_THREADS threads per column sorts the column's keys (keys only: a rank
// needs no permutation) by a bitonic network on P = tmr_padded(n) slots, the slots past n holding the largest key.  The
// network's stage (k, j) exchanges slots i and i + j (tmr_pair_lo) upwards where (i & k) = 0 (tmr_pair_up).  Stages with
// j < T = min(P, TM_MR_TILE) run on a tile of T keys held in LDS (64 KiB); stages with j >= T run on the column's key
// buffer in device memory, the workgroup waiting for itself between stages.  Every comparator of a stage touches two slots
// no other comparator of the stage touches, and exchanging equal keys changes nothing, so the result is the sorted column
// whatever the order of the threads.
//
// Transform kernel.  One thread per (column, t): two binary searches of key(v_t) in the sorted column (tmr_bounds), the same
// for key(f_t) in the sorted folded column, tmr_z of either, the two indicators.  Mean kernel: one thread per series.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "tamcmc_ess.h"
#include "tamcmc_modediag.h"
#include "tamcmc_quantile.h"

#define TMR_FN TME_FN

#define TM_MR_NOUT 8              // TAMCMC_MODERANK_NOUT
#define TM_MR_NSERIES 4           // TAMCMC_MODERANK_NSERIES
#define TM_MR_TILE 8192           // keys of a column held in LDS at a time, a power of two
#define TM_MR_LDS_BYTES (TM_MR_TILE * 8)   // the sort kernel's LDS: 65 536 bytes
#define TM_MR_SORT_THREADS 1024
#define TM_MR_THREADS 256         // transform kernel: one thread per sample
#define TM_MR_MEAN_THREADS 64     // mean kernel: one thread per series
#define TM_MR_MEAN_UNROLL 8       // loads in flight per series
#define TM_MR_DEFAULT_SCRATCH ((int64_t)256 << 20)

enum { TM_MR_Z = 0, TM_MR_ZFOLD, TM_MR_I05, TM_MR_I95 };                       // the series of a column, in this order
enum { TM_MR_ESS_BULK = 0, TM_MR_ESS_TAIL, TM_MR_RHAT, TM_MR_TAU_BULK, TM_MR_RHAT_BULK, TM_MR_RHAT_FOLD, TM_MR_ESS_Q05, TM_MR_ESS_Q95 };

// ---- g(q) = -Phi^-1(q), 0 < q < 1/2 ----
// A closed-form start (Acklam's rational approximations, relative error about 1e-9) and two Halley steps on
// F(z) = erfc(z / sqrt 2) / 2 - q:  r = F / phi(z),  z <- z + r / (1 - r z / 2).  Only + - x / sqrt log exp erfc.
TMR_FN double tmr_g(const double q)
{
    double x;
    if (q < 0.02425) {
        const double s = sqrt(-2.0 * log(q));
        x = (((((-7.784894002430293e-03 * s + -3.223964580411365e-01) * s + -2.400758277161838e+00) * s + -2.549732539343734e+00) * s +
              4.374664141464968e+00) * s + 2.938163982698783e+00) /
            ((((7.784695709041462e-03 * s + 3.224671290700398e-01) * s + 2.445134137142996e+00) * s + 3.754408661907416e+00) * s + 1.0);
    } else {
        const double u = q - 0.5, r = u * u;
        x = (((((-3.969683028665376e+01 * r + 2.209460984245205e+02) * r + -2.759285104469687e+02) * r + 1.383577518672690e+02) * r +
              -3.066479806614716e+01) * r + 2.506628277459239e+00) * u /
            (((((-5.447609879822406e+01 * r + 1.615858368580409e+02) * r + -1.556989798598866e+02) * r + 6.680131188771972e+01) * r +
              -1.328068155288572e+01) * r + 1.0);
    }
    double z = -x;
    for (int it = 0; it < 2; it++) {
        const double F = 0.5 * erfc(z * 0.70710678118654752440) - q;
        const double phi = 0.39894228040143267794 * exp(-0.5 * (z * z));
        const double r = F / phi;
        z = z + r / (1.0 - 0.5 * (r * z));
    }
    return z;
}

// z of rank2 among n: exact integers a, b, D < 2^53; one division
TMR_FN double tmr_z(const long long rank2, const long long n)
{
    const long long a = 4 * rank2 - 3, D = 8 * n + 2, b = D - a;
    if (a == b) return 0.0;
    const double g = tmr_g((double)(a < b ? a : b) / (double)D);
    return a < b ? -g : g;
}

TMR_FN double tmr_median(const uint64_t *sorted, const long long n)
{
    return 0.5 * tmq_unkey(sorted[(n - 1) / 2]) + 0.5 * tmq_unkey(sorted[n / 2]);
}
TMR_FN double tmr_fold(const double v, const double med) { return fabs(v - med); }
TMR_FN double tmr_indicator(const double v, const double Q) { return v <= Q ? 1.0 : 0.0; }

// lower and upper bound of key among sorted[0 ... n - 1]: *lb = #{s < key}, *ub = #{s <= key}; rank2 = *lb + *ub + 1.
// The two searches advance together: their loads are independent.
TMR_FN void tmr_bounds(const uint64_t *sorted, const long long n, const uint64_t key, long long *lb, long long *ub)
{
    long long lo1 = 0, hi1 = n, lo2 = 0, hi2 = n;
    while (lo1 < hi1 || lo2 < hi2) {
        const long long m1 = lo1 + ((hi1 - lo1) >> 1), m2 = lo2 + ((hi2 - lo2) >> 1);
        const uint64_t s1 = lo1 < hi1 ? sorted[m1] : 0, s2 = lo2 < hi2 ? sorted[m2] : 0;
        if (lo1 < hi1) { if (s1 < key) lo1 = m1 + 1; else hi1 = m1; }
        if (lo2 < hi2) { if (s2 <= key) lo2 = m2 + 1; else hi2 = m2; }
    }
    *lb = lo1; *ub = lo2;
}
TMR_FN long long tmr_rank2(const uint64_t *sorted, const long long n, const uint64_t key)
{
    long long lb, ub;
    tmr_bounds(sorted, n, key, &lb, &ub);
    return lb + ub + 1;
}

// ---- the sorting network ----
// slots of a column of n keys: the smallest power of two >= max(n, 2)
TMR_FN long long tmr_padded(const long long n)
{
    long long P = 2;
    while (P < n) P <<= 1;
    return P;
}
TMR_FN long long tmr_tile(const long long P) { return P < TM_MR_TILE ? P : (long long)TM_MR_TILE; }
// comparator p (0 <= p < P / 2) of a stage with distance j: its lower slot; the upper one is j above
TMR_FN long long tmr_pair_lo(const long long p, const long long j) { return ((p & ~(j - 1)) << 1) | (p & (j - 1)); }
// whether the comparator at slot i of the stages of block size k sorts upwards
TMR_FN bool tmr_pair_up(const long long i, const long long k) { return (i & k) == 0; }
TMR_FN void tmr_exchange(uint64_t *x, uint64_t *y, const bool up)
{
    const uint64_t a = *x, b = *y;
    if ((a > b) == up) { *x = b; *y = a; }
}
// One thread's comparators of stage (k, j), j < T, on a tile of T keys whose first slot is slot `base` of the column.
TMR_FN void tmr_tile_stage(uint64_t *tile, const int T, const long long base, const long long k, const int j, const int tid, const int nthreads)
{
    for (int p = tid; p < T / 2; p += nthreads) {
        const int lo = (int)tmr_pair_lo(p, j);
        tmr_exchange(tile + lo, tile + lo + j, tmr_pair_up(base + lo, k));
    }
}
// One thread's comparators of stage (k, j), j >= T, on the column's P slots.
TMR_FN void tmr_wide_stage(uint64_t *keys, const long long P, const long long k, const long long j, const int tid, const int nthreads)
{
    for (long long p = tid; p < P / 2; p += nthreads) {
        const long long lo = tmr_pair_lo(p, j);
        tmr_exchange(keys + lo, keys + lo + j, tmr_pair_up(lo, k));
    }
}

// device bytes of one column of a chunk: two key buffers, four series, their means, lag products, finish arrays and cut,
// med / Q05 / Q95 and the column's index (the header comment of tamcmc_moderank_diag states them)
inline size_t tmr_col_bytes(const long long n, const int L)
{
    return 2 * (size_t)tmr_padded(n) * sizeof(uint64_t) + TM_MR_NSERIES * ((size_t)n + 1 + (size_t)(L + 1) + TM_MD_NFIN) * sizeof(double) +
           3 * sizeof(double) + TM_MR_NSERIES * sizeof(int32_t) + sizeof(int32_t);
}

// ---- the plain statements ----
struct TmrTotals {                // tamcmc_moderank_totals
    int64_t n_used, lag;
    double min_ess_bulk, min_ess_tail, max_rhat;
    int64_t col_min_ess_bulk, col_min_ess_tail, col_max_rhat, n_truncated, n_constant, n_rhat_high;
};
// the smaller (larger) of two, a NaN skipped, NaN if both are
TMR_FN double tmr_min_skip(const double a, const double b) { return a != a ? b : (b != b ? a : (b < a ? b : a)); }
TMR_FN double tmr_max_skip(const double a, const double b) { return a != a ? b : (b != b ? a : (b > a ? b : a)); }
// totals over the selection in its order; cols: the table's column of entry k (NULL: k itself)
inline TmrTotals tmr_totals(const int n_sel, const int32_t *cols, const long long n, const int L, const double *ess_bulk, const double *ess_tail,
                            const double *rhat, const int32_t *cut_bulk, const double *A0_bulk)
{
    TmrTotals t{};
    t.n_used = n; t.lag = L;
    t.min_ess_bulk = t.min_ess_tail = t.max_rhat = (double)NAN;
    t.col_min_ess_bulk = t.col_min_ess_tail = t.col_max_rhat = -1;
    for (int k = 0; k < n_sel; k++) {
        const int64_t c = cols ? cols[k] : k;
        if (t.col_min_ess_bulk < 0 ? !(ess_bulk[k] != ess_bulk[k]) : ess_bulk[k] < t.min_ess_bulk) { t.min_ess_bulk = ess_bulk[k]; t.col_min_ess_bulk = c; }
        if (t.col_min_ess_tail < 0 ? !(ess_tail[k] != ess_tail[k]) : ess_tail[k] < t.min_ess_tail) { t.min_ess_tail = ess_tail[k]; t.col_min_ess_tail = c; }
        if (t.col_max_rhat < 0 ? !(rhat[k] != rhat[k]) : rhat[k] > t.max_rhat) { t.max_rhat = rhat[k]; t.col_max_rhat = c; }
        if (cut_bulk[k] == L + 1) t.n_truncated++;
        if (A0_bulk[k] == 0.0) t.n_constant++;
        if (rhat[k] > 1.01) t.n_rhat_high++;
    }
    return t;
}

#if defined(TMR_HOST_FEED)
// The sort kernel's walk on the host, tile by tile, stage by stage and thread by thread (tests/cpp/moderank_core_check.cpp).
// keys: P slots, the first n the column's keys in any order, the rest the largest key.
#include <vector>
inline void tmr_host_sort(uint64_t *keys, const long long P, const int nthreads)
{
    const int T = (int)tmr_tile(P);
    std::vector<uint64_t> tile((size_t)T);
    for (long long base = 0; base < P; base += T) {
        for (int i = 0; i < T; i++) tile[(size_t)i] = keys[base + i];
        for (long long k = 2; k <= T; k <<= 1)
            for (int j = (int)(k >> 1); j >= 1; j >>= 1)
                for (int tid = 0; tid < nthreads; tid++) tmr_tile_stage(tile.data(), T, base, k, j, tid, nthreads);
        for (int i = 0; i < T; i++) keys[base + i] = tile[(size_t)i];
    }
    for (long long k = 2 * (long long)T; k <= P; k <<= 1) {
        for (long long j = k >> 1; j >= T; j >>= 1)
            for (int tid = 0; tid < nthreads; tid++) tmr_wide_stage(keys, P, k, j, tid, nthreads);
        for (long long base = 0; base < P; base += T) {
            for (int i = 0; i < T; i++) tile[(size_t)i] = keys[base + i];
            for (int j = T >> 1; j >= 1; j >>= 1)
                for (int tid = 0; tid < nthreads; tid++) tmr_tile_stage(tile.data(), T, base, k, j, tid, nthreads);
            for (int i = 0; i < T; i++) keys[base + i] = tile[(size_t)i];
        }
    }
}
#endif

// ---- launch arguments (tamcmc_moderank.hip) ----
struct TmMrArgs {
    const double *table;          // [n_cols][max_samples]: the mode table's rows
    const int32_t *sel;           // [w] the chunk's columns, device memory
    uint64_t *keys;               // [2][w][P]: sorted keys of the values, of the folded values
    double *series;               // [TM_MR_NSERIES w][n]: series s of chunk column c at (TM_MR_NSERIES c + s) n
    double *mean;                 // [TM_MR_NSERIES w]
    double *medq;                 // [3][w]: med, Q05, Q95
    long long *rank2;             // NULL, or [2][w][n]: rank2 of the values, of the folded values
    long long n, max_samples, P;  // 4 <= n <= max_samples, P = tmr_padded(n)
    long long r05, r95;           // tmq_rank(0.05, n), tmq_rank(0.95, n), formed on the host
    int32_t w, pad;
};
// what the sort kernel reads (table, sel, n, max_samples, P, w) and writes (keys), and the two ranks every launch checks; the
// transform and mean kernels' arrays are left NULL
inline TmMrArgs tmr_sort_args(const double *table, const int32_t *sel, uint64_t *keys, const long long n, const long long max_samples,
                              const long long P, const int w)
{
    TmMrArgs a{};
    a.table = table; a.sel = sel; a.keys = keys; a.n = n; a.max_samples = max_samples; a.P = P; a.w = w;
    a.r05 = (long long)tmq_rank(0.05, (int64_t)n); a.r95 = (long long)tmq_rank(0.95, (int64_t)n);
    return a;
}

int tm_launch_moderank_sort(const TmMrArgs &a, int fold, void *stream);      // each returns a hipError_t
int tm_launch_moderank_transform(const TmMrArgs &a, void *stream);
int tm_launch_moderank_mean(const TmMrArgs &a, void *stream);
