// tamcmc_modepdf.h -- marginal histograms, shortest (HPD) intervals and pair densities of the posterior mode table's
// columns (tamcmc_modepdf_* in include/tamcmc_accel_pdf.h), from the accepted rows the table keeps on the device,
// column-major.  Every result is an integer count or an order statistic of a column: nothing below rounds but the one
// subtraction and the one multiplication of the class rule and the one subtraction of a width.
//
// Everything below is plain C++17: the kernels (tamcmc_modepdf.hip), the host side (tamcmc_modepdf_api.cpp) and the
// stand-alone check (tests/cpp/modepdf_core_check.cpp, built with g++) call these same functions.  The kernels' file
// includes this header under `#pragma clang fp contract(off)`; g++ builds it with -ffp-contract=off.
//
//   class    s = (double)n_bins / (hi - lo), formed once per column on the host                                 tmp_scale
//            v < lo: below;  v > hi: above;  !(hi > lo): class 0;  else u = (v - lo) * s (one subtraction, then one
//            multiplication), class = (int64)u, clamped to n_bins - 1 (v == hi, a product that rounds up)        tmp_class
//            Where hi - lo is so small that s overflows, u is +inf (the last class) or, at v == lo, 0 * inf: class 0.
//   range    an explicit range must be finite with hi >= lo and a finite hi - lo; a default range (the column's min
//            and max) that is not gets status TM_PDF_RANGE and no count                                         tmp_range_ok
//   edges    lo + (hi - lo) * ((double)b / n_bins), edge n_bins = hi exactly: for plots only.  They are NOT the count
//            rule: a value within an ulp of an edge is counted by tmp_class, whichever side the edge rounds to   tmp_edge
//   k        window length of mass m over n samples: (int64)ceil(m * (double)n) clamped to [1, n]               tmp_window
//   HPD      over the column sorted ascending in the order of tmq_key (-0 and +0 one value, returned as +0):
//            w_i = s[i + k - 1] - s[i], i = 0 ... n - k; the interval is the i of the least w_i under tmp_before: a NaN
//            width (inf - inf) after every other, then the smaller width, then the smaller i.  The order is total, so
//            no reduction tree can change the answer.
//   level    of mass m over the cells of a pair's counts: the largest t such that the cells with count >= t together
//            hold at least ceil(m * n_in) samples, n_in the samples inside the range; 0 where n_in = 0           tmp_level
//
// Histogram kernel.  One workgroup of TM_PDF_THREADS threads per selected column; n_bins uint32 counters (at most 16 KiB)
// and below / above in LDS, the column read with coalesced 8-byte loads, TM_PDF_UNROLL in flight per thread, added with LDS
// integer atomics (a wave whose active lanes all hit one counter adds their number once); the counters leave with plain
// stores and are widened on the host.  Pair kernel: one workgroup per pair, n_bins^2 counters of dynamic LDS (64 KiB at
// 128).  HPD kernel: one workgroup per (column, mass) on the sorted keys of tamcmc_moderank.hip's sort kernel.  Integer
// sums and a total order: no result depends on the order of arrival.  A column has fewer than 2^31 rows
// (tamcmc_modetable_create), so a uint32 counter cannot wrap.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "tamcmc_quantile.h"

#define TMP_FN TMQ_FN

#define TM_PDF_MAX_BINS 4096      // TAMCMC_MODEPDF_MAX_BINS
#define TM_PDF_MAX_BINS2D 128     // TAMCMC_MODEPDF_MAX_BINS2D
#define TM_PDF_MAX_PAIRS 1024     // TAMCMC_MODEPDF_MAX_PAIRS
#define TM_PDF_MAX_MASS 8         // TAMCMC_MODEPDF_MAX_MASS
#define TM_PDF_RANGE 1            // TAMCMC_MODEPDF_RANGE
#define TM_PDF_THREADS 512        // histogram and pair kernels
#define TM_PDF_UNROLL 4           // loads in flight per thread
#define TM_PDF_HPD_THREADS 256
#define TM_PDF_BELOW (-1)         // tmp_class: v < lo
#define TM_PDF_ABOVE (-2)         // tmp_class: v > hi
#define TM_PDF_DEFAULT_SCRATCH ((int64_t)256 << 20)

// ---- the class rule ----
TMP_FN bool tmp_range_ok(const double lo, const double hi)
{
    const double d = hi - lo;
    return lo - lo == 0.0 && hi - hi == 0.0 && hi >= lo && d - d == 0.0;      // (x - x is 0 for a finite x only)
}
TMP_FN double tmp_scale(const double lo, const double hi, const int n_bins) { return (double)n_bins / (hi - lo); }
TMP_FN long long tmp_class(const double v, const double lo, const double hi, const double s, const int n_bins)
{
    if (v < lo) return TM_PDF_BELOW;
    if (v > hi) return TM_PDF_ABOVE;
    if (!(hi > lo)) return 0;
    const double d = v - lo;
    const double u = d * s;
    if (!(u >= 0.0)) return 0;                          // 0 * inf: v == lo under a scale that overflowed
    if (u >= (double)n_bins) return n_bins - 1;
    return (long long)u;
}
// plot edge b of n_bins, 0 <= b <= n_bins: a host helper, not part of the count rule
inline double tmp_edge(const double lo, const double hi, const int b, const int n_bins)
{
    return b >= n_bins ? hi : lo + (hi - lo) * ((double)b / (double)n_bins);
}

// ---- the shortest interval ----
inline long long tmp_window(const double mass, const long long n)
{
    long long k = (long long)ceil(mass * (double)n);
    if (k < 1) k = 1;
    if (k > n) k = n;
    return k;
}
TMP_FN bool tmp_mass_ok(const double m) { return m > 0.0 && m <= 1.0; }      // (a NaN fails both)
// whether (wa, ia) comes before (wb, ib): NaN widths last, then the smaller width, then the smaller index
TMP_FN bool tmp_before(const double wa, const long long ia, const double wb, const long long ib)
{
    const bool na = wa != wa, nb = wb != wb;
    if (na != nb) return nb;
    if (!na && wa != wb) return wa < wb;
    return ia < ib;
}
TMP_FN double tmp_width(const uint64_t *sorted, const long long i, const long long k)
{
    return tmq_unkey(sorted[i + k - 1]) - tmq_unkey(sorted[i]);
}

// ---- the plain statements, over a column-major table: column c at table + c * stride ----
#include <algorithm>
#include <functional>
#include <vector>
// counts: n_bins entries; returns nothing else than what it writes
inline void tmp_host_hist(const double *col, const long long n, const double lo, const double hi, const int n_bins, int64_t *counts,
                          int64_t *below, int64_t *above)
{
    const double s = tmp_scale(lo, hi, n_bins);
    for (int b = 0; b < n_bins; b++) counts[b] = 0;
    *below = 0; *above = 0;
    for (long long t = 0; t < n; t++) {
        const long long c = tmp_class(col[t], lo, hi, s, n_bins);
        if (c == TM_PDF_BELOW) (*below)++;
        else if (c == TM_PDF_ABOVE) (*above)++;
        else counts[c]++;
    }
}
// counts: n_bins * n_bins entries, [a][b] with a the class of x
inline void tmp_host_hist2d(const double *x, const double *y, const long long n, const double lox, const double hix, const double loy,
                            const double hiy, const int n_bins, int64_t *counts, int64_t *outside)
{
    const double sx = tmp_scale(lox, hix, n_bins), sy = tmp_scale(loy, hiy, n_bins);
    for (size_t b = 0; b < (size_t)n_bins * (size_t)n_bins; b++) counts[b] = 0;
    *outside = 0;
    for (long long t = 0; t < n; t++) {
        const long long a = tmp_class(x[t], lox, hix, sx, n_bins), b = tmp_class(y[t], loy, hiy, sy, n_bins);
        if (a < 0 || b < 0) (*outside)++;
        else counts[(size_t)a * (size_t)n_bins + (size_t)b]++;
    }
}
// the sorted keys of a column (std::sort on tmq_key)
inline std::vector<uint64_t> tmp_host_sorted(const double *col, const long long n)
{
    std::vector<uint64_t> k((size_t)n);
    for (long long t = 0; t < n; t++) k[(size_t)t] = tmq_key(col[t]);
    std::sort(k.begin(), k.end());
    return k;
}
inline void tmp_host_hpd(const uint64_t *sorted, const long long n, const long long k, int64_t *start, double *lo, double *hi)
{
    long long bi = 0;
    double bw = tmp_width(sorted, 0, k);
    for (long long i = 1; i + k <= n; i++) {
        const double w = tmp_width(sorted, i, k);
        if (tmp_before(w, i, bw, bi)) { bw = w; bi = i; }
    }
    *start = bi; *lo = tmq_unkey(sorted[bi]); *hi = tmq_unkey(sorted[bi + k - 1]);
}
// level of one mass from the cells' counts sorted descending (tmp_sorted_counts), n_in their sum
inline std::vector<int64_t> tmp_sorted_counts(const int64_t *counts, const size_t cells)
{
    std::vector<int64_t> c(counts, counts + cells);
    std::sort(c.begin(), c.end(), std::greater<int64_t>());
    return c;
}
inline int64_t tmp_level(const std::vector<int64_t> &desc, const int64_t n_in, const double mass)
{
    if (n_in <= 0) return 0;
    const int64_t need = tmp_window(mass, n_in);
    int64_t cum = 0;
    for (const int64_t c : desc) {
        cum += c;
        if (cum >= need) return c;
    }
    return 0;
}

// device bytes of one column of an HPD chunk: its key slots, its index, and per mass start, lo, hi
inline size_t tmp_hpd_col_bytes(const long long P, const int n_mass)
{
    return (size_t)P * sizeof(uint64_t) + sizeof(int32_t) + (size_t)n_mass * 3 * sizeof(double);
}

// ---- launch arguments (tamcmc_modepdf.hip) ----
struct TmPdfHistArgs {
    const double *table;          // [n_cols][max_samples]: the mode table's rows
    const int32_t *sel;           // [n_sel] the selected columns
    const int32_t *status;        // [n_sel] 0, or TM_PDF_RANGE: every count 0
    const double *lo, *hi, *s;    // [n_sel] each
    uint32_t *out;                // [n_sel][n_bins + 2]: the classes, below, above
    long long n, max_samples;     // 1 <= n <= max_samples
    int32_t n_sel, n_bins;        // 1 <= n_bins <= TM_PDF_MAX_BINS
};
struct TmPdfPairArgs {
    const double *table;
    const int32_t *pairs;         // [n_pairs][2]
    const int32_t *status;        // [n_pairs]
    const double *lo, *hi, *s;    // [n_pairs][2] each
    uint32_t *out;                // [n_pairs][n_bins * n_bins + 1]: the cells, outside
    long long n, max_samples;
    int32_t n_pairs, n_bins;      // 1 <= n_bins <= TM_PDF_MAX_BINS2D
};
struct TmPdfHpdArgs {
    const uint64_t *keys;         // [w][P] sorted keys of the chunk's columns, the first n of each
    const long long *k;           // [n_mass] window lengths, 1 <= k <= n
    long long *start;             // [n_mass][w]
    double *lo, *hi;              // [n_mass][w] each
    long long n, P;
    int32_t w, n_mass;
};

int tm_launch_modepdf_hist(const TmPdfHistArgs &a, void *stream);            // each returns a hipError_t
int tm_launch_modepdf_pair(const TmPdfPairArgs &a, void *stream);
int tm_launch_modepdf_hpd(const TmPdfHpdArgs &a, void *stream);
