/* tamcmc_accel_pdf.h -- part of the C ABI of tamcmc_accel.h, which includes it: marginal histograms, shortest intervals
 * and pair densities of the posterior mode table's columns.
 *
 * ---- Mode table, marginal posteriors: histograms, HPD intervals, pair densities ----------------------------------------------
 * What a plot or a paper shows of a column beyond count, mean, sd and equal-tailed quantiles: the marginal itself in uniform
 * classes (the counterpart of the reference's Diagnostics::fwrite_histogram, for the derived columns), the shortest interval
 * holding a given mass -- the interval quoted for one-sided and skewed marginals such as an inclination piled up against
 * 90 degrees, the splitting of a low-S/N mode against 0, or a height -- and the joint density of two columns with its
 * contour levels.  Everything is computed on the device from the accepted rows of a table created with max_samples > 0;
 * n = n_used.  Every output is an integer count or an order statistic of a column: it equals the same statement in IEEE
 * double on the host bit for bit, whatever the pushes, max_samples, the selection, its order, or the scratch.
 *   Class rule (one function shared by host and device, never contracted), for a range lo, hi and n_bins classes:
 *     s = (double)n_bins / (hi - lo), formed once per column on the host;
 *     v < lo counts in `below`, v > hi in `above`; otherwise, if !(hi > lo), the class is 0; otherwise u = (v - lo) * s, one
 *     subtraction then one multiplication, and the class is (int64)u clamped to n_bins - 1 (v == hi, a product that rounds
 *     up).  (Where hi - lo is so small that s overflows, u is +inf, the last class, or at v == lo the invalid 0 * inf: class 0.)
 *   Range: lo / hi NULL means the column's min and max, exactly the doubles tamcmc_modetable_result returns; such a range
 *     that is not finite, or whose difference overflows (the seismic indices may hold +-inf), gives the column status
 *     TAMCMC_MODEPDF_RANGE and every count 0.  An explicit range must be finite with hi >= lo and a finite hi - lo,
 *     otherwise the call is refused.
 *   Plot edges: lo + (hi - lo) * ((double)b / n_bins), b = 0 ... n_bins, edge n_bins = hi exactly.  They are a helper for
 *     plots (ModeTable.hist_edges in Python), NOT part of the count rule: a value within an ulp of an edge is counted by the
 *     class rule above, whichever side the edge rounds to.
 *   hist     counts[j * n_bins + b], below[j], above[j] of selected column j; range[2 j], range[2 j + 1] the lo and hi used
 *            (NULL allowed); status[j] 0 or TAMCMC_MODEPDF_RANGE (NULL allowed).  n_bins 1 ... TAMCMC_MODEPDF_MAX_BINS; n_sel
 *            1 ... n_cols, cols NULL: the first n_sel columns; lo and hi both NULL or n_sel doubles each; n >= 1.
 *            counts + below + above sum to n for a column of status 0.
 *   hpd      the shortest interval holding mass_m of the column.  k_m = (int64)ceil(mass_m * (double)n) clamped to [1, n],
 *            formed on the host, returned in k[m] (NULL allowed).  Over the column sorted ascending in the order of the
 *            quantiles' keys (-0 and +0 are one value and come back as +0): w_i = s[i + k - 1] - s[i], i = 0 ... n - k, one
 *            subtraction; the interval is the i of the smallest w_i, the smallest i winning a tie, a NaN width (inf - inf)
 *            ranking above every other width, +inf included.  start, lo, hi are [n_mass][n_sel]: i, s[i], s[i + k - 1].
 *            n >= 4 (the sort kernel's condition); n_mass 1 ... TAMCMC_MODEPDF_MAX_MASS, each mass in (0, 1].  The columns are
 *            sorted in chunks that fit scratch_bytes of device memory of this feature's own (0: 256 MiB; at least one column
 *            a chunk: 8 P + 4 + 24 n_mass bytes a column, P the smallest power of two >= n, and 64 bytes); no bit depends on
 *            it.  TAMCMC_E_NOMEM leaves the object as it was.  At mass 1 the interval is the column's min and max.
 *            The interval is the highest-density region only of a unimodal marginal: regions of several intervals are not made.
 *   hist2d   counts[(p * n_bins + a) * n_bins + b] of pair p, a the class of column pairs[2 p], b of pairs[2 p + 1], by the
 *            class rule per axis; outside[p] the samples with either coordinate below or above its range; status[p]
 *            (NULL allowed) 1 if either axis is.  The two columns may be equal, a pair may repeat.  lo and hi both NULL or
 *            2 n_pairs doubles each, in the order of pairs.  n_bins 1 ... TAMCMC_MODEPDF_MAX_BINS2D per axis, n_pairs
 *            1 ... TAMCMC_MODEPDF_MAX_PAIRS, n >= 1.  level[m * n_pairs + p] is the largest count t such that the cells with
 *            count >= t together hold at least ceil(mass_m * n_in) samples, n_in the samples inside the range; 0 where
 *            n_in = 0: the contour level of mass m, computed on the host from the counts.  n_mass 0 ... 8; 0 with NULL mass
 *            and level.
 *   kernel_time  summed milliseconds and launch count of this feature's kernels since create or reset, the sort launches of
 *            hpd included; tamcmc_modetable_reset zeroes it.
 * Nothing of the table's state and nothing of tamcmc_modediag_*'s or tamcmc_moderank_*'s buffers is written: their results,
 * tamcmc_moderank_acov included, stay valid.  tamcmc_modetable_destroy frees the scratch.  All calls are synchronous, on the
 * context's stream.  Refused with TAMCMC_E_INVALID, before a device is touched: a NULL handle, a context with a batch in
 * flight or armed, max_samples = 0, too few rows, n_bins, n_sel, n_pairs or n_mass outside their ranges, a column index out
 * of range or (hist, hpd) repeated, a mass outside (0, 1] or NaN, an explicit range as above, only one of lo and hi, a
 * negative scratch_bytes, NULL counts, below, above, outside, start, lo or hi outputs. */
#ifndef TAMCMC_ACCEL_PDF_H
#define TAMCMC_ACCEL_PDF_H
#include "tamcmc_accel.h"
#ifdef __cplusplus
extern "C" {
#endif
#define TAMCMC_MODEPDF_MAX_BINS   4096
#define TAMCMC_MODEPDF_MAX_BINS2D 128
#define TAMCMC_MODEPDF_MAX_PAIRS  1024
#define TAMCMC_MODEPDF_MAX_MASS   8
#define TAMCMC_MODEPDF_RANGE      1
int tamcmc_modepdf_hist(tamcmc_modetable *mt, int32_t n_bins, int32_t n_sel, const int32_t *cols, const double *lo, const double *hi,
                        int64_t *counts, int64_t *below, int64_t *above, double *range, int32_t *status);
int tamcmc_modepdf_hpd(tamcmc_modetable *mt, int32_t n_mass, const double *mass, int32_t n_sel, const int32_t *cols, int64_t scratch_bytes,
                       int64_t *k, int64_t *start, double *lo, double *hi);
int tamcmc_modepdf_hist2d(tamcmc_modetable *mt, int32_t n_bins, int32_t n_pairs, const int32_t *pairs, const double *lo, const double *hi,
                          int32_t n_mass, const double *mass, int64_t *counts, int64_t *outside, int64_t *level, int32_t *status);
int tamcmc_modepdf_kernel_time(tamcmc_modetable *mt, double *total_ms, int64_t *launches);
#ifdef __cplusplus
}
#endif
#endif /* TAMCMC_ACCEL_PDF_H */
