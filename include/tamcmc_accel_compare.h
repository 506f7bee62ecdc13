/* tamcmc_accel_compare.h -- part of the C ABI of tamcmc_accel.h, which includes it: the comparison of K fits of one spectrum
 * from their pointwise log predictive values.
 *
 * ---- Comparing fits: elpd differences, Bayesian bootstrap, pseudo-BMA(+) and stacking weights ------------------------------
 * tamcmc_summary_loo_* gives elpd_loo and a Pareto k-hat per bin, tamcmc_summary_wloo_* per window.  This object takes those
 * pointwise values of K fits of ONE spectrum on ONE set of units (bins or windows) and answers which fit predicts better, by
 * how much, and with what weight each fit enters an average.  It is bound to a device and to no context or chain, as
 * tamcmc_scan_null is.
 *   Input      K fits, 2 <= K <= TAMCMC_COMPARE_MAX_FITS, N units, 1 <= N < 2^31.  elpd[k * N + i] in float64: elpd_loo,
 *              elpd_lwo, or lppd - var_l.  pareto_k[k * N + i] or NULL.  scale s, finite and > 0: the log predictive density of
 *              unit i under fit k is s * elpd[k][i]; 1 for chi(2,2p), 0.5 for chi_square, whose l is kept without the factor
 *              1/2.  A unit is INCLUDED iff elpd[k][i] is finite for every k; N' = n_included.  The other units are counted
 *              in n_excluded and enter nothing.  Fit 0 is the reference fit of the bootstrap.  The inputs are copied.
 *   diff       pair (a, b), on the host in unit order in long double, as the LOO totals are: d_i = elpd[a][i] - elpd[b][i],
 *              one float64 subtraction; elpd_diff = sum d_i; se_diff = sqrt(N' / (N' - 1) * sum (d_i - elpd_diff / N')^2), NaN
 *              for N' < 2; n_better = #{d_i > 0}, n_worse = #{d_i < 0}.  With pareto_k: n_k_high counts the units where the
 *              k-hat of a or of b exceeds 0.7 (a NaN k-hat is skipped, +inf counts, as in tamcmc_summary_loo_result) and
 *              diff_k_high = sum d_i over those units: how much of the difference rests on units LOO cannot vouch for.
 *              Without pareto_k: n_k_high = -1, diff_k_high = NaN.  With N' = 0: elpd_diff, se_diff, diff_k_high are NaN.
 *   bootstrap  Rubin's Bayesian bootstrap, n_replicates more replicates on the device.  The variate of (unit i, global
 *              replicate g) is e = -log(u), u the (g & 1)-th uniform of Philox call (seed, replicate word g >> 1, bin word i,
 *              t = 0) of the scan null's generator (two replicates share one call): a function of (seed, the unit's ORIGINAL
 *              index, g) alone.  Per replicate over the included units A = sum e_i, B_k = sum e_i * D_k,i, k = 1 ... K - 1,
 *              D_k,i = elpd[k][i] - elpd[0][i] formed once in float64; z_k = ((double)N' * B_k) / A, z_0 = 0.  The sums run in
 *              one fixed order: a thread's units ascending, the lanes of a wave by a butterfly, the four waves in order, the
 *              tiles of TAMCMC_COMPARE_TILE units in tile order.  Only z[R][K - 1] is kept.  Replicate r of the object is
 *              global replicate first_replicate + r; no bit of it depends on how the replicates are split over calls or on
 *              scratch_bytes (the device memory of a chunk's partial sums; 0: 64 MiB; at least one replicate a chunk).
 *   z          the R values z_rk of fit k (zeros for k = 0).
 *   prob       over the R replicates the integer counts n_greater = #{r : z_ra > z_rb} and n_equal = #{r : z_ra = z_rb}.
 *   interval   the order statistic of z_ra - z_rb (one float64 subtraction) at rank ceil(q R) - 1 clamped to [0, R - 1]: the
 *              rank rule of the quantiles.  q in [0, 1].
 *   weights    method TAMCMC_COMPARE_PSEUDO_BMA: the softmax over k of s * elpd_diff(k, 0) (the maximum subtracted, the sum
 *              in ascending k); TAMCMC_COMPARE_PSEUDO_BMA_PLUS: the mean over r, in r order, of the softmax over k of s * z_rk
 *              (R >= 1); TAMCMC_COMPARE_STACKING: what the last tamcmc_compare_stacking returned.
 *   stacking   maximises f(w) = (1 / N') sum_i log sum_k w_k P_ki on the simplex, P_ki = exp(s (elpd[k][i] - max_k' elpd[k'][i])),
 *              by the EM fixed point from w = 1 / K.  An iteration evaluates g_k = (1 / N') sum_i P_ki / sum_j w_j P_ji, f(w) and
 *              gap = max_k g_k - 1, which bounds f(w*) - f(w) for this concave problem.  If gap <= tol the iteration stops,
 *              converged = 1; if it was iteration max_iter it stops, converged = 0; otherwise w_k <- w_k g_k.  So w, gap and
 *              f returned belong together, and iterations counts evaluations.  Reaching max_iter is no error.  The sums run
 *              in one fixed order (a thread's units ascending, lanes, waves, tiles of TAMCMC_COMPARE_STACK_TILE units in
 *              tile order); the device freezes w at the first iteration whose gap passes, so no bit depends on how often
 *              the host looks (tamcmc_compare_stacking_cadence, a test hook: iterations per look, 1 ... 4096, default 16),
 *              nor on scratch_bytes: P is kept in a table if K N doubles fit scratch_bytes (0: 1 GiB), and formed again by
 *              the same function in every iteration if not.  tol finite and >= 0, max_iter 1 ... 2^24.
 *   variates   the N variates of replicate r >= 0 of the object (excluded units too), by the kernel's own function: for tests.
 *   profile / kernel_time   as tamcmc_scan_null_profile / _kernel_time; which = 0 the bootstrap's chunks, 1 the stacking's
 *              launches (prepare, and every group of iterations between two looks).
 * Refused with TAMCMC_E_INVALID before any device is touched: a NULL handle or output, K or N out of range, NULL elpd, a scale
 * that is not finite and > 0, first_replicate < 0, a, b or k outside 0 ... K - 1, more than TAMCMC_COMPARE_MAX_REPLICATES
 * replicates in total, a negative scratch_bytes, q outside [0, 1], an unknown method, weights that are not there yet, and with
 * N' = 0 bootstrap and stacking.  All calls are synchronous, on the object's own stream. */
#ifndef TAMCMC_ACCEL_COMPARE_H
#define TAMCMC_ACCEL_COMPARE_H
#include "tamcmc_accel.h"
#ifdef __cplusplus
extern "C" {
#endif
#define TAMCMC_COMPARE_MAX_FITS 8
#define TAMCMC_COMPARE_MAX_REPLICATES 16777216
#define TAMCMC_COMPARE_TILE 2048
#define TAMCMC_COMPARE_STACK_TILE 4096
#define TAMCMC_COMPARE_PSEUDO_BMA 0
#define TAMCMC_COMPARE_PSEUDO_BMA_PLUS 1
#define TAMCMC_COMPARE_STACKING 2
typedef struct tamcmc_compare tamcmc_compare;
typedef struct tamcmc_compare_totals {
    int64_t n_included, n_excluded, n_better, n_worse, n_k_high;
    double elpd_diff, se_diff, diff_k_high;
} tamcmc_compare_totals;
typedef struct tamcmc_compare_stacking_info {
    int64_t iterations;
    int32_t converged, table;   /* table: 1 if P was kept in a table, 0 if formed again in every iteration */
    double gap, f;
} tamcmc_compare_stacking_info;
int tamcmc_compare_create(tamcmc_compare **out, int device_id, int32_t K, int64_t N, const double *elpd, const double *pareto_k,
                          double scale, uint64_t seed, int64_t first_replicate);
int tamcmc_compare_info(const tamcmc_compare *h, int64_t *n_included, int64_t *n_excluded);
int tamcmc_compare_diff(const tamcmc_compare *h, int32_t a, int32_t b, tamcmc_compare_totals *totals);
int tamcmc_compare_bootstrap(tamcmc_compare *h, int64_t n_replicates, int64_t scratch_bytes);
int tamcmc_compare_replicates(const tamcmc_compare *h, int64_t *R);
int tamcmc_compare_z(const tamcmc_compare *h, int32_t k, double *out);
int tamcmc_compare_prob(const tamcmc_compare *h, int32_t a, int32_t b, int64_t *n_greater, int64_t *n_equal);
int tamcmc_compare_interval(const tamcmc_compare *h, int32_t a, int32_t b, double q, double *value);
int tamcmc_compare_weights(const tamcmc_compare *h, int32_t method, double *w);
int tamcmc_compare_stacking(tamcmc_compare *h, double tol, int64_t max_iter, int64_t scratch_bytes, double *w,
                            tamcmc_compare_stacking_info *info);
int tamcmc_compare_stacking_cadence(tamcmc_compare *h, int32_t iterations_per_look);
int tamcmc_compare_variates(tamcmc_compare *h, int64_t r, double *e);
int tamcmc_compare_profile(tamcmc_compare *h, int enable);
int tamcmc_compare_kernel_time(tamcmc_compare *h, int32_t which, double *total_ms, int64_t *launches);
int tamcmc_compare_destroy(tamcmc_compare *h);
#ifdef __cplusplus
}
#endif
#endif /* TAMCMC_ACCEL_COMPARE_H */
