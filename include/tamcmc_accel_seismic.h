/* tamcmc_accel_seismic.h -- part of the C ABI of tamcmc_accel.h, which includes it: the seismic indices of the posterior
 * mode table.
 *
 * ---- Mode table, seismic indices: Dnu, epsilon, nu_max, separations, second differences, d02 ... r10 per sample -------------
 * What stellar modelling consumes of a peak-bagging table, computed per stored sample on the device and appended to the
 * mode table as further columns.  Every call that works on the table's columns -- tamcmc_modetable_result, _quantiles,
 * tamcmc_modediag_ess / _cov / _corr, tamcmc_moderank_diag -- then serves the indices as it serves the base columns: the
 * posterior of a ratio is read off its own column (the ratios are nonlinear and the chains are not Gaussian: propagating
 * means and covariances of the frequencies is the wrong calculation), and the covariance matrix of the ratios, whose
 * neighbours share frequencies, is tamcmc_modediag_cov of the ratio columns.
 *   An index column is value = num / den - offset, num and den ordered lists of terms over the base columns x[] of the same
 *   row: a term is coef * x[src], or with a weight column wsrc >= 0 (coef * x[src]) * (x[wsrc] * x[wsrc]); src = -1 reads the
 *   constant 1.0.  acc = 0.0, then per term in order t = coef * x[src], t = t * (w * w) if weighted, acc = acc + t; one
 *   division when den has terms, one subtraction when offset is not 0.  Only + - * /, never contracted: the column equals
 *   the same expression in IEEE double on the host, bit for bit.
 *   The plan is fixed by tamcmc_modetable_indices_enable from a reference params row, derived as any sample is:
 *     radial modes  the l = 0 freq columns sorted by reference frequency; ladder index k = 0, 1, ... is the position.  The
 *                   unweighted straight line through (k, nu_ref) has slope b_ref and intercept a_ref; n_base =
 *                   floor(a_ref / b_ref - 0.5) and the absolute radial order is n = n_base + k, so epsilon of the reference
 *                   row is in [0.5, 1.5).  Refused: fewer than 3 radial modes; a radial mode further than 0.25 b_ref from
 *                   the line (a missing order); a slope that is not positive and finite; |n_base| >= 1e9.
 *     l >= 1        u = (nu_ref - a_ref) / b_ref - l / 2, k = rint(u); the mode has order k iff |u - k| <= 0.35 and no other
 *                   mode of its degree has the same rint(u).  The others (mixed modes, modes off the asymptotic pattern) are
 *                   counted in n_unassigned and enter no column; a column that would need one, or a mode the model does not
 *                   have, is not created.
 *     least squares for the assigned orders k_1 < ... < k_T of a degree, sums in that order in double: kbar = (sum k_i) / T,
 *                   S = sum (k_i - kbar)^2, c_i = (k_i - kbar) / S, a_i = 1 / T - kbar c_i.
 *   Columns, in this order, nu_{n,l} the freq column of the mode (n, l), terms in the order written:
 *     DNU_FIT   per degree l with T >= 2 assigned modes:  sum c_i nu_{k_i,l}
 *     EPSILON   (sum a_i nu_{k_i,0}) / (sum c_i nu_{k_i,0}) - n_base
 *     NUMAX     (sum nu_k A_k^2) / (sum A_k^2) over the radial modes, A the amplitude column
 *     DNU_NL    per (l, n), l ascending, then n:  nu_{n,l} - nu_{n-1,l}
 *     D2NU      per (l, n):  nu_{n+1,l} - 2 nu_{n,l} + nu_{n-1,l}
 *     D02       nu_{n,0} - nu_{n-1,2}            D13   nu_{n,1} - nu_{n-1,3}
 *     D01       0.125 nu_{n-1,0} - 0.5 nu_{n-1,1} + 0.75 nu_{n,0} - 0.5 nu_{n,1} + 0.125 nu_{n+1,0}
 *     D10       -0.125 nu_{n-1,1} + 0.5 nu_{n,0} - 0.75 nu_{n,1} + 0.5 nu_{n+1,0} - 0.125 nu_{n+1,1}
 *     R02, R01  the numerators of D02, D01 over nu_{n,1} - nu_{n-1,1}
 *     R13, R10  the numerators of D13, D10 over nu_{n+1,0} - nu_{n,0}
 *   tamcmc_modetable_col of an index column: mult = -1; order = the absolute n (-1: DNU_FIT, EPSILON, NUMAX); l = the degree
 *     (DNU_FIT, DNU_NL, D2NU), the first degree of the pair (D02, R02, D01, R01: 0; D13, R13, D10, R10: 1), -1 for EPSILON
 *     and NUMAX; m = 0; param_index = -1.
 *   Status: a sample whose status is OK and that has a NaN index column (0 / 0) gets TAMCMC_CHAIN_NAN and is rejected like
 *     any sample with a NaN column; +-inf from a zero denominator is a value.
 *   indices_enable  allowed once per object, while the table holds no sample and no diagnostics buffer exists (right after
 *                create or reset).  The block's rows, the state and the table are allocated again for n_base_cols +
 *                n_index_cols columns (the sizes stated at tamcmc_modetable_create, and B of the larger n_cols);
 *                TAMCMC_E_NOMEM leaves the object as it was.  Refused with TAMCMC_E_INVALID: NULL arguments, an Nparams
 *                mismatch, a reference row whose status is not OK, the plan's refusals above, a second call, a table that
 *                has taken a sample, a tamcmc_modediag_* or tamcmc_moderank_* call before it, a context with a batch in
 *                flight or armed.  tamcmc_modetable_reset keeps the plan.  Afterwards _columns, _column, _derive, _push,
 *                _result, _quantiles and every tamcmc_modediag_* / tamcmc_moderank_* call see all the columns.  An object it
 *                is never called on behaves as before, byte for byte.
 *   indices_info the same numbers again: dnu_ref = b_ref, eps_ref = a_ref / b_ref - n_base.  Refused before enable.
 *   index_terms  the terms of index column col, num first, then den: n_num and n_den are always written for an index column;
 *                src, wsrc, coef (cap entries each) and offset when cap >= n_num + n_den.  TAMCMC_E_INVALID: a base column,
 *                a cap that is too small, NULL arrays.
 *   tamcmc_seismic_kernel_time   summed milliseconds and launch count of the indices kernel of the pushes since create or
 *                reset; tamcmc_modetable_kernel_time keeps meaning derive and fold. */
#ifndef TAMCMC_ACCEL_SEISMIC_H
#define TAMCMC_ACCEL_SEISMIC_H
#include "tamcmc_accel.h"
#ifdef __cplusplus
extern "C" {
#endif
#define TAMCMC_MODETABLE_DNU_FIT    13
#define TAMCMC_MODETABLE_EPSILON    14
#define TAMCMC_MODETABLE_NUMAX      15
#define TAMCMC_MODETABLE_DNU_NL     16
#define TAMCMC_MODETABLE_D2NU       17
#define TAMCMC_MODETABLE_D02        18
#define TAMCMC_MODETABLE_D13        19
#define TAMCMC_MODETABLE_D01        20
#define TAMCMC_MODETABLE_D10        21
#define TAMCMC_MODETABLE_R02        22
#define TAMCMC_MODETABLE_R01        23
#define TAMCMC_MODETABLE_R13        24
#define TAMCMC_MODETABLE_R10        25
typedef struct {
    int64_t n_base_cols, n_index_cols, n_radial, n_unassigned, n_base;
    double  dnu_ref, eps_ref;
} tamcmc_seismic_info;
int tamcmc_modetable_indices_enable(tamcmc_modetable *mt, int32_t Nparams, const double *ref_params, tamcmc_seismic_info *info);
int tamcmc_modetable_indices_info(tamcmc_modetable *mt, tamcmc_seismic_info *info);
int tamcmc_modetable_index_terms(tamcmc_modetable *mt, int32_t col, int32_t cap, int32_t *n_num, int32_t *n_den,
                                 int32_t *src, int32_t *wsrc, double *coef, double *offset);
int tamcmc_seismic_kernel_time(tamcmc_modetable *mt, double *total_ms, int64_t *launches);
#ifdef __cplusplus
}
#endif
#endif /* TAMCMC_ACCEL_SEISMIC_H */
