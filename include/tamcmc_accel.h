/*
 * tamcmc_accel.h -- C ABI of the MI355X (gfx950) accelerator for TAMCMC's hot path:
 * for every parallel-tempered chain at once, params row -> model spectrum M(x) -> tempered
 * log-likelihood (-> gradient with respect to the relaxed variables).
 *
 * This is the drop-in boundary.  It replaces, for the whole batch of chains in one call, what the
 * reference does per chain inside its OpenMP loop (MALA.cpp:632-639):
 *
 *     Model_def::generate_model(Data*, long m, VectorXd Tcoefs)        model_def.cpp:358-367
 *       -> Model_def::call_model(Data*, int m)                          model_def.cpp:210-289
 *            -> model_MS_Global_* / model_MS_local_* / model_*_Gaussian models.cpp
 *       -> Model_def::call_likelihood(Data*, int m, VectorXd Tcoefs)    model_def.cpp:291-320
 *            -> likelihood_chi22p / likelihood_chi_square               likelihoods.cpp:17-39
 *
 * Conventions kept from the reference: all arithmetic fp64; logL is returned ALREADY DIVIDED by the
 * chain temperature Tcoefs[m] (model_def.cpp:302); the parameter layout is the flat `params` row
 * described by plength[0..10] (models.cpp:492-506); model / likelihood ids are the
 * integers of Config/default/models_ctrl.list and likelihoods_ctrl.list.  Where the reference would
 * print and exit() from inside the path the library reports a per-chain status instead.
 *
 * All entry points return TAMCMC_OK (0) or a TAMCMC_E_* code; none of them throws, prints or exits.
 * There is NO CPU fallback: without a usable HIP device tamcmc_ctx_create fails with
 * TAMCMC_E_NODEVICE.
 *
 * Environment switches read by tamcmc_ctx_create (developer knobs; none is needed in normal use, none changes a result
 * beyond rounding, and the tests exercise every one of them):
 *   TAMCMC_TILES, TAMCMC_TILES_GRAD   tiles per chain of the likelihood-only / gradient launch (default 8 units of 512 bins)
 *   TAMCMC_EQUAL_COST=1               per-chain tile boundaries of equal cost instead of equal length
 *   TAMCMC_COST, TAMCMC_COST_GRAD     "c0,a,b": the balancer's cost model
 *   TAMCMC_PRIO=1                     issue priority by launch rank
 *   TAMCMC_ORDER=0|1|2                launch order (default 2: tile-major, each chain's tiles costliest-first)
 *   TAMCMC_FUSED=0                    one-tile grids: prologue and evaluation as two launches instead of one
 *   TAMCMC_BG_EXACT=1                 Harvey background by exp() per bin instead of the per-cell polynomial
 *   TAMCMC_TAIL="frac,su2" | 0        gradient launch on long grids: 8-unit tiles for frac % of the units, su2-unit tiles for the
 *                                     rest (default "85,4"; 0: all tiles alike)
 *   TAMCMC_GATE_PATIENCE=n            polls (~2 us each) before the gate of an armed batch gives up (default 2^21: ~4 s; tests)
 * (tamcmc_sampler.h: TAMCMC_SAMPLER_THREADS, TAMCMC_SAMPLER_TIMING, TAMCMC_SAMPLER_ARM, TAMCMC_SAMPLER_ARRIVE.)
 *
 * Threading: one ctx = one device + one stream; calls on one ctx must be serialised by the caller;
 * different ctx objects (other GPUs, other stars) may be driven concurrently from different threads.
 * Ownership: the library copies x, y, sigma_y to the device at create time and never keeps caller
 * pointers after a call returns.
 */
#ifndef TAMCMC_ACCEL_H
#define TAMCMC_ACCEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tamcmc_ctx tamcmc_ctx;

/* error codes */
#define TAMCMC_OK                  0
#define TAMCMC_E_INVALID           1  /* bad argument (NULL pointer, negative size, plength/Nparams mismatch) */
#define TAMCMC_E_NODEVICE          2  /* no usable HIP device / device_id out of range                        */
#define TAMCMC_E_HIP               3  /* a HIP runtime call failed (see tamcmc_last_hip_error)                */
#define TAMCMC_E_MODEL_DISABLED    4  /* model id 4 or 5: the reference itself exits for these                */
#define TAMCMC_E_UNKNOWN_MODEL     5  /* id not in models_ctrl.list / likelihoods_ctrl.list                   */
#define TAMCMC_E_NOMEM             6
#define TAMCMC_E_NOVARS            7  /* gradient requested before tamcmc_ctx_set_vars                        */
#define TAMCMC_E_NOGRAD            8  /* gradient not available for this model/likelihood id, or (tamcmc_ctx_set_vars)
                                         for this many multiplets and variables: the backward kernel's tables would
                                         not fit its LDS; the context keeps its earlier variables              */
#define TAMCMC_PENDING            -1  /* tamcmc_eval_batch_poll only: not an error, the chain's result has not arrived yet */

/* per-chain status written by the eval calls */
#define TAMCMC_CHAIN_OK            0
#define TAMCMC_CHAIN_NAN           1  /* logL is NaN: legal, means "reject" (MALA.cpp:475,507-509).  Also where a
                                         width over- or underflows (AppWidth with an absurd exponent): the reference's
                                         formula stays finite there and loses the move by ~1e4 in logL -- same decision.
                                         The kernels overflow before the width itself does: a multiplet's components are
                                         summed over a common denominator, a product of 2 l + 1 factors of the order
                                         Gamma^2, so a Gamma beyond about 2e51 (l = 1), 1e31 (l = 2), 1e22 (l = 3) or
                                         1.34e154 (l = 0) gives this code where the reference's model is finite (id 10
                                         with a width reference frequency of 1e-6: Gamma = 3e37 ... 9e37)              */
#define TAMCMC_CHAIN_EMPTY_WINDOW  2  /* a truncation window is empty: the reference would exit(EXIT_FAILURE),
                                         build_lorentzian.cpp:428-443; logL is set to NaN                      */
#define TAMCMC_CHAIN_INTERNAL      3  /* internal consistency check of the tile balancer failed (never expected);
                                         logL is set to NaN                                                    */

/* Replaces: Config::setup() handing `Data` (data.h:24-36) + the integer switches
 * (config.cpp:95-98) to the Model_def constructor (model_def.cpp:27-55).
 *   device_id        HIP device ordinal (>= 0).
 *   model_case       models_ctrl.list id (0..14; 4 and 5 -> TAMCMC_E_MODEL_DISABLED).
 *   likelihood_case  0 = chi(2,2p), 1 = chi_square.
 *   likelihood_p     Model_def::likelihood_params; truncated to an integer like the reference's
 *                    `long p` argument (likelihoods.cpp:17).
 *   plength          the 11 block lengths of the params row.
 *   x, y, sigma_y    Nx doubles each on the host; sigma_y may be NULL unless likelihood_case == 1.
 *                    x must be the regular grid the reference assumes (build_lorentzian.cpp:423).
 *                    x[0] == 0 is supported (likelihood and gradient) with every active Harvey exponent |p| >= 1e-297;
 *                    a Harvey exponent of 0 on such a grid, and negative frequencies, are not.
 *   Nx               2 <= Nx <= 2^28 (TAMCMC_E_INVALID outside): the kernels address the grid with 32-bit byte
 *                    offsets; the reference itself reads at most 1e6 rows (config.cpp:531).  All launches are tested
 *                    against the oracle up to Nx = 4 194 779 (8193 units of 512 bins, 1025 / 1178 tiles per chain;
 *                    tests/test_long_grids_gpu.py); what changes between there and 2^28 -- the chain-major launch
 *                    above 65 535 tiles, the backward kernel's LDS growing with the tile count (tamcmc_ctx_set_vars) --
 *                    is tested on a short grid with tile counts given by hand, not at those lengths. */
int tamcmc_ctx_create(tamcmc_ctx **out, int device_id, int model_case, int likelihood_case,
                      double likelihood_p, const int32_t plength[11], int64_t Nx,
                      const double *x, const double *y, const double *sigma_y);

/* Replaces: Model_def::index_to_relax (model_def.cpp:81-88).  Declares which params columns are
 * the free variables; needed only for gradients.  grad column k = d(logL/T)/d params[index_to_relax[k]].
 * TAMCMC_E_NOGRAD (nothing changed) when the gradient tables of the layout with these variables exceed the backward
 * kernel's LDS (504 bytes per multiplet + 72 per variable + 12 per parameter + 4 per gradient tile > 150 KB: with every
 * entry a variable from some 210 (id 13) to 235 (id 2) multiplets on; 256 multiplets take up to 262 variables);
 * likelihood batches are not affected.  The tile term is what a long grid adds: the gradient launch has about
 * 0.144 tiles per unit of 512 bins (tamcmc_ctx_geometry_grad), i.e. 28 tiles per 1e5 bins.  For a typical layout
 * -- 21 multiplets, 56 parameters, 44 variables: 15 224 bytes + 4 per tile -- the largest accepted count is 34 593 tiles
 * (tested, through TAMCMC_TILES_GRAD on a short grid), which the default geometry exceeds from Nx = 123 211 777 on
 * (240 649 units; computed from the tile rule, not run): from there on such a star has a likelihood and no gradient.
 * TAMCMC_E_INVALID (nothing changed, the earlier variables stay) for an index outside 0 ... Nparams - 1, for an index that
 * occurs twice (hence for Nvars > Nparams: every variable is one column, in the order of the list, which need not be
 * ascending), and while a batch is in flight or armed.  Nvars = 0 takes the variables away: a gradient request then
 * returns TAMCMC_E_NOVARS. */
int tamcmc_ctx_set_vars(tamcmc_ctx *ctx, int32_t Nvars, const int32_t *index_to_relax);

/* Extension (no counterpart in the reference, which fits one spectrum per process): several spectra ON THE SAME GRID
 * and model layout in one context -- an ensemble of synthetic stars, noise realisations of one star -- so that their
 * chains share a batch (one launch at the full-batch rate; separate contexts on separate streams overlap only ~1.5x,
 * DESIGN.md section 6).  set_spectra replaces the resident spectrum by Nspectra blocks of Nx (sigma_y likewise, NULL
 * unless the likelihood is chi_square) and clears the map; set_chain_spectrum says which spectrum chain m of the
 * following batches is fitted to.  While more than one spectrum is resident every batch must be covered by the map:
 * an evaluation of more chains than the map holds (or without a map) returns TAMCMC_E_INVALID instead of fitting the
 * uncovered chains to spectrum 0.  A chain's result is bit for bit what a context holding only its spectrum returns. */
int tamcmc_ctx_set_spectra(tamcmc_ctx *ctx, int32_t Nspectra, const double *y, const double *sigma_y);
int tamcmc_ctx_set_chain_spectrum(tamcmc_ctx *ctx, int32_t Nchains, const int32_t *spectrum_of_chain);

/* Extension: fit GROUPS -- the likelihood batches of several contexts (different grids, model ids, likelihoods, parameter
 * layouts: the slices of a local fit, an ensemble of stars) evaluated together, one launch per kernel kind (at most a
 * setup launch, a fused one-tile launch and two eval launches -- the generic body of chi_square and ids 0 / 1 apart --
 * instead of one to two launches per context).
 *   create      members: n_members distinct contexts on one device, 1 <= n_members <= TAMCMC_GROUP_MAX_MEMBERS.  A
 *               context counts the groups it belongs to; while that count is non-zero tamcmc_ctx_destroy returns
 *               TAMCMC_E_INVALID and leaves it intact: destroy the group first.
 *   eval        host pointers, synchronous.  Nchains[k] >= 0 chains of member k (0: the member sits this call out; the
 *               sum must be >= 1), Nparams[k] must equal member k's.  params / Tcoefs / logL / status are the members'
 *               blocks concatenated in member order (member k: Nchains[k] rows of Nparams[k]); status may be NULL.
 *               One pinned staging area, one copy in, one copy out.
 *   eval_device the same with device pointers, enqueued on the group's stream without synchronising; d_status may be NULL.
 * Results: every chain's logL and status are bit for bit what its member returns alone through tamcmc_eval_batch --
 * multi-spectrum members included (their chain map applies, and must cover the member's batch as set_spectra requires).
 * Refused with TAMCMC_E_INVALID: NULL arguments, an Nparams mismatch, a negative count or an all-zero call, a member
 * that is armed or has a batch in flight, and a call whose 1-D launch would exceed 2^32 work-items.
 * Ordering: the group has a stream of its own (set_stream replaces it).  Work enqueued earlier on a member's stream runs
 * before a group call that includes the member, and work enqueued later on it runs after: solo calls and group calls
 * on the same contexts may alternate without any synchronisation by the caller.  Calls on one group, and on its
 * members, must be serialised by the caller as for a context.
 * Out of scope: gradients and model rows -- use a member alone for those. */
#define TAMCMC_GROUP_MAX_MEMBERS 1024
typedef struct tamcmc_group tamcmc_group;
int tamcmc_group_create(tamcmc_group **out, int32_t n_members, tamcmc_ctx *const *members);
int tamcmc_group_eval(tamcmc_group *g, const int32_t *Nchains, const int32_t *Nparams, const double *params,
                      const double *Tcoefs, double *logL, int32_t *status);
int tamcmc_group_eval_device(tamcmc_group *g, const int32_t *Nchains, const int32_t *Nparams, const double *d_params,
                             const double *d_Tcoefs, double *d_logL, int32_t *d_status);
int tamcmc_group_set_stream(tamcmc_group *g, void *hip_stream);
int tamcmc_group_synchronize(tamcmc_group *g);
int tamcmc_group_destroy(tamcmc_group *g);
/* tamcmc_group_eval in two halves, for callers that have host work to overlap with the GPU (a sampler per member, see
 * tamcmc_lockstep in tamcmc_sampler.h): _begin takes the same concatenated blocks and refuses what tamcmc_group_eval
 * refuses, copies params / Tcoefs into pinned, device-mapped, coherent memory owned by the group and enqueues the
 * launches, which read them and write logL / status there directly -- no copy-engine transfer; _end waits until every
 * result has arrived (a few microseconds before the launch retires, as for tamcmc_eval_batch_end) and delivers them
 * (status may be NULL); same bits as tamcmc_group_eval.  The inputs are double-buffered by call parity: filling the
 * buffers of one call never touches what a kernel of the previous call may still read.
 *   One batch in flight per group: while it is, a second _begin and every other entry point of the group return
 *   TAMCMC_E_INVALID, except _poll and _destroy (which waits for the batch and hands nothing out); _end without _begin
 *   returns TAMCMC_E_INVALID.  A failed launch ends _end with TAMCMC_E_HIP, and the members stay usable.
 *   _poll   chain `chain` of member `member` of the batch in flight: TAMCMC_OK with its logL and status once they have
 *           arrived, TAMCMC_PENDING before.  Read-only: any number of threads may poll while no other entry point of the
 *           group is called; _end is still due, and is the call that reports a failed launch.
 * Ordering is as stated above; on this path the group orders its stream after a member's own stream only when something
 * was enqueued there since it last did, and a member's stream is made to wait for the group's launches when it is next
 * used, not by the group call.
 * _members: the number of members, their Nparams[n_members] and the device (each pointer may be NULL). */
int tamcmc_group_eval_begin(tamcmc_group *g, const int32_t *Nchains, const int32_t *Nparams, const double *params,
                            const double *Tcoefs);
int tamcmc_group_eval_end(tamcmc_group *g, double *logL, int32_t *status);
int tamcmc_group_eval_poll(const tamcmc_group *g, int32_t member, int32_t chain, double *logL, int32_t *status);
int tamcmc_group_members(const tamcmc_group *g, int32_t *n_members, int32_t *Nparams, int32_t *device);

/* Extension: posterior SUMMARIES of a stored chain -- what a user does with the samples of an Acquire phase: the
 * posterior-mean model with its envelope, and WAIC to compare two fits of the same spectrum -- without handing S x Nx
 * model values through host memory.  (The reference's diagnostics.cpp needs gnuplot, Boost and the whole temperature
 * ladder; this is its data-parallel core: a per-bin reduction over samples of what the eval kernels already produce.)
 * A summary object is bound to one context, is fed parameter rows in any number of pushes and keeps per-bin running
 * statistics on the device.  Samples are evaluated at temperature 1.  For every sample s with status TAMCMC_CHAIN_OK and
 * every bin i: the model value M_is and the POINTWISE log-likelihood l_is,
 *     chi(2,2p)    l_is = -p (y_i / M_is + log M_is)        p = likelihood_p truncated as everywhere in this library
 *     chi_square   l_is = -(y_i - M_is)^2 / sigma_i^2       the REFERENCE'S convention (likelihoods.cpp:31-39): no factor
 *                                                            1/2, so lppd / p_waic / waic are on that scale too
 * Per bin, with n = samples accepted so far:
 *     mean_M, var_M   mean and variance (divisor n - 1) of M_is           min_M, max_M   the envelope
 *     mean_l, var_l   the same for l_is; var_l is the bin's WAIC penalty   lppd           log((1/n) sum_s exp l_is)
 * and the totals n_used, n_rejected, lppd_total = sum_i lppd_i, p_waic = sum_i var_l_i, waic = -2 (lppd_total - p_waic),
 * summed on the host in bin order in long double.  With n < 2 the two variances are NaN; with n = 0 everything is NaN.
 * A sample whose status is not OK is left out of every bin and counted in n_rejected.
 *   create       block_chains: samples evaluated per block (the object owns block_chains x Nx doubles for their model
 *                rows); 0 picks 64, lowered so that this buffer stays within 64 MiB.  A context counts its summary
 *                objects like its groups: while one exists tamcmc_ctx_destroy and tamcmc_ctx_set_spectra return
 *                TAMCMC_E_INVALID.
 *   push         host pointers, synchronous.  params: Nsamples x Nparams; logL / status (each may be NULL): per sample,
 *                the bits tamcmc_eval_batch returns for that row at T = 1 with that chain listed in model_rows.  More
 *                samples than one block are cut into blocks internally.
 *   push_device  the same with device pointers, enqueued on the context's stream without synchronising.
 *   result       synchronises the stream; may be called between pushes and does not disturb the running state.  Seven
 *                arrays of Nx doubles on the host, any of them (and totals) may be NULL.
 *   reset        forgets every sample.       destroy   TAMCMC_E_INVALID while a batch is armed on the context.
 * Every bin is folded one sample at a time in push order by one thread (Welford's recurrence for the two mean / variance
 * pairs, a running-maximum log-sum-exp for lppd; tamcmc_summary.hip), so every result is BIT FOR BIT independent of
 * block_chains and of how the samples are split over pushes.
 * Refused with TAMCMC_E_INVALID: NULL arguments, Nsamples < 1, an Nparams mismatch, block_chains < 0, a context with a
 * batch in flight or armed, and a context holding more than one spectrum (tamcmc_ctx_set_spectra; out of scope, as are
 * fit groups).
 *   profile / kernel_time   as tamcmc_ctx_profile / tamcmc_ctx_kernel_time, for the fold kernel alone (one event pair per
 *                block while enabled); in quantile mode, for the histogram kernel that takes its place.
 *
 * QUANTILES (credible bands): the exact per-bin order statistics of M_is over the accepted samples -- the median model
 * with its 16 / 84 % band, say -- by a radix selection that takes a few passes over the chain: the caller pushes the SAME
 * samples again once per pass, and every pass resolves bits_per_pass more bits of every requested quantile of every bin
 * (tamcmc_quantile.h).  Nothing is approximated: a resolved value is one of the pushed model values, bit for bit, and is
 * independent of block_chains and of how the samples are split over pushes (which may differ from pass to pass).
 *   Rank rule, the same for every bin: k = (int64_t)ceil(q n) - 1 clamped to [0, n - 1], n = n_used -- the smallest sample
 *   whose empirical CDF reaches q (numpy's method "inverted_cdf").  q = 0 is min_M, q = 1 is max_M, q = 0.5 with odd n is
 *   the middle sample.  Values are ordered as doubles with -0 = +0.  An accepted sample cannot hold a NaN model value: its
 *   logL would be NaN and its status TAMCMC_CHAIN_NAN.
 *   quantiles_begin   freezes the fold state (n_used, the envelope min_M / max_M), computes the ranks and allocates the
 *                selection's memory on the device: Nq x 2^bits x Nx x 4 bytes of histogram plus (16 Nq + 20) Nx bytes of
 *                state; TAMCMC_E_NOMEM when that fails, and the object stays as it was.  bits_per_pass: 1 ... 6, or 0 for
 *                the library's default (6).  Refused with TAMCMC_E_INVALID: n_used < 1 or >= 2^32, Nq outside
 *                1 ... TAMCMC_SUMMARY_MAX_QUANTILES, a q that is NaN or outside [0, 1], bits_per_pass outside 0 ... 6,
 *                quantile mode already on, a context with a batch in flight or armed.
 *   While the mode is on, push and push_device evaluate the rows as before and hand out the same logL and status bits, but
 *   feed the histogram kernel instead of the fold kernel; tamcmc_summary_result keeps returning the frozen fold results.
 *   quantiles_step    after the caller has pushed the same samples again.  If the pass saw n_used accepted samples, the
 *                fold pass's rejected count and no model value outside the envelope, every bracket is narrowed and
 *                *bits_left (may be NULL) gets the largest number of unresolved bits over all bins and quantiles; 0 =
 *                every result is exact.  Otherwise TAMCMC_E_INVALID: the pass is discarded, the state of the previous
 *                step stays and the pass can be repeated.  (A pass of other samples that happen to pass these three
 *                checks cannot be told apart and gives brackets without meaning.)  A bin's key range has u0 <= 64
 *                unresolved bits at first -- 48 or 49 for a typical posterior -- and exactness takes ceil(u0 / bits)
 *                steps.  A step with nothing left to resolve is a no-op that returns 0 bits left.
 *   quantiles_result  may be called after any step, and before the first (the bracket is the envelope then).  ranks[Nq],
 *                lo[Nq x Nx], hi[Nq x Nx] on the host, any of them may be NULL: the doubles of the lowest and highest key
 *                of the bracket that holds the order statistic, hi clipped to max_M.  Where a bin is resolved,
 *                lo == hi == the order statistic, bit for bit.
 *   quantiles_end     frees the selection's memory and goes back to fold mode: the running statistics are untouched and
 *                further pushes fold as before.  tamcmc_summary_reset also leaves the mode; tamcmc_summary_destroy works
 *                in either.  _step, _result and _end outside the mode return TAMCMC_E_INVALID.
 *
 * PSIS-LOO: leave-one-out cross-validation by Pareto-smoothed importance sampling (Vehtari, Gelman & Gabry 2017; Vehtari
 * et al. 2024) -- elpd_loo on the scale of lppd, and per bin the Pareto shape k-hat that says whether the bin's value can
 * be trusted (k-hat > 0.7: it cannot; WAIC is biased in the same bins and gives no sign of it).  A third mode beside fold
 * and quantile mode: after the fold pass the caller pushes the SAME samples once more.  For chi_square l keeps the
 * reference's convention without the factor 1/2, as lppd and WAIC do here, so elpd_loo / p_loo / looic are on that scale.
 *   Definition, per bin i, with x_s = -l_is over the n = n_used accepted samples:
 *     1. M = (int64)ceil(fmin(n / 5.0, 3.0 * sqrt((double)n))), xmax = max_s x_s, z_s = x_s - xmax.
 *     2. If n > M: c = max(the (M+1)-th largest z, log(DBL_MIN)); the tail T = {s : z_s > c} (strictly: ties with the
 *        cutoff are body), L = |T|.  If n <= M (only n = 1) there is no tail.
 *     3. If L >= 5: t_j = exp(z_(j)) - exp(c) ascending, j = 1 ... L, and the generalised Pareto fit of Zhang & Stephens:
 *        m = 30 + floor(sqrt(L)); theta_j = (1 - sqrt(m / (j - 0.5))) / (3 t_(q)) + 1 / t_(L), q = floor(L/4 + 0.5),
 *        j = 1 ... m; k_j = mean_i log1p(-theta_j t_i); l_j = L (log(-theta_j / k_j) - k_j - 1); w_j = 1 / sum_i exp(l_i -
 *        l_j), every w_j < 10 * 2^-52 dropped and the rest renormalised; theta = sum w_j theta_j; k = mean_i log1p(-theta
 *        t_i); sigma = -k / theta; k-hat = (L k + 5) / (L + 10).  If k-hat is finite the smoothed tail is zt_(j) =
 *        min(log(sigma / k-hat * expm1(-k-hat log1p(-p_j)) + exp(c)), 0), p_j = (j - 0.5) / L (for k-hat == 0 the inner
 *        term is -sigma log1p(-p_j)); otherwise zt = z.  If L <= 4: k-hat = +inf and zt = z (every n <= 20).
 *     4. elpd_loo_i = log(n_body + sum_T exp(zt_(j) - z_(j))) - xmax - log(sum_body exp(z_s) + sum_T exp(zt_(j))), the
 *        body sum accumulated as such.  With n = 0 everything is NaN.
 *     5. Totals, summed on the host in bin order in long double: elpd_loo; p_loo = lppd_total - elpd_loo; looic =
 *        -2 elpd_loo; k_max (may be +inf; a NaN k-hat is skipped); n_k_high = bins with k-hat > 0.7, +inf counted;
 *        n_k_inf = bins with k-hat = +inf.
 *   loo_begin    freezes the fold state as quantiles_begin does, computes M and allocates (M + 1) x Nx doubles for the
 *                per-bin sets of the M + 1 largest x plus 52 Nx bytes of state; TAMCMC_E_NOMEM when that fails, and the
 *                object stays as it was.  Refused with TAMCMC_E_INVALID: n_used < 1, M > TAMCMC_SUMMARY_LOO_MAX_TAIL
 *                (n_used > 466 033: thin the chain), quantile mode or LOO mode already on, a context with a batch in
 *                flight or armed.  tamcmc_summary_quantiles_begin is refused while LOO mode is on.
 *   While the mode is on, push and push_device evaluate the rows as before and hand out the same logL and status bits, but
 *   feed the tail kernel (tamcmc_loo.hip) instead of the fold kernel; tamcmc_summary_result keeps returning the frozen fold
 *   results.  Every result is bit for bit independent of block_chains and of how the pass is split over pushes.
 *   loo_result   totals, elpd_loo[Nx], pareto_k[Nx], cutoff[Nx], tail_len[Nx] on the host, any of them may be NULL.
 *                cutoff is the un-shifted (M+1)-th largest x, before the log(DBL_MIN) floor and before xmax is subtracted
 *                (NaN where there is no tail rule); tail_len is L.  If the pass did not see exactly the fold pass's
 *                accepted and rejected counts: TAMCMC_E_INVALID, the pass is discarded and may be repeated.  May be called
 *                again without another pass.
 *   loo_end      frees the mode's memory and goes back to fold mode: the running statistics are untouched and further
 *                pushes fold as before.  tamcmc_summary_reset also leaves the mode; tamcmc_summary_destroy works in any.
 *                _result and _end outside the mode return TAMCMC_E_INVALID.
 *   profile / kernel_time in LOO mode: the tail kernel of every block, and the finalize kernel of every loo_result.
 *
 * LOO-PIT: the leave-one-out probability integral transform (ArviZ's loo_pit).  The posterior predictive check below uses
 * each datum twice -- bin i's PIT is averaged over a posterior that was fitted to bin i -- so a narrow Lorentzian parked on
 * one noise spike looks calibrated there.  Here the same predictive tails are averaged with the Pareto-smoothed importance
 * weights of PSIS-LOO, and the same pass gives Kish's effective sample size of those weights, the diagnostic the `loo`
 * literature expects beside k-hat.  A sub-mode of LOO mode: after a complete LOO pass the caller pushes the SAME samples a
 * third time.  A stored MCMC chain repeats a row at every rejected proposal, so exact ties in the tail are the normal case.
 *   Definition, per bin i, with xmax, c, the tail T of length L, z_(j) ascending, k-hat and the smoothed zt_(j) of steps 1-3
 *   above, unchanged (zt = z where there is no usable fit).  For every accepted sample s, in push order:
 *     1. x = -l_is as the tail kernel forms it; z = x - xmax.
 *     2. The log weight lw_s.  Body (!(z > c), or no tail rule): lw = z.  Tail: let a..b be the run of sorted tail slots
 *        whose stored value equals x bit for bit; a run of length 1 gives lw = zt_(a), a longer one lw = log((sum_{j=a..b}
 *        exp(zt_(j))) / (b - a + 1)), summed in ascending j: every member of a tie gets the mean weight of the ranks the tie
 *        occupies, so the result does not depend on which of two equal samples came first.
 *     3. logP_is, logQ_is: the predictive tails of the posterior predictive check below, unchanged.
 *     4. Four running-maximum log-sum-exps by that check's recurrence (Kahan-compensated, terms of -inf skipped):
 *        lW = lse(lw), lA = lse(lw + logP), lB = lse(lw + logQ), lW2 = lse(2 lw).
 *     loo_log_cdf = lA - lW, loo_log_sf = lB - lW; loo_pit from the smaller tail on the host, as pit is; is_ess =
 *     exp(2 lW - lW2), Kish's effective sample size of the smoothed weights, in 1 ... n; log_wsum = lW.  A bin whose xmax is
 *     not finite gives NaN in all five.
 *   Totals, on the host in bin order in long double: n_used, n_rejected; ks_D and pit_hist of loo_pit as in the posterior
 *   predictive check; min_log_sf and min_log_cdf with their bins and min_is_ess with its bin, the first bin winning a tie
 *   (-1 and NaN where every bin is NaN).
 *   loo_pit_begin   allowed in LOO mode once the LOO pass has seen exactly the fold pass's counts.  Allocates M x Nx doubles
 *                for the table of log weights plus 116 Nx + 36 bytes of state (TAMCMC_E_NOMEM when that fails, and the
 *                object stays as it was), then runs the prepare kernel (tamcmc_loopit.hip): per bin the top set is
 *                sorted in place -- a sorted array is a valid heap, and loo_result keeps returning the same bits -- and the
 *                table is filled.  Refused with TAMCMC_E_INVALID: outside LOO mode; an incomplete LOO pass, which is left
 *                untouched (only loo_result discards it); a second call; a chi(2,2p) context with p < 1 or p >
 *                TAMCMC_SUMMARY_PREDICTIVE_MAX_P; a context with a batch armed or in flight.
 *   From then on push and push_device feed the PIT kernel; the top sets are frozen.  Every result is bit for bit independent
 *   of block_chains and of how the pass is split over pushes.
 *   loo_pit_result  totals and five arrays of Nx doubles on the host, any of them may be NULL.  If the third pass did not
 *                see exactly the fold pass's counts, or any tail sample was not found bit for bit among the stored values
 *                (the caller pushed other rows): TAMCMC_E_INVALID, the PIT pass is cleared and may be repeated.  May be
 *                called again without another pass.
 *   loo_end, tamcmc_summary_reset and tamcmc_summary_destroy free the sub-mode's memory with the mode's.
 *   loo_pit_kernel_time   as tamcmc_summary_predictive_kernel_time, for the PIT kernel alone; tamcmc_summary_kernel_time
 *                reports the prepare kernel with the tail and finalize kernels.
 *
 * WINDOW-LOO: leave-one-WINDOW-out PSIS-LOO, and LOO-PIT per window.  Leaving one bin of a 20-bin mode out tests almost
 * nothing -- the 19 neighbours pin the mode -- so per-bin elpd_loo and LOO-PIT are optimistic exactly where the question is
 * whether the model predicts the feature, and the windowed check below uses each datum twice.  Bins are conditionally
 * independent given the parameters, so leaving a window out is the same machinery fed with the window's sum of l: elpd and
 * k-hat at the granularity of a feature, the unit at which two fits of one spectrum should be compared.  A mode of its own
 * beside fold, quantile, LOO, ESS and band ESS mode, shaped like LOO mode and its LOO-PIT sub-mode; the windows are those of
 * the windowed check (W in 1 ... TAMCMC_SUMMARY_WINDOW_MAX_BINS, first in 1 ... W, 0 = W; window 0 is [0, min(first, Nx)),
 * window w >= 1 is [first + (w-1) W, min(first + w W, Nx))).  It does not need window_enable.
 *   Definition.
 *     Window sum: for window w and accepted sample s, S_ws = l_is (the fold kernel's l) added over the window's bins in
 *       ascending bin order, starting from the first term, in plain double without contraction.  x_ws = -S_ws.
 *     LOO per window: steps 1 - 5 of the PSIS-LOO definition above with "bin" read as "window" and x_ws for x_s: the same
 *       M(n), cutoff, tail, fit, smoothing and elpd; totals in window order in long double: elpd_lwo; p_lwo = (the sum of lppd
 *       over ALL bins, as tamcmc_summary_result forms it) - elpd_lwo; k_max, n_k_high, n_k_inf over the windows; n_windows,
 *       W, first.  W = 1 is LOO mode bit for bit.
 *     Sub-mode: steps 1 - 4 of the LOO-PIT definition above with x_ws for x, and for logP, logQ the windowed check's tails
 *       of that sample and window (the window sum of the residuals through the Gamma(p len) or Gaussian tails described
 *       under WINDOWED POSTERIOR PREDICTIVE CHECK, bit for bit what that check forms).  Per window: loo_pit, loo_log_cdf,
 *       loo_log_sf, is_ess, log_wsum; the totals are those of LOO-PIT with windows in place of bins (bin_min_* hold window
 *       indices).  W = 1 is LOO-PIT bit for bit where p is a power of two (as the windowed check is the per-bin check).
 *   wloo_begin   freezes the fold state as loo_begin does, resolves first and n_windows (*n_windows, may be NULL), computes
 *                M and allocates, with nw = n_windows and B = block_chains: 8 (M + 1) nw bytes for the per-window sets of the
 *                M + 1 largest x, 52 nw + 32 bytes of state and 8 B nw bytes for a block's window sums; TAMCMC_E_NOMEM when
 *                that fails, and the object stays as it was.  Refused with TAMCMC_E_INVALID: W or first out of range,
 *                n_used < 1, M > TAMCMC_SUMMARY_LOO_MAX_TAIL, any mode already on (quantile, LOO, ESS, band ESS, this one), a
 *                context with a batch in flight or armed.  While the mode is on every other mode's begin and the three
 *                _enable functions are refused.
 *   While the mode is on, push and push_device evaluate the rows as before and hand out the same logL and status bits, but
 *   feed the sums and tail kernels (tamcmc_wloo.hip); the fold, predictive, window and scan states are not touched.  Every
 *   result is bit for bit independent of block_chains and of how the pass is split over pushes.
 *   wloo_result  totals and, per window, elpd_lwo, pareto_k, cutoff (doubles), tail_len (int32), first_bin and last_bin
 *                (int64, inclusive) on the host, any of them may be NULL.  If the pass did not see exactly the fold pass's
 *                accepted and rejected counts: TAMCMC_E_INVALID, the pass is discarded and may be repeated.  May be called
 *                again without another pass.
 *   wloo_pit_begin  allowed in the mode once its pass has seen exactly the fold pass's counts.  Allocates 8 M nw bytes for
 *                the table of log weights, 116 nw + 36 bytes of state and 16 B nw bytes for a block's tails (TAMCMC_E_NOMEM
 *                when that fails, and the object stays as it was), then sorts the top sets in place and fills the table (the
 *                prepare kernel of LOO-PIT).  Refused with TAMCMC_E_INVALID: outside the mode; an incomplete pass, which is
 *                left untouched; a second call; a chi(2,2p) context with p < 1 or p W > TAMCMC_SUMMARY_WINDOW_MAX_SHAPE; a
 *                context with a batch armed or in flight.  From then on push and push_device feed the sub-mode's kernels.
 *   wloo_pit_result  totals and five arrays of n_windows doubles on the host, any of them may be NULL.  If the third pass
 *                did not see exactly the fold pass's counts, or a tail sample was not found bit for bit among the stored
 *                values: TAMCMC_E_INVALID, the PIT pass is cleared and may be repeated.  May be called again.
 *   wloo_end     frees the mode's memory, the sub-mode's included, and goes back to fold mode; tamcmc_summary_reset also
 *                leaves the mode, tamcmc_summary_destroy works in any.  _result, _pit_* and _end outside the mode return
 *                TAMCMC_E_INVALID.
 *   profile / kernel_time in the mode: the sums and tail kernels of every block of the LOO pass, the finalize kernel of
 *   every wloo_result and the prepare kernel; wloo_pit_kernel_time: the sums, tails and PIT kernels of every block of the
 *   third pass together.
 *
 * POSTERIOR PREDICTIVE CHECK: is the residual spectrum distributed as the likelihood claims, and in which bins is it not?
 * Per bin the predictive CDF of the datum averaged over the chain -- its probability integral transform (PIT) -- and both
 * tail probabilities as logarithms, which stay meaningful far below 1e-300: a missed mode has y / M of a few thousand.
 * (The classical residual is y / M at the best fit with the false-alarm probability exp(-y / M); this is its posterior
 * version.)  Not a mode and no pass of its own: a setting of the object under which every fold-mode block runs one more
 * kernel (tamcmc_predictive.hip) behind the fold kernel, on the same rows and the same stream.
 *   Definition, per bin i, over the n = n_used accepted samples s, M = M_is:
 *     chi(2,2p)    p = likelihood_p truncated as everywhere in this library, an integer in 1 ... 64.  Under the sample's
 *                  model the datum is Gamma-distributed with shape p and scale M / p: with z = p y_i / M_is,
 *                  P_is = P(p, z), the regularised lower incomplete gamma function, Q_is = Q(p, z) = exp(-z) sum_{k<p}
 *                  z^k / k!, the upper one.  z <= 0 (y_i <= 0): P = 0, Q = 1.
 *     chi_square   the library's l = -(y - M)^2 / sigma^2 is the logarithm of a Gaussian density with standard deviation
 *                  sigma / sqrt(2), not sigma; the check takes the likelihood at its word: with r = (y_i - M_is) / sigma_i,
 *                  P_is = erfc(-r) / 2 and Q_is = erfc(r) / 2.
 *     log_cdf_i = log((1/n) sum_s P_is)        log_sf_i = log((1/n) sum_s Q_is)
 *                  Both tails of a sample are computed as logarithms and directly, each by adding terms of one sign, never
 *                  as 1 - the other where that cancels, for any finite z >= 0 and any |r| < 1.3e154 (tamcmc_predictive.h
 *                  has the forms and their measured error: a few ulp of max(1, |value|) for p = 1 and chi_square, 2^-42
 *                  for p > 1).  Each sum is a running-maximum log-sum-exp in push order by the fold kernel's recurrence,
 *                  with four additions: a term of -inf adds nothing; a sum without a finite term is -inf; (-inf) -
 *                  (-inf) is never formed; the sum is Kahan-compensated (a bin the model explains has log_cdf of order
 *                  -1e-9, which n plain additions of terms near 1 would blur by n 2^-53).  So y_i = 0 gives log_cdf =
 *                  -inf, log_sf = 0 and pit = 0 exactly.
 *     mean_resid_i the mean (Welford) of y_i / M_is for chi(2,2p), of r for chi_square.
 *     pit_i        from the smaller tail, on the host: exp(log_cdf) if log_cdf < log_sf, else -expm1(log_sf).
 *     With n = 0 everything is NaN (and the two bins of the totals are -1).
 *   Totals, on the host in long double and in bin order: n_used, n_rejected; ks_D = max_k max((k + 1) / Nx - u_k, u_k -
 *   k / Nx) over the pit sorted ascending as u_0 <= ... <= u_{Nx-1}, the Kolmogorov distance from uniform; pit_hist, the
 *   count of bins in cell min(19, floor(20 pit)); min_log_sf with its bin (the strongest unexplained excess) and
 *   min_log_cdf with its bin (the strongest deficit), the first bin winning a tie.
 *   predictive_enable   allowed only while the object holds no sample (fresh, or after tamcmc_summary_reset) and is in fold
 *                mode.  Allocates 56 Nx bytes of state; TAMCMC_E_NOMEM when that fails, and the object stays as it was.
 *                Refused with TAMCMC_E_INVALID: a chi(2,2p) context with p < 1 or p > TAMCMC_SUMMARY_PREDICTIVE_MAX_P, a
 *                second call, samples already pushed, quantile or LOO mode, a context with a batch armed or in flight.
 *                Stays on until tamcmc_summary_destroy; tamcmc_summary_reset clears the state and keeps the setting.
 *   While enabled, the fold kernel runs unchanged -- every result of tamcmc_summary_result keeps its bits -- and passes
 *   pushed in quantile mode or LOO mode do not touch the predictive state.  Every result is bit for bit independent of
 *   block_chains and of how the samples are split over pushes.
 *   predictive_result   synchronises the stream; may be called between pushes, in any mode and repeatedly, and disturbs
 *                nothing.  totals and four arrays of Nx doubles on the host, any of them may be NULL.  TAMCMC_E_INVALID
 *                when the check is not enabled, and (as tamcmc_summary_result) with a batch in flight or armed.
 *   predictive_kernel_time   as tamcmc_summary_kernel_time, for the predictive kernel alone, under the same
 *                tamcmc_summary_profile switch; tamcmc_summary_kernel_time keeps reporting the fold kernel alone.
 *                Refused exactly as tamcmc_summary_kernel_time is (NULL arguments, a batch armed; a batch in flight is
 *                not refused: its stream is waited for), and with TAMCMC_E_INVALID when the check is not enabled.
 *
 * WINDOWED PREDICTIVE CHECK: the same question over groups of bins.  An unfitted mode of modest height is tens to hundreds
 * of bins wide with y / M of 2 ... 4 in each: per bin that is log_sf of -2 ... -4, and on a 1e5-bin grid the model's own
 * noise reaches -11.5 somewhere.  The sum over a window of len independent bins is Gamma-distributed with shape p len (the
 * H0 test on binned spectra, Appourchaux 2004; this is its posterior version): twenty bins at a mean ratio of 2 give
 * log Q(20, 40) = -8.6, at a ratio of 4 log Q(20, 80) = -35.8.  Like the per-bin check a setting of the object and no pass
 * of its own: every fold-mode block runs three more kernels (tamcmc_window.hip) behind the fold kernel -- and behind the
 * predictive kernel where that is on -- on the same rows and the same stream.
 *   Windows: disjoint, covering the grid.  W = bins per window, 1 ... TAMCMC_SUMMARY_WINDOW_MAX_BINS; first = the length of
 *   the first window, 1 ... W, 0 meaning W (a second object or run with another `first` has staggered windows, so that a
 *   feature cut by a boundary in one is whole in the other).  Window 0 is bins [0, min(first, Nx)), window w >= 1 is
 *   [first + (w-1) W, min(first + w W, Nx)), len_w its number of bins, n_windows = 1 + ceil(max(Nx - first, 0) / W).
 *   Definition, per window w, over the n = n_used accepted samples s (exactly the samples the fold kernel counts):
 *     chi(2,2p)    S_sw = sum_{i in w} y_i / M_is, one division per bin, added in ascending bin order without FMA
 *                  contraction; z = (double)p S_sw; shape a_w = p len_w; P_sw = P(a_w, z), Q_sw = Q(a_w, z), the regularised
 *                  incomplete gamma functions; z <= 0: P = 0, Q = 1.  p = likelihood_p truncated, as everywhere.
 *     chi_square   R_sw = sum_{i in w} (y_i - M_is) sqrt(isig2_i) in the same order; g = R_sw c_w with c_w = 1 /
 *                  sqrt((double)len_w) formed on the host; P_sw = erfc(-g) / 2, Q_sw = erfc(g) / 2.  The likelihood is taken
 *                  at its word as per bin: each r has standard deviation 1 / sqrt(2), and so has g.
 *     log_cdf_w = log((1/n) sum_s P_sw)        log_sf_w = log((1/n) sum_s Q_sw)
 *                  the per-bin check's guarded, compensated log-sum-exp in push order, unchanged; both tails of a sample as
 *                  logarithms by the per-bin check's forms at shape a_w, the largest term written about its maximum
 *                  where a window has two or more bins (tamcmc_window.h has the forms and their measured error: a few
 *                  ulp of max(1, |value|) at shape 1 and for chi_square, 3.2e-14 at shape 512).
 *     mean_resid_w the mean (Welford) over s of S_sw / len_w (chi(2,2p)) or R_sw / len_w (chi_square).
 *     pit_w        from the smaller tail, on the host, as per bin.   With n = 0 everything is NaN (the two windows of the
 *                  totals are -1).
 *   W = 1 is the per-bin check: c_1 = 1.0, S / 1 = S, and p (y / M) = (p y) / M where p is a power of two -- bit for bit then.
 *   Totals, on the host in long double and in window order: n_used, n_rejected, n_windows, W, first (as resolved: never 0);
 *   ks_D and pit_hist over the window PITs as for the bins; min_log_sf with win_min_log_sf and min_log_cdf with
 *   win_min_log_cdf, the first window winning a tie.
 *   window_enable   allowed only while the object holds no sample (fresh, or after tamcmc_summary_reset) and is in fold mode,
 *                once per object; *n_windows (may be NULL) gets the number of windows.  Allocates 7 n_windows doubles of
 *                state plus 3 block_chains n_windows doubles of scratch on the device; TAMCMC_E_NOMEM when that fails, and
 *                the object stays as it was.  Refused with TAMCMC_E_INVALID: W outside 1 ... TAMCMC_SUMMARY_WINDOW_MAX_BINS,
 *                first outside 0 ... W, a chi(2,2p) context with p < 1 or p W > TAMCMC_SUMMARY_WINDOW_MAX_SHAPE (the form of
 *                Q in use overflows past a shape of about 700), a second call, samples already pushed, quantile or LOO mode,
 *                a context with a batch armed or in flight.  Stays on until tamcmc_summary_destroy; tamcmc_summary_reset
 *                clears the state and keeps the setting.  Independent of predictive_enable: either, both, in either order.
 *   While enabled, the fold kernel and the predictive kernel run unchanged -- tamcmc_summary_result and
 *   tamcmc_summary_predictive_result keep their bits -- and passes pushed in quantile mode or LOO mode do not touch the
 *   windows' state.  Every result is bit for bit independent of block_chains and of how the samples are split over pushes.
 *   window_result   as predictive_result, with arrays of n_windows doubles: synchronises the stream; may be called between
 *                pushes, in any mode and repeatedly, and disturbs nothing; totals and any array may be NULL.
 *                TAMCMC_E_INVALID when the check is not enabled, and with a batch in flight or armed.
 *   window_kernel_time   as predictive_kernel_time, for the three window kernels of a block together (one event pair per
 *                block), under the same tamcmc_summary_profile switch, refused in the same cases.
 *
 * SLIDING-WINDOW PREDICTIVE SCAN: the windowed check at every start position and for several widths at once.  The disjoint
 * windows above dilute a feature that one of their boundaries cuts, and take one width per object; the documented remedy, a
 * second pass with another `first` or another W, costs a pass over the chain each.  The scan is a third setting of the
 * object beside predictive_enable and window_enable: every fold-mode block runs the kernels of tamcmc_scan.hip behind the
 * window kernels, on the same rows and the same stream.
 *   Widths: a strictly ascending list W_0 < ... < W_{K-1}, 1 <= K <= TAMCMC_SUMMARY_SCAN_MAX_WIDTHS, each 1 ...
 *   TAMCMC_SUMMARY_WINDOW_MAX_BINS and at most Nx.  Width k has the positions j = 0 ... Nx - W_k, n_pos_k = Nx - W_k + 1 of them;
 *   the window of position j is the bins [j, j + W_k).  Every window is full.
 *   Definition, per (accepted sample s, width k, position j), exactly as for a full window of W_k bins of the disjoint check:
 *   the sum S (R) over the window's bins in ascending bin order starting from the first term, without FMA contraction -- the
 *   sums of all widths at one position are prefixes of one ascending sum, so their bits are those of separate sums --, the
 *   two tails at the shape p W_k (c = 1 / sqrt((double)W_k)), log_cdf and log_sf by the guarded, compensated log-sum-exp in
 *   push order, mean_resid the Welford mean of S / (double)W_k, pit from the smaller tail on the host.  Position j of width W
 *   equals window w of window_enable(W, first) wherever that window is full and starts at bin j, bit for bit in all four
 *   arrays.  With n = 0 everything is NaN.
 *   Totals per width, on the host in position order, the first position winning a tie and a NaN skipped: n_used, n_rejected,
 *   W, n_positions; min_log_sf with pos_min_log_sf and min_log_cdf with pos_min_log_cdf (a position of -1: every value was NaN).
 *   There is no ks_D and no pit_hist: overlapping windows are not independent, and a uniformity test over them would mislead.
 *   Regions, on the host: for a width k, a side `which` (0: log_sf, an excess; 1: log_cdf, a deficit) and a line log_below < 0,
 *   a region is a maximal run of consecutive positions whose value is below the line (a NaN is never below it): {pos_first,
 *   pos_last, bin_first = pos_first, bin_last = pos_last + W_k - 1, pos_min = the first position of the run's minimum,
 *   min_log, mean_resid_at_min}, in position order.  log_below = NaN picks log(0.01 * (double)W_k / (double)Nx), the Bonferroni
 *   line at 1 % over Nx / W_k independent windows.
 *   scan_enable  allowed only while the object holds no sample (fresh, or after tamcmc_summary_reset) and is in fold mode, once
 *                per object.  With total = sum_k n_pos_k it allocates 56 total bytes of state plus 24 C total bytes of scratch
 *                on the device, C = max(1, min(block_chains, 4096, 256 MiB / (24 total bytes))) samples: a block with more
 *                samples is worked in chunks of C, which cannot change a bit.  At most 256 MiB of scratch, or 24 total bytes
 *                where one sample takes more -- Nx = 1e5 with eight widths: 19 MB a sample, C = 13, and 45 MB of state.
 *                TAMCMC_E_NOMEM when that fails, and the object stays as it was.  Refused with TAMCMC_E_INVALID: n_widths
 *                outside 1 ... TAMCMC_SUMMARY_SCAN_MAX_WIDTHS, a NULL list, a width outside 1 ... TAMCMC_SUMMARY_WINDOW_MAX_BINS
 *                or above Nx, widths not strictly ascending, a chi(2,2p) context with p < 1 or p W_{K-1} >
 *                TAMCMC_SUMMARY_WINDOW_MAX_SHAPE, a second call, samples already pushed, quantile, LOO or ESS mode, a context
 *                with a batch armed or in flight.  Stays on until tamcmc_summary_destroy; tamcmc_summary_reset clears the state
 *                and keeps the setting.  Independent of predictive_enable and window_enable: any combination, in any order.
 *   While enabled, the fold, predictive and window kernels run unchanged -- their results keep their bits -- and passes pushed
 *   in quantile, LOO or ESS mode do not touch the scan's state.  Every scan result is bit for bit independent of block_chains,
 *   of how the samples are split over pushes, and of which other widths are in the list.
 *   scan_result  width k = 0 ... K-1: totals and four arrays of n_pos_k doubles on the host, any of them may be NULL.
 *                Synchronises the stream; may be called between pushes, in any mode and repeatedly, and disturbs nothing.
 *                TAMCMC_E_INVALID: k out of range, the scan not enabled, a batch in flight or armed.
 *   scan_regions as scan_result.  Always writes the number of regions to *n_regions and fills at most max_regions records, the
 *                first ones in position order; regions == NULL with max_regions == 0 only counts.  TAMCMC_E_INVALID also for
 *                which outside 0 ... 1, log_below >= 0, max_regions < 0, a NULL n_regions, NULL regions with max_regions > 0.
 *   scan_kernel_time   as window_kernel_time, for all scan kernels of a block together (one event pair per block), under the
 *                same tamcmc_summary_profile switch, refused in the same cases.
 *
 * EFFECTIVE SAMPLE SIZE, MCSE AND SPLIT R-HAT: every number above is a Monte-Carlo estimate over an autocorrelated chain;
 * this says per bin how many independent draws the chain is worth (Geyer's initial monotone sequence on the
 * autocorrelation over the sample order, as Stan uses for one chain), the Monte-Carlo standard error of mean_M that
 * follows, the split R-hat of the two halves of the chain, and the relative efficiency r_eff the `loo` literature expects
 * beside k-hat.  A fourth mode beside fold, quantile and LOO mode: after the fold pass the caller pushes the SAME samples
 * once more, in the same order.
 *   Definition, per bin i, with n = n_used and t = 0 ... n - 1 counting the accepted samples in push order (a rejected
 *   sample is skipped and counted and does not advance t: lags are counted in accepted samples):
 *     1. Two series, centred with the frozen fold results (the very doubles tamcmc_summary_result returns):
 *          model        a_t = M_it - mean_M_i
 *          likelihood   u_t = exp(l_it - lppd_i) - 1.0, l restated without FMA contraction as in LOO mode.  The mean of
 *                       exp(l - lppd) is 1 by construction and l - lppd <= log n: nothing overflows.
 *     2. Lag limit: L = the largest odd number <= min(max_lag | 1, n - 1); max_lag = 0 picks the library's default, 255.
 *     3. Lag products, for each series d: A_k = sum_{t=k}^{n-1} d_t d_{t-k}, k = 0 ... L, each accumulated from +0.0 in
 *        ascending t by A = fma(d_t, d_{t-k}, A): the product is not rounded before it is added (tamcmc_ess.h).
 *     4. Finish, in double, in this order, without contraction: rho_k = A_k / A_0; P_m = rho_{2m} + rho_{2m+1} for
 *        m = 0 ... (L-1)/2; K = the first m for which P_m >= 0 does not hold (a NaN stops the sum too), K = (L+1)/2 if there
 *        is none; P_m = min(P_m, P_{m-1}) for m = 1 ... K-1; tau = -1 + 2 sum_{m<K} P_m in ascending m; tau = max(tau,
 *        1 / log10(n)), the log10 evaluated on the host; ess = n / tau; cut = 2K, and cut = L + 1 says the bin was truncated:
 *        the sequence had not turned negative within L lags and ess is an upper bound.  A_0 zero or not finite: ess = tau
 *        = NaN, cut = 0.
 *     5. Split R-hat of the model series: h = floor(n / 2), the halves t in [0, h) and [n - h, n), each with its own
 *        Welford mean m and sum of squared deviations M2 of M_it accumulated in push order on the device; on the host
 *        s^2 = M2 / (h - 1), W = (s1^2 + s2^2) / 2, Bn = (m1 - mb)^2 + (m2 - mb)^2 with mb = (m1 + m2) / 2,
 *        rhat = sqrt(((h - 1) / h * W + Bn) / W); W = 0: NaN.
 *     6. Per bin: ess_M, tau_M, cut_M; mcse_M = sqrt(var_M / ess_M) with the frozen var_M; rhat_M; ess_l, cut_l,
 *        r_eff = ess_l / n.
 *     7. Totals, on the host in bin order, the first bin winning a tie and a NaN skipped (a bin of -1: every value was NaN):
 *        n_used, n_rejected, lag = L; min_ess_M with bin_min_ess_M, min_ess_l with bin_min_ess_l, max_rhat with
 *        bin_max_rhat; n_truncated_M, n_truncated_l = bins with cut = L + 1; n_rhat_high = bins with rhat > 1.01.
 *   ess_begin    freezes the fold state as loo_begin does, resolves L (*lag_used, may be NULL) and allocates on the device,
 *                per series, (L + 1) x Nx accumulators and a ring of L + 64 centred values per bin (the last L are the carry
 *                that bridges blocks and pushes, 64 is the number of samples one pair of launches takes), plus 4 Nx doubles
 *                of half-chain moments, Nx of lppd and 5 Nx of results: (32 L + 1120) Nx + 32 bytes in all -- 0.93 GB for Nx =
 *                1e5 at L = 255.  TAMCMC_E_NOMEM when that fails, and the object stays as it was.  Refused with
 *                TAMCMC_E_INVALID: n_used < 4, max_lag outside 0 ... TAMCMC_SUMMARY_ESS_MAX_LAG, any mode already on
 *                (tamcmc_summary_quantiles_begin and tamcmc_summary_loo_begin are likewise refused while ESS mode is on, and
 *                so are predictive_enable, window_enable and scan_enable), a context with a batch in flight or armed.
 *   While the mode is on, push and push_device evaluate the rows as before and hand out the same logL and status bits, but
 *   feed the ESS kernels (tamcmc_ess.hip) instead of the fold kernel; tamcmc_summary_result keeps returning the frozen fold
 *   results, and the predictive and window states are not touched.  Every (bin, lag) accumulator is advanced by one
 *   thread in sample order, so every result is bit for bit independent of block_chains and of how the pass is split over
 *   pushes -- pushes shorter than L and pushes of one sample included.
 *   ess_result   totals and eight arrays of Nx on the host, any of them may be NULL.  If the pass did not see exactly the
 *                fold pass's accepted and rejected counts: TAMCMC_E_INVALID, the pass is discarded and may be repeated.  May
 *                be called again without another pass.
 *   ess_acov     the lag products of a complete pass: which = 0 the model series, 1 the likelihood series; acov is
 *                (L + 1) x Nx on the host, A_k of bin i at acov[k * Nx + i].  TAMCMC_E_INVALID for an incomplete pass (which
 *                it leaves alone), a NULL acov, which outside 0 ... 1.
 *   ess_end      frees the mode's memory and goes back to fold mode: the running statistics are untouched and further
 *                pushes fold as before.  tamcmc_summary_reset also leaves the mode; tamcmc_summary_destroy works in any.
 *                _result, _acov and _end outside the mode return TAMCMC_E_INVALID.
 *   profile / kernel_time in ESS mode: the centre and lag kernels of every block together (one event pair per block), and
 *   the finish kernel of every ess_result.
 *
 * ESS AND MCSE OF THE CREDIBLE-BAND EDGES (band ESS mode): the quantiles above are Monte-Carlo estimates too, and the ESS of
 * mean_M does not say how well they are determined: a chain worth 2000 independent draws for the mean can be worth 150 for
 * its 2.5 % edge.  Following Vehtari et al. (2021), the ESS of a quantile estimate is the ESS of the indicator series
 * I(M_t <= q) at the quantile's value (their tail-ESS is the smaller of the two at the 5 % and 95 % values).  A fifth mode
 * beside fold, quantile, LOO and ESS mode: after the fold pass the caller pushes the SAME samples once more, in the same order.
 * The thresholds are whatever the caller hands in -- normally the resolved lo == hi of the quantile selection -- and the mode
 * does not depend on quantile mode.  An indicator is 0 or 1, so everything on the device up to one conversion is exact
 * integer arithmetic.
 *   Definition, per threshold j (K arrays of Nx doubles, 1 <= K <= TAMCMC_SUMMARY_MAX_QUANTILES) and bin i, with n = n_used and
 *   t = 0 ... n - 1 counting the accepted samples in push order (a rejected sample is skipped and counted and does not advance t):
 *     1. Series: b_t = (M_it <= thr_ji), the IEEE comparison of doubles: -0 = +0, and a NaN threshold gives 0 throughout.
 *     2. Lag limit: L as in ESS mode, from max_lag and n.
 *     3. Counts, exact integers: N = sum b_t; C_k = sum_{t=k}^{n-1} b_t b_{t-k}, k = 0 ... L; H_k = sum_{t<k} b_t (the first k
 *        samples); T_k = sum_{t>=n-k} b_t (the last k).
 *     4. Centred lag products times n^2, still exact: E_k = n^2 C_k - n N (2N - H_k - T_k) + (n - k) N^2
 *        = n^2 sum_{t=k}^{n-1} (b_t - N/n)(b_{t-k} - N/n), held in int64_t (|E_k| < 2^62 for n < 2^20); E_0 = n N (n - N).
 *     5. Finish: A_k = (double)E_k, one rounding, then step 4 of ESS mode on A_0 ... A_L as it stands: the same rule, the same
 *        1 / log10(n) from the host, the same meaning of cut.  A constant series (N = 0 or N = n) has A_0 = 0: tau = ess = NaN,
 *        cut = 0.
 *     6. Per (j, bin), at [j * Nx + i]: count_le = N; ess, tau, cut; p_hat = (double)N / (double)n;
 *        mcse_p = sqrt(p_hat * (1.0 - p_hat) / ess), on the host in that order, without contraction.
 *     7. Totals, per threshold, on the host in bin order, the first bin winning a tie and a NaN skipped (a bin of -1: every
 *        value was NaN): n_used, n_rejected, lag = L, n_thresholds = K; min_ess[j] with bin_min_ess[j]; n_truncated[j] = bins
 *        with cut = L + 1; n_constant[j] = bins with N = 0 or N = n.  Entries j >= K: NaN, -1, 0, 0.
 *   bandess_begin   freezes the fold state as ess_begin does, copies the thresholds (thr[j * Nx + i]), resolves L (*lag_used, may
 *                be NULL) and allocates on the device: the series as ONE BIT per sample -- per threshold and bin a ring of
 *                ceil(L / 64) + 2 64-bit words (the chunk under way and the L bits before it) and the first ceil(L / 64) words
 *                for H_k --, (L + 1) 32-bit counters per threshold and bin, one column of L + 1 doubles per bin that the
 *                thresholds share at the finish, and 28 K bytes per bin of thresholds and results:
 *                ((4 K + 8) (L + 1) + 16 K (ceil(L / 64) + 1) + 28 K) Nx + 32 bytes in all -- 0.54 GB for Nx = 1e5 at L = 255 and
 *                K = 3.  TAMCMC_E_NOMEM when that fails, and the object stays as it was.  Refused with TAMCMC_E_INVALID: what
 *                ess_begin refuses (n_used < 4, max_lag outside 0 ... TAMCMC_SUMMARY_ESS_MAX_LAG, any mode already on, a batch in
 *                flight or armed), K outside 1 ... 8, NULL thr, n_used >= 2^20 (thin the chain).  While the mode is on,
 *                quantiles_begin, loo_begin, ess_begin, predictive_enable, window_enable and scan_enable are refused.
 *   While the mode is on, push and push_device evaluate the rows as before and hand out the same logL and status bits, but
 *   feed the band kernels (tamcmc_bandess.hip) instead of the fold kernel; tamcmc_summary_result keeps returning the frozen fold
 *   results, and the predictive, window and scan states are not touched.  Integer sums do not depend on the order of their
 *   terms: every result is bit for bit independent of block_chains and of how the pass is split over pushes.
 *   bandess_result  totals and six arrays of K x Nx on the host, any of them may be NULL.  If the pass did not see exactly the
 *                fold pass's accepted and rejected counts: TAMCMC_E_INVALID, the pass is discarded and may be repeated.  May
 *                be called again without another pass.
 *   bandess_counts  of a complete pass and threshold j: C_k (they fit int32_t) and E_k, each (L + 1) x Nx on the host, lag k of
 *                bin i at [k * Nx + i]; either may be NULL.  TAMCMC_E_INVALID for an incomplete pass (which it leaves alone)
 *                and for j outside 0 ... K - 1.
 *   bandess_end     frees the mode's memory and goes back to fold mode.  tamcmc_summary_reset also leaves the mode;
 *                tamcmc_summary_destroy works in any.  _result, _counts and _end outside the mode return TAMCMC_E_INVALID.
 *   profile / kernel_time in the mode: the pack and lag kernels of every block together (one event pair per block), and the
 *   finish kernel of every bandess_result (one launch per threshold).
 *   Not here: the MCSE of a quantile on the value scale, which needs order statistics at ranks that differ from bin to bin, and
 *   rank-normalised bulk ESS, which needs per-bin ranks of every sample. */
typedef struct tamcmc_summary tamcmc_summary;
typedef struct {
    int64_t n_used, n_rejected;
    double lppd_total, p_waic, waic;
} tamcmc_summary_totals;
int tamcmc_summary_create(tamcmc_summary **out, tamcmc_ctx *ctx, int32_t block_chains);
int tamcmc_summary_push(tamcmc_summary *s, int32_t Nsamples, int32_t Nparams, const double *params,
                        double *logL, int32_t *status);
int tamcmc_summary_push_device(tamcmc_summary *s, int32_t Nsamples, int32_t Nparams, const double *d_params,
                               double *d_logL, int32_t *d_status);
int tamcmc_summary_result(tamcmc_summary *s, tamcmc_summary_totals *totals,
                          double *mean_M, double *var_M, double *min_M, double *max_M,
                          double *mean_l, double *var_l, double *lppd);
int tamcmc_summary_reset(tamcmc_summary *s);
int tamcmc_summary_destroy(tamcmc_summary *s);
int tamcmc_summary_profile(tamcmc_summary *s, int enable);
int tamcmc_summary_kernel_time(tamcmc_summary *s, double *total_ms, int64_t *launches);
#define TAMCMC_SUMMARY_MAX_QUANTILES 8
int tamcmc_summary_quantiles_begin(tamcmc_summary *s, int32_t Nq, const double *q, int32_t bits_per_pass);
int tamcmc_summary_quantiles_step(tamcmc_summary *s, int32_t *bits_left);
int tamcmc_summary_quantiles_result(tamcmc_summary *s, int64_t *ranks, double *lo, double *hi);
int tamcmc_summary_quantiles_end(tamcmc_summary *s);
#define TAMCMC_SUMMARY_LOO_MAX_TAIL 2048
typedef struct {
    int64_t n_used, n_rejected;
    double elpd_loo, p_loo, looic, k_max;
    int64_t n_k_high, n_k_inf;
} tamcmc_summary_loo_totals;
int tamcmc_summary_loo_begin(tamcmc_summary *s);
int tamcmc_summary_loo_result(tamcmc_summary *s, tamcmc_summary_loo_totals *totals,
                              double *elpd_loo, double *pareto_k, double *cutoff, int32_t *tail_len);
int tamcmc_summary_loo_end(tamcmc_summary *s);
#define TAMCMC_SUMMARY_PREDICTIVE_MAX_P 64
#define TAMCMC_SUMMARY_PIT_CELLS 20
typedef struct {
    int64_t n_used, n_rejected;
    double ks_D, min_log_sf, min_log_cdf;
    int64_t bin_min_log_sf, bin_min_log_cdf;
    int64_t pit_hist[TAMCMC_SUMMARY_PIT_CELLS];
} tamcmc_summary_predictive_totals;
int tamcmc_summary_predictive_enable(tamcmc_summary *s);
int tamcmc_summary_predictive_result(tamcmc_summary *s, tamcmc_summary_predictive_totals *totals,
                                     double *pit, double *log_cdf, double *log_sf, double *mean_resid);
int tamcmc_summary_predictive_kernel_time(tamcmc_summary *s, double *total_ms, int64_t *launches);
typedef struct {
    int64_t n_used, n_rejected;
    double ks_D, min_log_sf, min_log_cdf, min_is_ess;
    int64_t bin_min_log_sf, bin_min_log_cdf, bin_min_is_ess;
    int64_t pit_hist[TAMCMC_SUMMARY_PIT_CELLS];
} tamcmc_summary_loo_pit_totals;
int tamcmc_summary_loo_pit_begin(tamcmc_summary *s);
int tamcmc_summary_loo_pit_result(tamcmc_summary *s, tamcmc_summary_loo_pit_totals *totals,
                                  double *loo_pit, double *loo_log_cdf, double *loo_log_sf, double *is_ess, double *log_wsum);
int tamcmc_summary_loo_pit_kernel_time(tamcmc_summary *s, double *total_ms, int64_t *launches);
#define TAMCMC_SUMMARY_WINDOW_MAX_BINS 512
#define TAMCMC_SUMMARY_WINDOW_MAX_SHAPE 512
typedef struct {
    int64_t n_used, n_rejected, n_windows, W, first;
    double ks_D, min_log_sf, min_log_cdf;
    int64_t win_min_log_sf, win_min_log_cdf;
    int64_t pit_hist[TAMCMC_SUMMARY_PIT_CELLS];
} tamcmc_summary_window_totals;
int tamcmc_summary_window_enable(tamcmc_summary *s, int32_t W, int32_t first, int32_t *n_windows);
int tamcmc_summary_window_result(tamcmc_summary *s, tamcmc_summary_window_totals *totals,
                                 double *pit, double *log_cdf, double *log_sf, double *mean_resid);
int tamcmc_summary_window_kernel_time(tamcmc_summary *s, double *total_ms, int64_t *launches);
typedef struct {
    int64_t n_used, n_rejected, n_windows, W, first;
    double elpd_lwo, p_lwo, k_max;
    int64_t n_k_high, n_k_inf;
} tamcmc_summary_wloo_totals;
int tamcmc_summary_wloo_begin(tamcmc_summary *s, int32_t W, int32_t first, int32_t *n_windows);
int tamcmc_summary_wloo_result(tamcmc_summary *s, tamcmc_summary_wloo_totals *totals,
                               double *elpd_lwo, double *pareto_k, double *cutoff, int32_t *tail_len,
                               int64_t *first_bin, int64_t *last_bin);
int tamcmc_summary_wloo_pit_begin(tamcmc_summary *s);
int tamcmc_summary_wloo_pit_result(tamcmc_summary *s, tamcmc_summary_loo_pit_totals *totals,
                                   double *loo_pit, double *loo_log_cdf, double *loo_log_sf, double *is_ess, double *log_wsum);
int tamcmc_summary_wloo_pit_kernel_time(tamcmc_summary *s, double *total_ms, int64_t *launches);
int tamcmc_summary_wloo_end(tamcmc_summary *s);
#define TAMCMC_SUMMARY_SCAN_MAX_WIDTHS 8
typedef struct {
    int64_t n_used, n_rejected, W, n_positions;
    double min_log_sf, min_log_cdf;
    int64_t pos_min_log_sf, pos_min_log_cdf;
} tamcmc_summary_scan_totals;
typedef struct {
    int64_t pos_first, pos_last, bin_first, bin_last, pos_min;
    double min_log, mean_resid_at_min;
} tamcmc_summary_scan_region;
int tamcmc_summary_scan_enable(tamcmc_summary *s, int32_t n_widths, const int32_t *W);
int tamcmc_summary_scan_result(tamcmc_summary *s, int32_t k, tamcmc_summary_scan_totals *totals,
                               double *pit, double *log_cdf, double *log_sf, double *mean_resid);
int tamcmc_summary_scan_regions(tamcmc_summary *s, int32_t k, int32_t which, double log_below,
                                int32_t max_regions, tamcmc_summary_scan_region *regions, int32_t *n_regions);
int tamcmc_summary_scan_kernel_time(tamcmc_summary *s, double *total_ms, int64_t *launches);
#define TAMCMC_SUMMARY_ESS_MAX_LAG 1023
typedef struct {
    int64_t n_used, n_rejected, lag;
    double min_ess_M, min_ess_l, max_rhat;
    int64_t bin_min_ess_M, bin_min_ess_l, bin_max_rhat;
    int64_t n_truncated_M, n_truncated_l, n_rhat_high;
} tamcmc_summary_ess_totals;
int tamcmc_summary_ess_begin(tamcmc_summary *s, int32_t max_lag, int32_t *lag_used);
int tamcmc_summary_ess_result(tamcmc_summary *s, tamcmc_summary_ess_totals *totals,
                              double *ess_M, double *tau_M, double *mcse_M, double *rhat_M, int32_t *cut_M,
                              double *ess_l, double *r_eff, int32_t *cut_l);
int tamcmc_summary_ess_acov(tamcmc_summary *s, int32_t which, double *acov);
int tamcmc_summary_ess_end(tamcmc_summary *s);
typedef struct {
    int64_t n_used, n_rejected, lag, n_thresholds;
    double  min_ess[TAMCMC_SUMMARY_MAX_QUANTILES];
    int64_t bin_min_ess[TAMCMC_SUMMARY_MAX_QUANTILES],
            n_truncated[TAMCMC_SUMMARY_MAX_QUANTILES],
            n_constant[TAMCMC_SUMMARY_MAX_QUANTILES];
} tamcmc_summary_bandess_totals;
int tamcmc_summary_bandess_begin(tamcmc_summary *s, int32_t K, const double *thr, int32_t max_lag, int32_t *lag_used);
int tamcmc_summary_bandess_result(tamcmc_summary *s, tamcmc_summary_bandess_totals *totals,
                                  int32_t *count_le, double *p_hat, double *ess, double *tau,
                                  double *mcse_p, int32_t *cut);
int tamcmc_summary_bandess_counts(tamcmc_summary *s, int32_t j, int32_t *C, int64_t *E);
int tamcmc_summary_bandess_end(tamcmc_summary *s);

/* MONTE-CARLO NULL OF THE SCAN: the law of the sliding-window scan's extremes under a correctly specified model, and the
 * lines and p-values that follow from it.  The scan's default line log(0.01 W / Nx) is Bonferroni over Nx / W independent
 * windows, per width: neither the overlap of neighbouring positions nor the several widths enter it, and a pure-noise
 * spectrum crosses it several times more often than the 1 % it names.  If the model is right, y_i / M_i is Gamma(p, 1 / p)
 * for chi(2,2p) and r_i is N(0, 1/2) for chi_square, independent of the model: the null distribution of the scan's extremes
 * depends on (likelihood, p, Nx, widths) alone.  An object of its own, bound to a device and to no context or chain; it
 * simulates R replicate noise spectra on the device (tamcmc_scan_null.hip), the scan's own sums over them, and keeps per
 * (replicate, width) the two extreme sums.  Nothing of size R x Nx ever exists in memory.
 *   Generator: Philox4x32-10 -- multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten rounds --
 *   with key = (seed low 32 bits, seed high 32 bits) and counter = (bin i, pair index t, replicate low 32 bits, replicate high
 *   32 bits), the replicate being the GLOBAL one, first_replicate + r.  The output words (w0, w1, w2, w3) give two uniforms,
 *     u = ((double)(((uint64_t)wa << 20) | (wb >> 12)) + 0.5) * 2^-52,   u_even from (w0, w1), u_odd from (w2, w3):
 *   each exact and strictly inside (0, 1).
 *   Variate of bin i, replicate r:
 *     chi(2,2p)    e_k = -log(u_k), k = 0 ... p-1, u_k the (k & 1)-th uniform of call t = k >> 1; z = e_0 + e_1 + ... in
 *                  ascending k without FMA contraction; q_i = z / (double)p.  p = likelihood_p truncated, as everywhere.
 *     chi_square   q_i = sqrt(-log(u_even)) * cospi(2.0 * u_odd) of call t = 0: variance 1/2, the likelihood taken at its
 *                  word as in the predictive check.
 *   Sums: for width k and position j, S = the scan's ascending sum of q[j ... j + W_k), all widths prefixes of one walk.  Per
 *   (replicate, width): S_max with its first position and S_min with its first position.
 *   Statistic, on the host with the functions the scan's tails use, without FMA contraction: which = 0 (excess): min_log =
 *   log Q at S_max, at the shape p W_k (c = 1 / sqrt((double)W_k)); which = 1 (deficit): log P at S_min.  The tails are
 *   monotone in S, so this is the minimum over positions of what the scan computes for a chain of one sample.
 *   Calibration: integer counting over the R replicates done so far, per side.  With m[r][k] = min_log and cnt[r][k] =
 *   #{r' : m[r'][k] <= m[r][k]}:  vmin[r] = min_k cnt[r][k];  p_width(v) = (1 + n_v) / (R + 1) with n_v = #{r : m[r][k] <= v};
 *   p_joint(v) = (1 + #{r : vmin[r] <= n_v}) / (R + 1).  The line at level alpha, with j = floor(alpha (R + 1)): per width the
 *   j-th smallest m[.][k]; jointly the c-th smallest m[.][k], where c is the j-th smallest vmin.  The joint line is never
 *   above the per-width line.
 *   What it calibrates: the multiplicity over overlapping positions and several widths under a correctly specified model.
 *   The chain's statistic is a posterior average of per-sample tails, never more extreme than the plug-in value simulated
 *   here.  The fit's own degrees of freedom -- a window over a fitted mode -- are not accounted for.
 *   create       widths, p and their limits exactly as tamcmc_summary_scan_enable, refused the same way (TAMCMC_E_INVALID; a
 *                likelihood_case other than 0 or 1: TAMCMC_E_UNKNOWN_MODEL); Nx >= 1; first_replicate >= 0.  Every argument
 *                is checked before a device is touched; TAMCMC_E_NODEVICE without a usable device.  Allocates the partials of
 *                one chunk of replicates, at most 64 MiB, on the device.  chi_square ignores likelihood_p.
 *   run          appends n_replicates >= 1 replicates; synchronous.  At most TAMCMC_SCAN_NULL_MAX_REPLICATES in all,
 *                TAMCMC_E_INVALID beyond.  Replicate r is bit for bit the same however the replicates are split over runs,
 *                whichever other widths are in the list, and for an object created at first_replicate = r.
 *   result       width k, side which: R doubles / int64 each, any may be NULL.
 *   line         TAMCMC_E_INVALID: k or which out of range, no replicate yet, a NULL log_below, j < 1 or j > R.
 *   pvalue       TAMCMC_E_INVALID likewise, and for a NaN value.
 *   variates     the Nx variates of replicate r >= 0 (run or not), generated on the device by the kernels' own function: for
 *                tests and plots.
 *   profile / kernel_time   as tamcmc_summary_profile / _kernel_time: one event pair around the kernels of each chunk. */
#define TAMCMC_SCAN_NULL_MAX_REPLICATES 16777216
typedef struct tamcmc_scan_null tamcmc_scan_null;
int tamcmc_scan_null_create(tamcmc_scan_null **out, int device_id, int likelihood_case, double likelihood_p, int64_t Nx,
                            int32_t n_widths, const int32_t *W, uint64_t seed, int64_t first_replicate);
int tamcmc_scan_null_run(tamcmc_scan_null *h, int64_t n_replicates);
int tamcmc_scan_null_replicates(const tamcmc_scan_null *h, int64_t *R);
int tamcmc_scan_null_result(tamcmc_scan_null *h, int32_t k, int32_t which, double *ext_sum, int64_t *pos, double *min_log);
int tamcmc_scan_null_line(tamcmc_scan_null *h, int32_t k, int32_t which, double alpha, int32_t joint, double *log_below);
int tamcmc_scan_null_pvalue(tamcmc_scan_null *h, int32_t k, int32_t which, double value, double *p_width, double *p_joint);
int tamcmc_scan_null_variates(tamcmc_scan_null *h, int64_t r, double *q);
int tamcmc_scan_null_profile(tamcmc_scan_null *h, int enable);
int tamcmc_scan_null_kernel_time(tamcmc_scan_null *h, double *total_ms, int64_t *launches);
int tamcmc_scan_null_destroy(tamcmc_scan_null *h);

/* ---- Posterior mode table: the derived mode parameters of a stored chain --------------------------------------------
 * Per params row the quantities the kernels derive from it -- the derivation of the setup and backward kernels, run on the
 * device for all 11 ids that have modes -- and their statistics over the rows pushed: count, mean, standard deviation,
 * minimum, maximum, exact quantiles.  The spectrum plays no part.
 *   Columns, a function of the context's layout alone (tamcmc_modetable_column describes each):
 *     chain level, first:   inclination (degrees), eta, a3, asymmetry.  The inclination is the one the m-height ratios are
 *       derived from: ids 2, 9, 10, 11 atan(p4 / p3) of the sqrt(a1) cos i, sqrt(a1) sin i pair, a value in [-90, 90] --
 *       the quotient's sign decides, not the quadrant of the pair (p3 = 0 gives +-90, p4 = 0 gives 0, both 0 a NaN);
 *       ids 3, 6, 7, 8 the inclination entry as given, bit for bit, never reduced (150 stays 150, -20 stays -20);
 *       ids 12, 13, 14, which have none, +0.
 *     per multiplet j = 0 ... n_mult - 1, in the chain's table order, l its degree:
 *       freq, width, height (= sum of the h_m, added in the order m = -l ... l), amplitude (= sqrt((pi height) width), the
 *       reference's H = A^2 / (pi Gamma)), splitting (exactly 0 for l = 0), window_lo, window_hi (the truncation window
 *       [lo, hi) in bins, as doubles), nu_m for m = -l ... l, h_m for m = -l ... l
 *     n_cols = 4 + sum_j (7 + 2 (2 l_j + 1)).  A row describes the sample's mode spectrum completely: with the noise
 *     parameters the model can be rebuilt from it.
 *   tamcmc_modetable_col: mult = -1 (and order = l = -1) for chain-level columns; order = the radial index n of the
 *     multiplet; m = 0 except on nu_m and h_m columns; param_index = the params index of the mode frequency on freq
 *     columns (the column equals that entry bit for bit), -1 elsewhere.
 *   Status of a sample: the largest status of its multiplets (an empty truncation window: TAMCMC_CHAIN_EMPTY_WINDOW), else
 *     TAMCMC_CHAIN_NAN when any of its columns is a NaN or the square of a width is infinite (Gamma > 1.34e154: the AppWidth
 *     width of id 9 with an exponent out of range), else TAMCMC_CHAIN_OK -- the code tamcmc_eval_batch gives a row whose
 *     noise parameters are healthy, with one exception, "finite columns, overflowing sum": a row whose columns are all
 *     finite and describe a finite model, but which has a width so large that the eval kernels' sum over the components of
 *     a multiplet overflows -- they multiply 2 l + 1 factors of the order Gamma^2, so from a Gamma near 2e51 for l = 1,
 *     1e31 for l = 2 and 1e22 for l = 3 (the AppWidth v2 width of id 10 with a reference frequency of 1e-6 is 3e37 ... 9e37;
 *     the AppWidth v1 width of id 9 with an exponent of 2600 where its largest value stays below 1.34e154).
 *     tamcmc_eval_batch gives such a row TAMCMC_CHAIN_NAN, the table TAMCMC_CHAIN_OK: the row is what the reference's
 *     formulas give, and the model rebuilt from it is the reference's.  A sample whose status is not OK, or whose entry of
 *     `skip` is not 0, enters neither the statistics nor the table, and is counted in n_rejected.
 *   create       max_samples >= 0 rows of the table are kept on the device for the quantiles: 8 max_samples n_cols bytes,
 *                plus 8 B (Nparams + n_cols + 1) bytes for a block of B = min(4096, 2^23 / n_cols) samples and
 *                128 n_cols + 64 bytes of state; TAMCMC_E_NOMEM when that fails.  max_samples = 0: statistics only.  Refused
 *                with TAMCMC_E_INVALID: NULL arguments, max_samples < 0 or >= 2^31, a context of model id 0 or 1 (no
 *                multiplets), a context with a batch in flight or armed.  tamcmc_ctx_destroy is refused while the object lives.
 *   columns / column   the numbers of columns and multiplets; the description of column col (TAMCMC_E_INVALID out of range).
 *   derive       the plain map: Nsamples x Nparams params rows -> Nsamples x n_cols rows (and status, which may be NULL), host
 *                pointers; nothing is accumulated or stored.
 *   push         derives the rows, folds the accepted ones into the statistics in push order and appends them to the table.
 *                skip (Nsamples entries) and status may be NULL.  A push after which the table would hold more than
 *                max_samples accepted rows (max_samples > 0) is refused whole with TAMCMC_E_INVALID: nothing changes, status
 *                is not written.  No result bit depends on how the rows are cut into pushes.
 *   result       totals and four arrays of n_cols doubles, any may be NULL; sd with n - 1, NaN for fewer than two samples (every
 *                array NaN for none).
 *   quantiles    Nq = 1 ... TAMCMC_SUMMARY_MAX_QUANTILES probabilities in [0, 1]; ranks (Nq, may be NULL) are those of numpy's
 *                inverted_cdf: the smallest accepted sample whose empirical CDF reaches q; out[k * n_cols + col] is that order
 *                statistic of column col itself, bit for bit (a zero comes back as +0).  TAMCMC_E_INVALID: no accepted sample,
 *                max_samples = 0, Nq out of range, a q that is NaN or outside [0, 1].
 *   reset        forgets every sample (and puts the kernel time back to zero).   destroy   NULL is fine.
 *   kernel_time  summed milliseconds and launch count of the derive and fold kernels of the pushes since create or reset.
 * Work goes on the context's stream; every entry point but _destroy is refused with TAMCMC_E_INVALID while the context has a
 * batch in flight or armed (_destroy: armed), and NULL arguments and an Nparams mismatch before a device is touched. */
#define TAMCMC_MODETABLE_INCLINATION 0
#define TAMCMC_MODETABLE_ETA         1
#define TAMCMC_MODETABLE_A3          2
#define TAMCMC_MODETABLE_ASYMMETRY   3
#define TAMCMC_MODETABLE_FREQ        4
#define TAMCMC_MODETABLE_WIDTH       5
#define TAMCMC_MODETABLE_HEIGHT      6
#define TAMCMC_MODETABLE_AMPLITUDE   7
#define TAMCMC_MODETABLE_SPLITTING   8
#define TAMCMC_MODETABLE_WINDOW_LO   9
#define TAMCMC_MODETABLE_WINDOW_HI  10
#define TAMCMC_MODETABLE_NU_M       11
#define TAMCMC_MODETABLE_H_M        12
typedef struct tamcmc_modetable tamcmc_modetable;
typedef struct {
    int32_t kind, mult, order, l, m, param_index;
} tamcmc_modetable_col;
typedef struct {
    int64_t n_used, n_rejected, n_cols, n_mult;
} tamcmc_modetable_totals;
int tamcmc_modetable_create(tamcmc_modetable **out, tamcmc_ctx *ctx, int64_t max_samples);
int tamcmc_modetable_columns(tamcmc_modetable *mt, int32_t *n_cols, int32_t *n_mult);
int tamcmc_modetable_column(tamcmc_modetable *mt, int32_t col, tamcmc_modetable_col *out);
int tamcmc_modetable_derive(tamcmc_modetable *mt, int32_t Nsamples, int32_t Nparams, const double *params, double *rows,
                            int32_t *status);
int tamcmc_modetable_push(tamcmc_modetable *mt, int32_t Nsamples, int32_t Nparams, const double *params, const int32_t *skip,
                          int32_t *status);
int tamcmc_modetable_result(tamcmc_modetable *mt, tamcmc_modetable_totals *t, double *mean, double *sd, double *min, double *max);
int tamcmc_modetable_quantiles(tamcmc_modetable *mt, int32_t Nq, const double *q, int64_t *ranks, double *out);
int tamcmc_modetable_reset(tamcmc_modetable *mt);
int tamcmc_modetable_destroy(tamcmc_modetable *mt);
int tamcmc_modetable_kernel_time(tamcmc_modetable *mt, double *total_ms, int64_t *launches);

/* ---- Mode table diagnostics: ESS, MCSE, split R-hat and correlations of its columns ---------------------------------
 * Each call works on the accepted rows a mode table created with max_samples > 0 holds on the device; the caller makes no
 * second pass over the chain, and nothing of the table's state is written (result and quantiles return the same bits
 * before and after).  n = n_used; v_t = column c of the t-th accepted row in push order, t = 0 ... n - 1 (rejected and
 * skipped samples are not in the table and do not advance t).
 *   ESS, MCSE, R-hat of column c: steps 1-6 of "EFFECTIVE SAMPLE SIZE" above, applied to a column instead of a bin.
 *     1  d_t = v_t - mean_c, mean_c the double tamcmc_modetable_result returns; one subtraction, never contracted.
 *     2  L = the largest odd number <= min(max_lag | 1, n - 1); max_lag = 0 ... TAMCMC_MODEDIAG_MAX_LAG, 0 meaning 255.
 *     3  A_k = sum_{t=k}^{n-1} d_t d_{t-k}, k = 0 ... L: one accumulator per (column, k), started at +0.0 and advanced in
 *        ascending t by A = fma(d_t, d_{t-k}, A).  No (column, lag) sum is split over threads; no atomics.
 *     4  Geyer's initial monotone sequence as stated there (rho_k = A_k / A_0, P_m = rho_2m + rho_2m+1, ...), with
 *        tau_floor = 1 / log10(n) formed on the host: tau, ess = n / tau, cut (cut = L + 1: truncated).  A_0 zero or not finite:
 *        tau = ess = NaN, cut = 0.  A constant column (splitting at l = 0, inclination where the model has none, a window
 *        edge that never moves) centres to exact zeros -- Welford's mean of equal values is that value -- so A_0 = 0, and
 *        n_constant counts it.
 *     5  split R-hat: h = floor(n / 2), the halves [0, h) and [n - h, n), each by the Welford recurrence over d_t in t order
 *        (the centred values of step 1: R-hat does not change with the shift, and the recurrence's mean update then rounds
 *        at the size of the column's spread instead of its value), then
 *        W = (s1^2 + s2^2) / 2, Bn = (m1 - mb)^2 + (m2 - mb)^2, rhat = sqrt(((h - 1) / h W + Bn) / W); W = 0: NaN.
 *     6  mcse = sd / sqrt(ess), sd the double tamcmc_modetable_result returns; NaN where ess is NaN.
 *     7  totals, in column order (the first column wins a tie, a NaN is skipped): n_used, lag = L, min_ess with col_min_ess
 *        (NaN and -1 if every value is a NaN), max_rhat with col_max_rhat likewise, n_truncated (cut = L + 1), n_constant
 *        (A_0 = 0), n_rhat_high (rhat > 1.01).
 *   Covariance of columns i, j: S_ij = sum_t d_{i,t} d_{j,t} from +0.0 in ascending t by S = fma(d_{i,t}, d_{j,t}, S), d as in
 *     step 1; cov_ij = S_ij / (double)(n - 1).  cov is symmetric bit for bit, and S_ii is A_0 of the same column bit for bit.
 *   Correlation, on the host without contraction: r_ij = cov_ij / (sqrt(cov_ii) sqrt(cov_jj)) clamped to [-1, 1]; r_ii = 1.0
 *     exactly where cov_ii > 0 and finite; r_ij = NaN where either variance is 0 or not finite.
 *   ess          five arrays of n_cols entries and the totals, any may be NULL.  The lag products and the results stay on the
 *                device: 8 (L + 4) n_cols + 4 n_cols bytes, allocated at the first call, reallocated only when L grows, freed
 *                by tamcmc_modetable_destroy; TAMCMC_E_NOMEM leaves the object as it was.
 *   acov         the (L + 1) x n_cols lag products of the last _ess call, A_k of column c at acov[k * n_cols + c]; refused when
 *                there was no _ess call since the last push or reset.
 *   cov / corr   n_sel x n_sel doubles of the columns cols[0 ... n_sel - 1], in that order (cols NULL: the first n_sel
 *                columns); 8 n_sel^2 + 4 n_sel bytes on the device, allocated at the first call, reallocated only when n_sel
 *                grows.
 *   kernel_time  summed milliseconds and launch count of the lag, finish and covariance kernels since create or reset
 *                (tamcmc_modetable_reset puts it back to zero).
 * All calls are synchronous, on the context's stream.  Refused with TAMCMC_E_INVALID, before a device is touched: a NULL
 * handle, a context with a batch in flight or armed, max_samples = 0, n < 4 (_ess, _acov) or n < 2 (_cov, _corr), max_lag
 * outside 0 ... 1023, n_sel outside 1 ... min(n_cols, TAMCMC_MODEDIAG_MAX_COLS), a column index out of range or repeated, a
 * NULL acov, cov or corr. */
#define TAMCMC_MODEDIAG_MAX_LAG 1023
#define TAMCMC_MODEDIAG_MAX_COLS 1024
typedef struct {
    int64_t n_used, lag;
    double  min_ess, max_rhat;
    int64_t col_min_ess, col_max_rhat, n_truncated, n_constant, n_rhat_high;
} tamcmc_modediag_totals;
int tamcmc_modediag_ess(tamcmc_modetable *mt, int32_t max_lag, tamcmc_modediag_totals *totals,
                        double *ess, double *tau, double *mcse, double *rhat, int32_t *cut);
int tamcmc_modediag_acov(tamcmc_modetable *mt, double *acov);
int tamcmc_modediag_cov(tamcmc_modetable *mt, int32_t n_sel, const int32_t *cols, double *cov);
int tamcmc_modediag_corr(tamcmc_modetable *mt, int32_t n_sel, const int32_t *cols, double *corr);
int tamcmc_modediag_kernel_time(tamcmc_modetable *mt, double *total_ms, int64_t *launches);

/* ---- Mode table diagnostics on ranks: bulk and tail ESS, rank-normalised and folded split R-hat ------------------------
 * The diagnostics of Vehtari, Gelman, Simpson, Carpenter and Buerkner, "Rank-normalization, folding, and localization"
 * (2021), of the columns of a mode table created with max_samples > 0: what the block above says of the raw values, said of
 * their ranks, which heavy tails, skewness and ties (window edges are integers) cannot mislead.  ESS here is this project's
 * single-chain Geyer estimate (steps 2-4 of the block above) applied to the transformed series, NOT Stan's multi-chain
 * formula; R-hat is the split R-hat of step 5 of the transformed series.  Nothing of the table's state and nothing of
 * tamcmc_modediag_*'s buffers is written.  n = n_used >= 4; v_t = column c of the t-th accepted row in push order; order
 * is that of the quantiles' keys (-0 and +0 are one value; the table holds no NaN).
 *     1  rank2_t = #{s : v_s < v_t} + #{s : v_s <= v_t} + 1: twice the average rank, an integer in [2, 2n]; sum_t rank2_t =
 *        n (n + 1) exactly.
 *     2  z_t: a = 4 rank2_t - 3, D = 8 n + 2, b = D - a (p = a / D is Blom's (r - 3/8) / (n + 1/4)).  a < b: z = -g(a / D);
 *        a > b: z = +g(b / D); a = b: z = +0.0, where g(q) = -Phi^-1(q) for 0 < q < 1/2 from the one division
 *        (double)a / (double)D.  The smaller tail is always the one inverted, so z(rank2) = -z(2 (n + 1) - rank2) bit for
 *        bit.  g is a closed-form start and two Halley steps on erfc; host and device use their own libm, and either meets
 *        |z - z_exact| <= 10 2^-50 q / phi(z) + 4 2^-52 |z|.
 *     3  fold: med = 0.5 s_[(n-1)/2] + 0.5 s_[n/2] of the sorted column (a zero as +0), f_t = |v_t - med| (one subtraction,
 *        never contracted); rank2 and z of f by steps 1-2 give zf_t.
 *     4  tail indicators: i05_t = (v_t <= Q05), i95_t = (v_t <= Q95) as 0.0 / 1.0, Q the order statistic
 *        tamcmc_modetable_quantiles returns for 0.05 and 0.95, bit for bit.
 *     5  each of the four series (Z, ZFOLD, I05, I95) gets its mean by the Welford recurrence in t order, then goes through
 *        steps 1-5 of the block above unchanged, by the same kernels: centred values, lag products A_k, Geyer's finish,
 *        split R-hat of the centred halves.
 *     6  per column, out[k][n_sel], k = 0 ... TAMCMC_MODERANK_NOUT - 1: ess_bulk = ess(Z); ess_tail = the smaller of ess(I05) and
 *        ess(I95), a NaN skipped, NaN if both are; rhat = the larger of rhat(Z) and rhat(ZFOLD), likewise; tau_bulk = tau(Z);
 *        rhat_bulk = rhat(Z); rhat_fold = rhat(ZFOLD); ess_q05 = ess(I05); ess_q95 = ess(I95).  cut[s][n_sel]: cut of series s.
 *        A constant column has every rank2 = n + 1, so z = +0 throughout and A_0 = 0: NaN, cut 0, counted in n_constant.
 *     7  totals, in the order of the selection (the first wins a tie, a NaN is skipped): n_used, lag = L; min_ess_bulk,
 *        min_ess_tail, max_rhat, each with the table's column it belongs to (NaN and -1 if every value is a NaN);
 *        n_truncated (cut of Z = L + 1), n_constant (A_0 of Z = 0), n_rhat_high (rhat > 1.01).
 *   diag         cols[0 ... n_sel - 1] are the columns, in that order (cols NULL: the first n_sel columns); totals, out and
 *                cut may be NULL.  The columns are processed in chunks sized so that a chunk fits scratch_bytes of device
 *                memory (0: 256 MiB): per column 16 P + 32 (n + L + 5) + 44 bytes, P the smallest power of two >= n (two
 *                buffers of sorted keys, four series, their means, lag products and finish arrays).  At least one column
 *                goes in a chunk; when even that cannot be allocated, TAMCMC_E_NOMEM, and the object is as it was.  No
 *                result bit depends on the chunking or on the selection.  The scratch is kept for the next call and freed by
 *                tamcmc_modetable_destroy.
 *   acov         the (L + 1) x n_sel lag products of series `series` (0 ... TAMCMC_MODERANK_NSERIES - 1) of the last _diag call,
 *                A_k of selected column j at acov[k * n_sel + j]; refused when there was no _diag call since the last push or
 *                reset.
 *   series       one column recomputed by the same kernels, for tests and plots: rank2 and rank2_fold (n each), the four
 *                series ([TAMCMC_MODERANK_NSERIES][n]), their means, and {med, Q05, Q95}; any may be NULL.
 *   kernel_time  summed milliseconds and launch count of the sort, transform, mean, lag and finish kernels of _diag and
 *                _series since create or reset.
 * All calls are synchronous, on the context's stream.  Refused with TAMCMC_E_INVALID, before a device is touched: a NULL
 * handle, a context with a batch in flight or armed, max_samples = 0, n < 4, max_lag outside 0 ... 1023, n_sel outside
 * 1 ... n_cols, a column index out of range or repeated, a negative scratch_bytes, a NULL acov, a series outside 0 ... 3. */
#define TAMCMC_MODERANK_NOUT 8     /* ess_bulk, ess_tail, rhat, tau_bulk, rhat_bulk, rhat_fold, ess_q05, ess_q95 */
#define TAMCMC_MODERANK_NSERIES 4  /* Z, ZFOLD, I05, I95 */
typedef struct {
    int64_t n_used, lag;
    double  min_ess_bulk, min_ess_tail, max_rhat;
    int64_t col_min_ess_bulk, col_min_ess_tail, col_max_rhat, n_truncated, n_constant, n_rhat_high;
} tamcmc_moderank_totals;
int tamcmc_moderank_diag(tamcmc_modetable *mt, int32_t max_lag, int32_t n_sel, const int32_t *cols, int64_t scratch_bytes,
                         tamcmc_moderank_totals *totals, double *out, int32_t *cut);
int tamcmc_moderank_acov(tamcmc_modetable *mt, int32_t series, double *acov);
int tamcmc_moderank_series(tamcmc_modetable *mt, int32_t col, int64_t *rank2, int64_t *rank2_fold, double *series, double *mean,
                           double *med_q);
int tamcmc_moderank_kernel_time(tamcmc_modetable *mt, double *total_ms, int64_t *launches);

/* Replaces: the `for chain` loop of generate_model() calls (MALA.cpp:632-639, model_def.cpp:139-143).
 * Host pointers, row-major.  Synchronous: results are valid on return.
 *   params      Nchains x Nparams
 *   Tcoefs      Nchains temperatures (MALA.cpp:103)
 *   logL        Nchains, tempered: logL/T
 *   grad        NULL, or Nchains x Nvars
 *   model_rows  n_rows chain indices whose model spectrum is wanted (Model_def::model rows), or NULL
 *   model_out   n_rows x Nx, or NULL
 *   status      NULL or Nchains TAMCMC_CHAIN_* codes
 * Largest batch of one call -- here and in every other entry point that evaluates chains on one context (_device, _begin,
 * _arm, _reserve, and the blocks of tamcmc_summary_push): no launch may exceed 2^32 - 1 work-items, the rule of
 * tamcmc_group_eval, so with T tiles per chain (tamcmc_ctx_geometry)
 *     Nchains * T <= 16 777 215          (workgroups of 256 threads), and
 *     Nchains     <=  8 388 607          (per-chain workgroups of 512 threads) unless the grid is one tile and no gradient
 *                                        is asked for (one launch of 256 threads per chain).
 * A larger Nchains is refused with TAMCMC_E_INVALID before anything is allocated or enqueued; split the batch -- a chain's
 * result depends neither on the batch nor on its position in it.  Device memory is the limit met first on most grids:
 * a batch needs a few KB per chain and tile (more with a gradient).  Tested at 70 001 chains on every launch path and at
 * 131 073 on the one-tile path (tests/test_chain_counts_gpu.py, tests/test_summary_large_gpu.py). */
int tamcmc_eval_batch(tamcmc_ctx *ctx, int32_t Nchains, int32_t Nparams,
                      const double *params, const double *Tcoefs,
                      double *logL, double *grad,
                      int32_t n_rows, const int32_t *model_rows, double *model_out,
                      int32_t *status);

/* Same computation with DEVICE pointers (hipMalloc'ed on the ctx device), enqueued on the ctx stream
 * without synchronising: for a sampler that keeps chain state resident in HBM.
 * d_grad / d_status may be NULL. */
int tamcmc_eval_batch_device(tamcmc_ctx *ctx, int32_t Nchains, int32_t Nparams,
                             const double *d_params, const double *d_Tcoefs,
                             double *d_logL, double *d_grad, int32_t *d_status);

/* tamcmc_eval_batch split in two for callers that have host work to overlap with the GPU (the sampler draws the next
 * iteration's random numbers meanwhile): _begin copies params / Tcoefs and enqueues the likelihood evaluation, _end
 * waits and delivers logL / status.  Likelihood only (no gradient, no model rows); one batch in flight per ctx.
 * Both host-pointer entry points return as soon as every result has arrived in the library's pinned staging buffer,
 * which can be a few microseconds before the launch itself retires on the ctx stream; everything else in this API
 * that touches the ctx is ordered after it on that stream (or synchronises it). */
int tamcmc_eval_batch_begin(tamcmc_ctx *ctx, int32_t Nchains, int32_t Nparams, const double *params, const double *Tcoefs);
int tamcmc_eval_batch_end(tamcmc_ctx *ctx, int32_t Nchains, double *logL, int32_t *status);

/* Armed batch -- for a host loop whose next parameters depend on the results of the batch in flight (a sampler):
 * _arm puts the launches of the NEXT likelihood-only batch into the stream behind a one-wave gate kernel, while the
 * current batch is still being evaluated (allowed between _begin / _fire and _end of a batch of the same size; the
 * buffers must already be sized: tamcmc_ctx_reserve or an earlier batch), so that the launch calls cost nothing on the
 * critical path; _fire copies the parameters into the pinned input buffer and opens the gate with one store -- it takes
 * the place of _begin, and _end collects the results as usual.  While a batch is armed every other entry point of the
 * context returns TAMCMC_E_INVALID except _fire, _end (of the batch in flight), _disarm and tamcmc_ctx_destroy.  _disarm
 * opens the gate of a batch that will not be fired (it runs on the previous parameters, is waited for, and nothing is
 * handed out).  The gate itself gives up after ~4 s, so that a wave never outlives a host that died before firing; a
 * host that was merely held up that long loses time, not a result: _fire notices that the gate has expired (the armed
 * launches ran on stale input), lets them drain and evaluates the batch the plain way. */
int tamcmc_eval_batch_arm(tamcmc_ctx *ctx, int32_t Nchains);
/* One chain of the batch in flight (_begin / _fire, not yet _end): TAMCMC_OK with its logL and status once they have
 * arrived, TAMCMC_PENDING before.  Results arrive chain by chain (each is finalized by the last of its tiles), so a host
 * loop can start on a chain's accept step while the others are still being evaluated.  Read-only: any number of threads
 * may poll (different or the same chains) while no other entry point of the context is called; _end is still due, and
 * is the call that reports a failed launch -- a poller must bound its patience and then go there. */
int tamcmc_eval_batch_poll(const tamcmc_ctx *ctx, int32_t chain, double *logL, int32_t *status);
int tamcmc_eval_batch_fire(tamcmc_ctx *ctx, int32_t Nchains, int32_t Nparams, const double *params, const double *Tcoefs);
int tamcmc_eval_batch_disarm(tamcmc_ctx *ctx);

/* Sizes the context's buffers for batches of up to Nchains chains ahead of _arm, which never reallocates under a batch in
 * flight (refused while a batch is in flight or armed). */
int tamcmc_ctx_reserve(tamcmc_ctx *ctx, int32_t Nchains);

/* Replaces: Model_def::call_model_explicit (model_def.cpp:199-208) as used by tools/getmodel.cpp:111.
 * One params row -> model spectrum (Nx doubles, host).  *status gets the TAMCMC_CHAIN_* code. */
int tamcmc_model_explicit(tamcmc_ctx *ctx, int32_t Nparams, const double *params,
                          double *model_out, int32_t *status);

/* Stream plumbing.  hip_stream is a hipStream_t created on the ctx device (NULL = the ctx's own stream). */
int tamcmc_ctx_set_stream(tamcmc_ctx *ctx, void *hip_stream);
int tamcmc_ctx_synchronize(tamcmc_ctx *ctx);

/* Kernel timing with HIP events recorded on the ctx stream around the dominant kernel of every eval call while
 * enabled (enable = 1), or of every n-th call (enable = n > 1: an event pair costs ~3 us of stream time, which a
 * throughput measurement over the same calls would otherwise carry in full).  tamcmc_ctx_kernel_time synchronises the stream, then returns the summed
 * duration and the number of launches since profiling was enabled. */
int tamcmc_ctx_profile(tamcmc_ctx *ctx, int enable);
int tamcmc_ctx_kernel_time(tamcmc_ctx *ctx, double *total_ms, int64_t *launches);

/* Shader-clock probe: _begin launches ONE wave on a stream of its own that watches the core-cycle counter against the
 * constant 100 MHz counter for `milliseconds`; _end waits for it and returns the mean core clock over that window.
 * Evaluations enqueued between the two calls run beside it, so this is the clock under that load (used by bench.py to
 * turn instruction counts into a fraction of the fp64 issue rate with a clock measured in the same run). */
int tamcmc_ctx_clock_probe_begin(tamcmc_ctx *ctx, double milliseconds);
int tamcmc_ctx_clock_probe_end(tamcmc_ctx *ctx, double *core_GHz, double *seconds);

/* Launch geometry actually used (for DESIGN.md / bench bookkeeping): bins_per_tile = the largest tile of the
 * likelihood-only launch (16 units of 512 bins; 8 when TAMCMC_EQUAL_COST balances the tiles, and always for the gradient
 * launch), tiles = tiles per chain of the most recent likelihood-only call. */
int tamcmc_ctx_geometry(tamcmc_ctx *ctx, int32_t *bins_per_tile, int32_t *tiles, int32_t *threads_per_block,
                        int32_t *n_multiplets);
/* The same for the gradient launch: tiles = tiles per chain of a gradient batch (fixed at create time: the tail rule on
 * long grids, or TAMCMC_TILES_GRAD), bins_per_tile = its largest tile (8 units of 512 bins).  Either pointer may be NULL. */
int tamcmc_ctx_geometry_grad(tamcmc_ctx *ctx, int32_t *tiles, int32_t *bins_per_tile);

/* TAMCMC_E_INVALID (and nothing happens) while the context is a member of a fit group or has a summary object. */
int tamcmc_ctx_destroy(tamcmc_ctx *ctx);

int tamcmc_device_count(void);
const char *tamcmc_strerror(int code);
const char *tamcmc_last_hip_error(void);
const char *tamcmc_version(void);

#ifdef __cplusplus
}
#endif

/* The seismic indices of the mode table (large separation, epsilon, nu_max, small separations, frequency ratios as further
 * columns of the table): the kind codes after TAMCMC_MODETABLE_H_M and the entry points, in a header of their own. */
#include "tamcmc_accel_seismic.h"
/* Marginal histograms, shortest (HPD) intervals and pair densities of the mode table's columns: the tamcmc_modepdf_* entry
 * points, in a header of their own. */
#include "tamcmc_accel_pdf.h"
/* The comparison of several fits of one spectrum from their pointwise LOO values (elpd differences, Bayesian bootstrap,
 * pseudo-BMA and stacking weights): the tamcmc_compare_* entry points, in a header of their own. */
#include "tamcmc_accel_compare.h"
#endif /* TAMCMC_ACCEL_H */
