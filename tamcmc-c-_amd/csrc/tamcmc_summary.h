// tamcmc_summary.h -- posterior summaries of a stored chain (tamcmc_summary_* in include/tamcmc_accel.h): per-bin running
// statistics, over the samples pushed so far, of the model value M and of the pointwise log-likelihood l.
//
// A block of B samples takes two stages on the context's stream, with no host round trip in between: the context's own
// launches with a row map that covers every chain (the B model rows land in a B x Nx buffer of the summary object), then
// tamcmc_summary_fold_kernel (tamcmc_summary.hip), which folds those rows into the running state.
//
// Running state, structure of arrays, TM_SUM_NSTATE blocks of Nx doubles.  The ninth quantity of the recurrences, the
// number of accepted samples, is the same for every bin and is kept once (TmSummaryArgs::cnt_in / cnt_out).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "tamcmc_summary_walk.h"

enum {
    TM_SUM_MEAN_M = 0, TM_SUM_M2_M, TM_SUM_MIN_M, TM_SUM_MAX_M,   // Welford mean / sum of squared deviations, envelope
    TM_SUM_MEAN_L, TM_SUM_M2_L,                                   // the same pair for l
    TM_SUM_LSE_A, TM_SUM_LSE_R,                                   // sum_s exp l_s = r exp(a), a = the running maximum of l
    TM_SUM_NSTATE
};
#define TM_SUM_THREADS 256        // one thread owns one bin: a wave reads 512 consecutive bytes of a row
#define TM_SUM_UNROLL 8           // row loads in flight per thread

struct TmSummaryArgs {
    const double *rows;           // [B][Nx] model rows of the block (stage 1)
    const int32_t *status;        // [B] TAMCMC_CHAIN_* of the block's samples, device memory: a sample that is not OK is skipped
    const double *y, *isig2;      // the context's spectrum; 1 / sigma^2 (chi_square only, else NULL)
    double *state;                // [TM_SUM_NSTATE][Nx]
    // {accepted, rejected} samples before this block / after it.  Two different pairs (the object alternates them from
    // launch to launch): no workgroup reads a word that another workgroup of the same launch writes.
    const long long *cnt_in;
    long long *cnt_out;
    int32_t Nx, B;
    int32_t likelihood_case, pad;
    double like_p;                // already truncated (TmLayout::like_p)
};

// host: lppd_i = log((1/n) sum_s exp l_is) from the bin's running-maximum log-sum-exp (a, r) and n accepted samples
inline double tm_lppd(const double a, const double r, const double n) { return a + log(r / n); }

int tm_launch_summary_fold(const TmSummaryArgs &a, void *stream);      // tamcmc_summary.hip; returns a hipError_t
