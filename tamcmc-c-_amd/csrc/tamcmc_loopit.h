// tamcmc_loopit.h -- leave-one-out PIT of a stored chain (tamcmc_summary_loo_pit_* in include/tamcmc_accel.h): the
// predictive tail probabilities of tamcmc_predictive.h averaged with the Pareto-smoothed importance weights of PSIS-LOO
// (tamcmc_loo.h), per bin, and Kish's effective sample size of those weights.  A third pass over the same samples, in LOO
// mode, after a complete LOO pass.
//
// The arithmetic below is plain C++17: the kernels (tamcmc_loopit.hip) and the stand-alone check
// (tests/cpp/loopit_core_check.cpp, built with g++) call these same functions.  tamcmc_loopit.hip includes this header
// under `#pragma clang fp contract(off)`, so on the device none of it is contracted into FMAs.
//
//   prepare  per bin the M candidates above the root of the top set, sorted ascending (tml_load_sorted), go back into heap
//            slots 1 ... M -- a sorted array is a valid min-heap, so tamcmc_summary_loo_result keeps its bits -- and
//            tml_finalize leaves the tail's log weights zt_(j) behind.  The table lw[M][Nx] gets, per sorted slot, the log
//            weight a sample with that x carries: z for a body slot, zt_(j) for a tail slot that is alone with its value, and
//            for a run a..b of tail slots whose x are equal bit for bit the logarithm of the mean weight of the ranks the
//            run occupies, log((sum_{j=a..b} exp(zt_(j))) / (b - a + 1)) summed in ascending j               tlp_tie_lw
//   search   a sample of the tail (z > c) finds its slot by a lower-bound search down the bin's sorted column: a fixed
//            number of steps tlp_trips(M) = ceil(log2(M + 1)), no branch, every index clamped into [1, M], so a pass of
//            other rows cannot read outside the column; it ends on the first slot whose value is not below x, and a
//            value there that is not x bit for bit raises the pass's not-found flag                           tlp_find
//   sums     four running-maximum log-sum-exps in push order by tmp_lse_step (Kahan, -inf terms skipped):
//            lW = lse(lw), lA = lse(lw + logP), lB = lse(lw + logQ), lW2 = lse(2 lw)                          tlp_add
//   results  loo_log_cdf = lA - lW, loo_log_sf = lB - lW, is_ess = exp(2 lW - lW2), log_wsum = lW, on the host    tlp_lse
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "tamcmc_loo.h"
#include "tamcmc_predictive.h"

#ifndef TM_LOOPIT_UNROLL
#define TM_LOOPIT_UNROLL TM_LOO_UNROLL      // row loads in flight per thread
#endif
#define TM_LOOPIT_THREADS 64      // PIT kernel: one bin per thread; prepare kernel: one wave per bin (TM_LOO_THREADS)

enum {
    TM_LOOPIT_W_A = 0, TM_LOOPIT_W_R, TM_LOOPIT_W_C,        // sum_s w_s = (r - c) exp(a)
    TM_LOOPIT_A_A, TM_LOOPIT_A_R, TM_LOOPIT_A_C,            // sum_s w_s P_is
    TM_LOOPIT_B_A, TM_LOOPIT_B_R, TM_LOOPIT_B_C,            // sum_s w_s Q_is
    TM_LOOPIT_W2_A, TM_LOOPIT_W2_R, TM_LOOPIT_W2_C,         // sum_s w_s^2
    TM_LOOPIT_NSTATE
};

TML_FN bool tlp_same_bits(const double a, const double b)
{
    uint64_t u, v;
    memcpy(&u, &a, sizeof u);
    memcpy(&v, &b, sizeof v);
    return u == v;
}

// sv[0 .. L): the tail's x ascending; zt[0 .. L): its log weights; the log weight of every sample whose x is sv[j]
TML_FN double tlp_tie_lw(const double *sv, const double *zt, const int L, const int j)
{
    int a = j, b = j;
    while (a > 0 && tlp_same_bits(sv[a - 1], sv[j])) a--;
    while (b + 1 < L && tlp_same_bits(sv[b + 1], sv[j])) b++;
    if (a == b) return zt[j];
    double sum = 0.0;
    for (int i = a; i <= b; i++) sum += exp(zt[i]);
    return log(sum / (double)(b - a + 1));
}

// steps of the search over a column of M >= 1 slots: the first T with 2^T >= M + 1
TML_FN int tlp_trips(const int M)
{
    int T = 0;
    while (((long long)1 << T) < (long long)M + 1) T++;
    return T;
}

// The search keeps pos = the number of slots known to hold a value below x, 0 at the start, and tries pos + 2^t for t =
// T - 1 ... 0.  tlp_probe: the slot to read for this step, in [1, M];  tlp_advance: pos after it, v the value read;
// tlp_slot: once all steps are done, the slot that holds x if any slot does, in [1, M].
TML_FN int tlp_probe(const int pos, const int step, const int M) { const int i = pos + step; return i < M ? i : M; }
TML_FN int tlp_advance(const int pos, const int step, const int M, const double v, const double x)
{
    const int i = pos + step;
    return ((i <= M) & (v < x)) ? i : pos;
}
TML_FN int tlp_slot(const int pos, const int M) { return pos < M ? pos + 1 : M; }

// one sample's search on its own: col[slot * stride], slot 1 ... M.  *found: the slot's value is x bit for bit
TML_FN int tlp_find(const double *col, const size_t stride, const int M, const int trips, const double x, bool *found)
{
    int pos = 0;
    for (int t = trips - 1; t >= 0; t--) {
        const int step = 1 << t;
        pos = tlp_advance(pos, step, M, col[(size_t)tlp_probe(pos, step, M) * stride], x);
    }
    const int slot = tlp_slot(pos, M);
    *found = tlp_same_bits(col[(size_t)slot * stride], x);
    return slot;
}

// The four sums of one bin, (a, r, c) each, and one accepted sample added to them.
struct TlpSums {
    double wa, wr, wc, aa, ar, ac, ba, br, bc, qa, qr, qc;
};
TML_FN void tlp_add(TlpSums *s, const double lw, const double logP, const double logQ)
{
    tmp_lse_step(&s->wa, &s->wr, &s->wc, lw);
    tmp_lse_step(&s->aa, &s->ar, &s->ac, lw + logP);
    tmp_lse_step(&s->ba, &s->br, &s->bc, lw + logQ);
    tmp_lse_step(&s->qa, &s->qr, &s->qc, 2.0 * lw);
}

// host: log of a sum (r - c) exp(a); a sum without a finite term is -inf
inline double tlp_lse(const double a, const double r, const double c) { return r == 0.0 ? -(double)INFINITY : a + log(r - c); }

// ---- launch arguments (tamcmc_loopit.hip) ----
struct TmLooPitArgs {
    const double *rows;           // [B][Nx] model rows of the block (stage 1)
    const int32_t *status;        // [B]
    const double *y, *isig2;      // as TmSummaryArgs
    double *heap;                 // [cap][Nx]: the LOO pass's top sets; prepare sorts slots 1 ... cap - 1 in place
    const double *body;           // [3][Nx] of the LOO pass (prepare)
    double *lw;                   // [cap - 1][Nx]: the log weight of sorted slot j + 1
    double *xmax, *c;             // [Nx] each, written by prepare
    int32_t *first;               // [Nx]: the first tail slot, cap where the tail is empty
    double *state;                // [TM_LOOPIT_NSTATE][Nx]
    const long long *cnt_in;      // {accepted, rejected} of the PIT pass before the block / after it (as TmSummaryArgs)
    long long *cnt_out;
    int32_t *flag;                // set to 1 when a tail sample is not among the stored values
    long long n;                  // the LOO pass's accepted samples
    int32_t Nx, B;
    int32_t likelihood_case, cap; // cap = M + 1
    int32_t p, nterms;            // as TmPredArgs
    int32_t trips, pad;           // tlp_trips(cap - 1)
    double like_p, lf_pm1, lf_p;
};

int tm_launch_loopit_prepare(const TmLooPitArgs &a, void *stream);    // return a hipError_t
int tm_launch_loopit(const TmLooPitArgs &a, void *stream);
