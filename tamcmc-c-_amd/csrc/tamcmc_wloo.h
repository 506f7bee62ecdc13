// tamcmc_wloo.h -- leave-one-window-out PSIS-LOO of a stored chain and its PIT sub-mode (tamcmc_summary_wloo_* in
// include/tamcmc_accel.h): the machinery of tamcmc_loo.h and tamcmc_loopit.h with "bin" read as "window", over the disjoint
// windows of tamcmc_window.h.  Bins are conditionally independent given the parameters, so leaving a window out is PSIS fed
// with x_ws = -sum_{i in w} l_is in place of x_is = -l_is.  Leaving one bin of a 20-bin mode out tests almost nothing -- its 19
// neighbours pin the mode -- and the windowed predictive check uses the window's data twice; this is the statistic at the
// granularity of a feature.
//
// The arithmetic below is plain C++17: the kernels (tamcmc_wloo.hip) and the stand-alone check
// (tests/cpp/wloo_core_check.cpp, built with g++) call these same functions.  tamcmc_wloo.hip includes this header under
// `#pragma clang fp contract(off)`, so on the device none of it is contracted into FMAs.
//
//   windows   tmw_begin / tmw_end / tmw_partition of tamcmc_window.h: W bins each, the first one `first` bins.
//   sum       S_ws = l_is (tms_like, the fold kernel's) added over the window's bins in ascending bin order starting from the
//             first term, plain double: tmw_sum's order.  x_ws = -S_ws.  A window of one bin has S = l bit for bit, so W = 1
//             is the per-bin mode.                                                                          tmw_sum
//   LOO       tml_top_push per (window, accepted sample) into a heap [M + 1][n_windows] and a body [3][n_windows]; the
//             finalize kernel of tamcmc_loo.hip with n_windows for Nx.
//   PIT       the prepare kernel of tamcmc_loopit.hip with n_windows for Nx; per (sample, window) logP, logQ = tmw_chi /
//             tmw_gauss on the window sum of tms_resid, as the windowed check forms them; then tlp_find for a tail sample
//             and tlp_add, one sample at a time in push order.
//   scratch   [Bcap][n_windows] doubles per plane: S in LOO mode; in the sub-mode two more planes, the residual sum -- replaced
//             in place by logP -- and logQ.
// Device memory of the mode, in bytes, with nw = n_windows, M = tml_tail_M(n_used), B = block_chains:
//   wloo_begin       8 (M + 1) nw  +  52 nw + 32  +  8 B nw            heap | state | scratch                twl_begin_bytes
//   wloo_pit_begin   8 M nw  +  116 nw + 36  +  16 B nw                log weights | state | scratch         twl_pit_bytes
#pragma once
#include "tamcmc_loopit.h"
#include "tamcmc_summary_walk.h"
#include "tamcmc_window.h"

#define TM_WLOO_THREADS 64        // tail and PIT kernels: one window per thread
#define TM_WLOO_UNROLL 8          // scratch loads in flight per thread of the tail kernel
#define TM_WLOO_PIT_UNROLL 4      // samples whose three scratch words the PIT kernel requests before it uses the first

inline size_t twl_state_bytes(const size_t nw) { return 6 * nw * sizeof(double) + 4 * sizeof(long long) + nw * sizeof(int32_t); }
inline size_t twl_heap_bytes(const size_t nw, const size_t M) { return (M + 1) * nw * sizeof(double); }
inline size_t twl_scratch_bytes(const size_t nw, const size_t B) { return B * nw * sizeof(double); }
inline size_t twl_begin_bytes(const size_t nw, const size_t M, const size_t B)
{
    return twl_heap_bytes(nw, M) + twl_state_bytes(nw) + twl_scratch_bytes(nw, B);
}
inline size_t twl_pit_state_bytes(const size_t nw)
{
    return ((size_t)TM_LOOPIT_NSTATE + 2) * nw * sizeof(double) + 4 * sizeof(long long) + (nw + 1) * sizeof(int32_t);
}
inline size_t twl_lw_bytes(const size_t nw, const size_t M) { return M * nw * sizeof(double); }
inline size_t twl_pit_bytes(const size_t nw, const size_t M, const size_t B)
{
    return twl_lw_bytes(nw, M) + twl_pit_state_bytes(nw) + 2 * twl_scratch_bytes(nw, B);
}

// ---- launch arguments (tamcmc_wloo.hip) ----
struct TmWlooArgs {
    const double *rows;           // [B][Nx] model rows of the block (stage 1)
    const int32_t *status;        // [B]
    const double *y, *isig2;      // as TmSummaryArgs
    double *sum;                  // [Bcap][n_windows]: S of every (sample, window) of the block
    double *logP, *logQ;          // [Bcap][n_windows] each, sub-mode only: logP holds the residual sum until the tails kernel ran
    double *heap;                 // [cap][n_windows]
    double *body;                 // [3][n_windows]: a | r | c
    const double *lw;             // [cap - 1][n_windows]: the log weight of sorted slot j + 1 (sub-mode)
    const double *xmax, *c;       // [n_windows] each, written by the prepare kernel (sub-mode)
    const int32_t *first_slot;    // [n_windows]: the first tail slot, cap where the tail is empty (sub-mode)
    double *state;                // [TM_LOOPIT_NSTATE][n_windows] (sub-mode)
    const long long *cnt_in;      // {accepted, rejected} of the pass before the block / after it (as TmSummaryArgs)
    long long *cnt_out;
    int32_t *flag;                // set to 1 when a tail sample is not among the stored values (sub-mode)
    int32_t Nx, B;
    int32_t Bcap;                 // block_chains: the scratch's stride
    int32_t n_windows;
    int32_t W, first;
    int32_t likelihood_case, p;   // p: chi(2,2p) of the sub-mode's tails
    int32_t cap, trips;           // cap = M + 1; tlp_trips(cap - 1)
    double like_p;
    TmWinShape shape[3];          // sub-mode
};

// sums kernel and tail kernel of a block of the LOO pass, in that order on `stream`; returns a hipError_t
int tm_launch_wloo_tail(const TmWlooArgs &a, void *stream);
// sums kernel (both sums), tails kernel and PIT kernel of a block of the sub-mode's pass
int tm_launch_wloo_pit(const TmWlooArgs &a, void *stream);
