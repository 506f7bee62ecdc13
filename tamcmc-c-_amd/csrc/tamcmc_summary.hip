// tamcmc_summary.hip -- stage 2 of a posterior summary (tamcmc_summary.h): fold the model rows of one block of samples
// into the per-bin running statistics.
//
// One thread owns one bin.  It loads the bin's running state, walks the block's rows ONE SAMPLE AT A TIME IN PUSH ORDER
// with the fixed update formulas below, and stores the state back.  Nothing is shared between threads: no LDS, no
// barrier, no atomics, no cross-lane reduction -- so a bin's results are bit for bit independent of the block size and
// of how the samples were split over pushes (the tests pin this).  The formulas are compiled without FMA contraction:
// they are part of that contract, not a matter of the optimiser's mood.
//
//   model value v = M_is, pointwise log-likelihood l = l_is: tms_like (tamcmc_summary_walk.h)
//   Welford, for v and for l:      d = v - mean;  mean += d / n;  M2 += d (v - mean)
//   envelope:                      min, max
//   running-maximum log-sum-exp:   first sample a = l, r = 1;  then  l > a:  r = r exp(a - l) + 1, a = l;  else r += exp(l - a)
//
// The walk over the block's rows is tms_walk (tamcmc_summary_walk.h): rejected samples (status != TAMCMC_CHAIN_OK) are
// skipped and counted from the pair {accepted, rejected} the previous launch left, and the host never looks at the
// status words; thread 0 of the launch stores the new pair into the OTHER pair of words, which the next launch reads.
//
// The kernel is a stream over B x Nx doubles read once: TM_SUM_UNROLL row loads are requested per thread before the
// first of them is folded (the rows of a block sit in one buffer of up to 64 MiB by default).
#include <hip/hip_runtime.h>
#include <cmath>

#include "tamcmc_summary.h"

#pragma clang fp contract(off)

struct TmSumState {
    double mean_M, M2_M, min_M, max_M, mean_l, M2_l, a, r;
};

__device__ __forceinline__ void tm_summary_fold_one(TmSumState &s, const long long n, const double v, const double l)
{
    const double dn = (double)n;
    double d = v - s.mean_M;
    s.mean_M += d / dn;
    s.M2_M += d * (v - s.mean_M);
    d = l - s.mean_l;
    s.mean_l += d / dn;
    s.M2_l += d * (l - s.mean_l);
    if (n == 1) {
        s.min_M = v; s.max_M = v;
        s.a = l; s.r = 1.0;
    } else {
        s.min_M = v < s.min_M ? v : s.min_M;
        s.max_M = v > s.max_M ? v : s.max_M;
        if (l > s.a) { s.r = s.r * exp(s.a - l) + 1.0; s.a = l; }
        else s.r += exp(l - s.a);
    }
}

__global__ __launch_bounds__(TM_SUM_THREADS) void tamcmc_summary_fold_kernel(const TmSummaryArgs a)
{
    const int bin = (int)(blockIdx.x * TM_SUM_THREADS + threadIdx.x);
    if (bin >= a.Nx) return;
    const size_t nx = (size_t)a.Nx;
    double *__restrict__ st = a.state + bin;
    TmSumState s;
    s.mean_M = st[TM_SUM_MEAN_M * nx]; s.M2_M = st[TM_SUM_M2_M * nx];
    s.min_M = st[TM_SUM_MIN_M * nx]; s.max_M = st[TM_SUM_MAX_M * nx];
    s.mean_l = st[TM_SUM_MEAN_L * nx]; s.M2_l = st[TM_SUM_M2_L * nx];
    s.a = st[TM_SUM_LSE_A * nx]; s.r = st[TM_SUM_LSE_R * nx];
    const TmsBinLike lk(a, bin);
    const TmsCount cnt = tms_walk<TM_SUM_UNROLL>(a.rows + bin, a.status, 0, a.B, nx, TmsCount{a.cnt_in[0], a.cnt_in[1]},
                                                 [&](const double v, const long long n) { tm_summary_fold_one(s, n, v, lk.l(v)); });

    st[TM_SUM_MEAN_M * nx] = s.mean_M; st[TM_SUM_M2_M * nx] = s.M2_M;
    st[TM_SUM_MIN_M * nx] = s.min_M; st[TM_SUM_MAX_M * nx] = s.max_M;
    st[TM_SUM_MEAN_L * nx] = s.mean_l; st[TM_SUM_M2_L * nx] = s.M2_l;
    st[TM_SUM_LSE_A * nx] = s.a; st[TM_SUM_LSE_R * nx] = s.r;
    if (bin == 0) { a.cnt_out[0] = cnt.n; a.cnt_out[1] = cnt.rej; }
}

int tm_launch_summary_fold(const TmSummaryArgs &a, void *stream)
{
    hipLaunchKernelGGL(tamcmc_summary_fold_kernel, dim3(tms_blocks(a.Nx, TM_SUM_THREADS)), dim3(TM_SUM_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
