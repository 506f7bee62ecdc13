// tamcmc_predictive.hip -- the posterior predictive check of a summary object (tamcmc_predictive.h): behind the fold
// kernel of every fold-mode block, on the same rows and the same stream, accumulate per bin the predictive CDF and
// survival function of the datum (two running-maximum log-sum-exps) and the mean residual.
//
// Shaped like the fold kernel (tamcmc_summary.hip).  One thread owns one bin: it loads the bin's seven state words, walks
// the block's rows ONE SAMPLE AT A TIME IN PUSH ORDER and stores the state back.  Rows are read coalesced with 64-bit row
// offsets, TM_PRED_UNROLL loads requested before the first is used; the status words come from device memory and a sample
// that is not OK is skipped (a wave-uniform test).  The loop is written out here and is not tms_walk
// (tamcmc_summary_walk.h): DESIGN.md has the measurement.  No LDS, no barrier, no atomics, no cross-lane work: a bin's
// results are bit for bit independent of the block size and of how the samples were split over pushes.  The number of
// accepted samples before the block is the pair the block's fold launch read; this kernel writes no count.
//
// Which of the three per-sample routines runs is decided by launch arguments alone (likelihood, p): chi_square; p = 1,
// which has no loop; p > 1, whose two loops have trip counts fixed by p (tamcmc_predictive.h says how its lane-dependent
// choices are laid out and why).  Everything is compiled without FMA contraction.
#include <hip/hip_runtime.h>
#include <cmath>

#pragma clang fp contract(off)

#include "tamcmc_predictive.h"
#include "tamcmc_summary_walk.h"

__global__ __launch_bounds__(TM_PRED_THREADS) void tamcmc_summary_predictive_kernel(const TmPredArgs a)
{
    const int bin = (int)(blockIdx.x * TM_PRED_THREADS + threadIdx.x);
    if (bin >= a.Nx) return;
    const size_t nx = (size_t)a.Nx;
    long long n = a.cnt_in[0];
    double *__restrict__ st = a.state + bin;
    double ca = st[TM_PRED_CDF_A * nx], cr = st[TM_PRED_CDF_R * nx], cc = st[TM_PRED_CDF_C * nx];
    double sa = st[TM_PRED_SF_A * nx], sr = st[TM_PRED_SF_R * nx], sc = st[TM_PRED_SF_C * nx];
    double mean = st[TM_PRED_MEAN_RESID * nx];
    const double y = a.y[bin];
    const bool gauss = a.likelihood_case != 0;
    const double isig = gauss ? sqrt(a.isig2[bin]) : 0.0;
    const int p = a.p;
    const double dp = (double)p;
    const double *__restrict__ rows = a.rows + bin;

    for (int s0 = 0; s0 < a.B; s0 += TM_PRED_UNROLL) {
        double v[TM_PRED_UNROLL];
#pragma unroll
        for (int k = 0; k < TM_PRED_UNROLL; k++)
            v[k] = (s0 + k < a.B) ? rows[(size_t)(s0 + k) * nx] : 1.0;       // (a rejected sample's row is loaded and dropped)
#pragma unroll
        for (int k = 0; k < TM_PRED_UNROLL; k++) {
            if (s0 + k >= a.B) break;
            if (a.status[s0 + k] != 0) continue;
            n++;
            double resid, lP, lQ;                             // (the residual is formed inside its branch: see DESIGN.md)
            if (gauss) {
                resid = tms_resid(true, y, v[k], isig);
                tmp_gauss(resid, &lP, &lQ);
            } else {
                resid = tms_resid(false, y, v[k], isig);
                if (p == 1) tmp_chi_p1(resid, &lP, &lQ);
                else tmp_chi_p(p, a.lf_pm1, a.lf_p, a.nterms, dp * y / v[k], &lP, &lQ);
            }
            tmp_lse_step(&ca, &cr, &cc, lP);
            tmp_lse_step(&sa, &sr, &sc, lQ);
            mean += (resid - mean) / (double)n;
        }
    }

    st[TM_PRED_CDF_A * nx] = ca; st[TM_PRED_CDF_R * nx] = cr; st[TM_PRED_CDF_C * nx] = cc;
    st[TM_PRED_SF_A * nx] = sa; st[TM_PRED_SF_R * nx] = sr; st[TM_PRED_SF_C * nx] = sc;
    st[TM_PRED_MEAN_RESID * nx] = mean;
}

int tm_launch_predictive(const TmPredArgs &a, void *stream)
{
    if (a.likelihood_case == 0 && (a.p < 1 || a.p > TM_PRED_MAX_P)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_summary_predictive_kernel, dim3(tms_blocks(a.Nx, TM_PRED_THREADS)), dim3(TM_PRED_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
