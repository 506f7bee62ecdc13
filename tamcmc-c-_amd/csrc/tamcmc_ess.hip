// tamcmc_ess.hip -- stage 2 of a block of samples while a summary object is in ESS mode (tamcmc_ess.h), and the kernel that
// turns the pass's lag products into per-bin tau, ESS and cut.
//
// A block is cut into chunks of at most TM_ESS_CHUNK pushed samples; a chunk is two launches.
//
// Centre kernel.  One thread owns one bin, as in the fold kernel (tamcmc_summary.hip): rows are read coalesced with 64-bit
// row offsets; the status words come from device memory and a sample that is not OK is skipped and counted.  The loop is the
// kernel's own, one load at a time: tms_walk (tamcmc_summary_walk.h) changes its registers; l is tms_like.  For every
// accepted sample t the thread writes the two centred values a_t = M - mean_M and u_t = exp(l - lppd) - 1 into slot t mod R
// of the two rings (R = L + TM_ESS_CHUNK: the chunk's values land behind the L values before them, which stay readable), and
// folds M into the Welford moments of the half-chain t belongs to.  Thread 0 stores the new {accepted, rejected} pair into
// the other pair of words.
//
// Lag kernel.  One thread owns one bin, one series and TM_ESS_G consecutive lags: it keeps those accumulators and the
// window of past values in registers and walks the chunk's accepted samples t0 ... t1 - 1 (the two count pairs) in
// ascending t: per sample one load of d_t and one of d_{t-k0} from the ring, TM_ESS_G fused multiply-adds (tme_lag_group).
// A workgroup is TM_ESS_BINS bins x TM_ESS_GROUPS lag groups, one wave per group, lanes along bins.  No LDS, no atomics, no
// cross-thread reduction: every (bin, lag) accumulator belongs to one thread and takes its terms in sample order, so the
// result is bit for bit independent of the block size and of how the pass was split over pushes.
//
// Finish kernel.  One thread per bin and series: tme_finish on the bin's column of accumulators.  It reads the pass's state
// and writes only the three result arrays, so it can run again.
#include <hip/hip_runtime.h>
#include <cmath>

// no FMA contraction anywhere in this file: the shared arithmetic of tamcmc_ess.h is compiled under that rule (its one
// fused operation is written out)
#pragma clang fp contract(off)

#include "tamcmc_ess.h"
#include "tamcmc_summary_walk.h"

__global__ __launch_bounds__(TM_ESS_THREADS) void tamcmc_ess_centre_kernel(const TmEssArgs a)
{
    const int bin = (int)(blockIdx.x * TM_ESS_THREADS + threadIdx.x);
    if (bin >= a.Nx) return;
    const size_t nx = (size_t)a.Nx;
    long long t = a.cnt_in[0], rej = a.cnt_in[1];
    const int R = a.R;
    int slot = (int)(t % R);
    const TmsBinLike lk(a, bin);
    const double mean_M = a.mean_M[bin], lppd = a.lppd[bin];
    double *const hs = a.half + bin;
    double m1 = hs[TM_ESS_H1_MEAN * nx], q1 = hs[TM_ESS_H1_M2 * nx], m2 = hs[TM_ESS_H2_MEAN * nx], q2 = hs[TM_ESS_H2_M2 * nx];
    const double *__restrict__ rows = a.rows + bin;
    double *const ring_M = a.ring + bin, *const ring_l = a.ring + (size_t)R * nx + bin;

    for (int s = 0; s < a.B; s++) {
        const double v = rows[(size_t)s * nx];                               // (a rejected sample's row is loaded and dropped)
        if (a.status[s] != 0) { rej++; continue; }
        ring_M[(size_t)slot * nx] = tme_centre_model(v, mean_M);
        ring_l[(size_t)slot * nx] = tme_centre_like(lk.l(v), lppd);
        if (t < a.h) tme_welford(&m1, &q1, t + 1, v);
        if (t >= a.n - a.h && t < a.n) tme_welford(&m2, &q2, t - (a.n - a.h) + 1, v);
        t++;
        slot = slot + 1 == R ? 0 : slot + 1;
    }

    hs[TM_ESS_H1_MEAN * nx] = m1; hs[TM_ESS_H1_M2 * nx] = q1; hs[TM_ESS_H2_MEAN * nx] = m2; hs[TM_ESS_H2_M2 * nx] = q2;
    if (bin == 0) { a.cnt_out[0] = t; a.cnt_out[1] = rej; }
}

__global__ __launch_bounds__(TM_ESS_BINS * TM_ESS_GROUPS) void tamcmc_ess_lag_kernel(const TmEssArgs a)
{
    const int bin = (int)(blockIdx.x * TM_ESS_BINS + threadIdx.x);
    const int k0 = (int)(blockIdx.y * TM_ESS_GROUPS + threadIdx.y) * TM_ESS_G;
    if (bin >= a.Nx || k0 > a.L) return;
    const size_t nx = (size_t)a.Nx, series = blockIdx.z;
    const long long t0 = a.cnt_in[0], t1 = a.cnt_out[0];
    if (t1 <= t0) return;                                                    // every sample of the chunk was rejected
    tme_lag_group(a.ring + series * (size_t)a.R * nx + bin, nx, a.R, t0, t1, k0, a.L,
                  a.acc + (series * (size_t)(a.L + 1) + (size_t)k0) * nx + bin);
}

__global__ __launch_bounds__(TM_ESS_THREADS) void tamcmc_ess_finish_kernel(const TmEssArgs a)
{
    const int bin = (int)(blockIdx.x * TM_ESS_THREADS + threadIdx.x);
    if (bin >= a.Nx) return;
    const size_t nx = (size_t)a.Nx, series = blockIdx.y;
    const TmeFinish f = tme_finish(a.acc + series * (size_t)(a.L + 1) * nx + bin, nx, a.L, (double)a.n, a.tau_floor);
    a.tau[series * nx + bin] = f.tau;
    a.ess[series * nx + bin] = f.ess;
    a.cut[series * nx + bin] = f.cut;
}

static bool ess_args_ok(const TmEssArgs &a)
{
    return a.Nx >= 1 && a.L >= 1 && a.L <= TM_ESS_MAX_LAG && (a.L & 1) == 1 && a.R == tme_ring_slots(a.L);
}

int tm_launch_ess_chunk(const TmEssArgs &a, void *stream)
{
    if (!ess_args_ok(a) || a.B < 1 || a.B > TM_ESS_CHUNK) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_ess_centre_kernel, dim3(tms_blocks(a.Nx, TM_ESS_THREADS)), dim3(TM_ESS_THREADS), 0, (hipStream_t)stream, a);
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    const int groups = (a.L + 1 + TM_ESS_G - 1) / TM_ESS_G;
    const dim3 grid(tms_blocks(a.Nx, TM_ESS_BINS), (unsigned)((groups + TM_ESS_GROUPS - 1) / TM_ESS_GROUPS), 2);
    hipLaunchKernelGGL(tamcmc_ess_lag_kernel, grid, dim3(TM_ESS_BINS, TM_ESS_GROUPS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_ess_finish(const TmEssArgs &a, void *stream)
{
    if (!ess_args_ok(a) || a.n < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_ess_finish_kernel, dim3(tms_blocks(a.Nx, TM_ESS_THREADS), 2), dim3(TM_ESS_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
