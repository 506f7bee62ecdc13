// tamcmc_bandess.hip -- stage 2 of a block of samples while a summary object is in band ESS mode (tamcmc_bandess.h), and the
// kernel that turns the pass's integer lag counts into per-bin tau, ESS and cut of every threshold.
//
// A block is cut into chunks of at most TM_ESS_CHUNK pushed samples; a chunk is two launches.
//
// Pack kernel.  One thread owns one bin, as in the fold kernel (tamcmc_summary.hip): rows are read coalesced with 64-bit row
// offsets; the status words come from device memory and are uniform over the wave, so a sample that is not OK is skipped
// and counted without divergence.  Every accepted row is compared with the bin's K thresholds (slots K ... 7 hold NaN and
// compare false) and the results are shifted into eight 64-bit registers, bit i for the chunk's i-th accepted sample; after
// the walk the c <= 64 bits of each threshold are appended to its ring and head at sample t0 (tmb_store_bits).  Thread 0 stores
// the new {accepted, rejected} pair into the other pair of words.
//
// Lag kernel.  One thread owns one bin, one threshold and TM_BANDESS_G consecutive lags: it takes the chunk's bits and the
// three ring words its lags' windows lie in, and adds popcount(new & window_k) to each of its counters (tmb_lag_group).  A
// workgroup is TM_BANDESS_BINS bins x TM_BANDESS_GROUPS lag groups, one wave per group, lanes along bins: every load and
// store is coalesced.  No LDS, no atomics: every counter belongs to one thread, and integer sums do not depend on the order
// of their terms, so the result is independent of the block size and of how the pass was split over pushes.
//
// Finish kernel.  One thread per bin, for one threshold: H_k and T_k by masked popcounts of the head and the ring, E_k in
// int64 (tmb_centred), written into the work column as doubles and handed to tme_finish -- or, for
// tamcmc_summary_bandess_counts, written as int64 and left there.  It reads the pass's state and writes only the work
// column and the three result arrays, so it can run again.
#include <hip/hip_runtime.h>
#include <cmath>

// tme_finish is compiled as in tamcmc_ess.hip: no FMA contraction
#pragma clang fp contract(off)

#include "tamcmc_bandess.h"
#include "tamcmc_summary_walk.h"

__global__ __launch_bounds__(TM_BANDESS_THREADS) void tamcmc_bandess_pack_kernel(const TmBandArgs a)
{
    const int bin = (int)(blockIdx.x * TM_BANDESS_THREADS + threadIdx.x);
    if (bin >= a.Nx) return;
    constexpr int MK = TM_BANDESS_MAX_K;
    const size_t nx = (size_t)a.Nx;
    const long long t0 = a.cnt_in[0];
    long long rej = a.cnt_in[1];
    double thr[MK];
    uint64_t nb[MK];
#pragma unroll
    for (int j = 0; j < MK; j++) {
        thr[j] = j < a.K ? a.thr[(size_t)j * nx + bin] : (double)NAN;
        nb[j] = 0;
    }
    const double *__restrict__ rows = a.rows + bin;
    int c = 0;
    for (int s = 0; s < a.B; s++) {
        const double v = rows[(size_t)s * nx];                               // (a rejected sample's row is loaded and dropped)
        if (a.status[s] != 0) { rej++; continue; }
#pragma unroll
        for (int j = 0; j < MK; j++) nb[j] |= tmb_le(v, thr[j]) << c;
        c++;
    }
    if (c > 0) {
#pragma unroll
        for (int j = 0; j < MK; j++)
            if (j < a.K)
                tmb_store_bits(a.ring + (size_t)j * (size_t)a.RW * nx + bin, a.head + (size_t)j * (size_t)a.HW * nx + bin, nx, a.RW, a.HW,
                               t0, c, nb[j]);
    }
    if (bin == 0) { a.cnt_out[0] = t0 + c; a.cnt_out[1] = rej; }
}

__global__ __launch_bounds__(TM_BANDESS_BINS * TM_BANDESS_GROUPS) void tamcmc_bandess_lag_kernel(const TmBandArgs a)
{
    const int bin = (int)(blockIdx.x * TM_BANDESS_BINS + threadIdx.x);
    const int k0 = (int)(blockIdx.y * TM_BANDESS_GROUPS + threadIdx.y) * TM_BANDESS_G;
    if (bin >= a.Nx || k0 > a.L) return;
    const size_t nx = (size_t)a.Nx, j = blockIdx.z;
    const long long t0 = a.cnt_in[0], t1 = a.cnt_out[0];
    if (t1 <= t0) return;                                                    // every sample of the chunk was rejected
    tmb_lag_group(a.ring + j * (size_t)a.RW * nx + bin, nx, a.RW, t0, t1, k0, a.L,
                  a.C + (j * (size_t)(a.L + 1) + (size_t)k0) * nx + bin, nx);
}

__global__ __launch_bounds__(TM_BANDESS_THREADS) void tamcmc_bandess_finish_kernel(const TmBandArgs a)
{
    const int bin = (int)(blockIdx.x * TM_BANDESS_THREADS + threadIdx.x);
    if (bin >= a.Nx) return;
    const size_t nx = (size_t)a.Nx, j = (size_t)a.j;
    const uint64_t *const ring = a.ring + j * (size_t)a.RW * nx + bin, *const head = a.head + j * (size_t)a.HW * nx + bin;
    const uint32_t *const C = a.C + j * (size_t)(a.L + 1) * nx + bin;
    if (a.want_E) {
        tmb_centred(ring, head, nx, a.RW, a.n, a.L, C, nx, static_cast<long long *>(a.work) + bin, nx);
        return;
    }
    double *const A = static_cast<double *>(a.work) + bin;
    tmb_centred(ring, head, nx, a.RW, a.n, a.L, C, nx, A, nx);
    const TmeFinish f = tme_finish(A, nx, a.L, (double)a.n, a.tau_floor);
    a.tau[j * nx + bin] = f.tau;
    a.ess[j * nx + bin] = f.ess;
    a.cut[j * nx + bin] = f.cut;
}

static bool bandess_args_ok(const TmBandArgs &a)
{
    return a.Nx >= 1 && a.L >= 1 && a.L <= TM_ESS_MAX_LAG && (a.L & 1) == 1 && a.RW == tmb_ring_words(a.L) && a.HW == tmb_head_words(a.L) &&
           a.K >= 1 && a.K <= TM_BANDESS_MAX_K && a.n > a.L && a.n < TM_BANDESS_MAX_N;
}

int tm_launch_bandess_chunk(const TmBandArgs &a, void *stream)
{
    if (!bandess_args_ok(a) || a.B < 1 || a.B > TM_ESS_CHUNK) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_bandess_pack_kernel, dim3(tms_blocks(a.Nx, TM_BANDESS_THREADS)), dim3(TM_BANDESS_THREADS), 0, (hipStream_t)stream, a);
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    const int groups = (a.L + 1 + TM_BANDESS_G - 1) / TM_BANDESS_G;
    const dim3 grid(tms_blocks(a.Nx, TM_BANDESS_BINS), (unsigned)((groups + TM_BANDESS_GROUPS - 1) / TM_BANDESS_GROUPS), (unsigned)a.K);
    hipLaunchKernelGGL(tamcmc_bandess_lag_kernel, grid, dim3(TM_BANDESS_BINS, TM_BANDESS_GROUPS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_bandess_finish(const TmBandArgs &a, void *stream)
{
    if (!bandess_args_ok(a) || a.j < 0 || a.j >= a.K) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_bandess_finish_kernel, dim3(tms_blocks(a.Nx, TM_BANDESS_THREADS)), dim3(TM_BANDESS_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
