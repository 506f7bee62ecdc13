// tamcmc_loo.hip -- stage 2 of a block of samples while a summary object is in LOO mode (tamcmc_loo.h), and the kernel that
// turns the pass into per-bin PSIS-LOO results.
//
// Tail kernel.  One thread owns one bin and walks the block's rows as the fold kernel does: rows are read coalesced with
// 64-bit row offsets, TM_LOO_UNROLL loads requested before the first is used; the status words come from device memory and
// a sample that is not OK is skipped and counted.  The loop is written out here and is not tms_walk
// (tamcmc_summary_walk.h): DESIGN.md has the measurement.  Per bin the thread keeps the exact multiset of the M + 1
// largest x = -l seen so far in a binary min-heap laid out [slot][Nx] (a wave's accesses to one slot are consecutive),
// with the root in a register: the common sample (x <= root) goes into the body's running-maximum log-sum-exp (a Kahan sum
// whose maximum follows lazily: tamcmc_loo.h) and touches no memory.
// While the heap fills, every thread writes the same slots (the number of accepted samples is the same for every bin); a
// replacement walks down a path of its own.  No LDS, no atomics, no cross-thread reduction: a bin's state after a pass is
// bit for bit independent of the block size and of how the pass was split over pushes.
// l is the fold kernel's: both call tms_like (tamcmc_summary_walk.h).
//
// Finalize kernel.  One wave per bin.  The bin's heap goes into LDS (the M <= 2048 values above the root, padded with
// +inf to a power of two), is sorted ascending by a bitonic network, and tml_finalize (tamcmc_loo.h) does the rest with
// fixed-order wave reductions: 64 partial sums over the tail in stride-64 order, then a butterfly of 6 exchanges that
// leaves the same bits in every lane.  LDS: the sorted values, the tail's t_j, and the profile's theta / l: 2 x 16 KiB +
// 1.2 KiB.  The kernel reads the pass's state and writes only the four result arrays, so it can run again.
#include <hip/hip_runtime.h>
#include <cmath>

// no FMA contraction anywhere in this file: the shared arithmetic of tamcmc_loo.h (heap, body sum, tml_finalize) is
// compiled under that rule
#pragma clang fp contract(off)

#include "tamcmc_loo.h"
#include "tamcmc_summary_walk.h"

__global__ __launch_bounds__(TM_LOO_THREADS) void tamcmc_loo_tail_kernel(const TmLooArgs a)
{
    const int bin = (int)(blockIdx.x * TM_LOO_THREADS + threadIdx.x);
    if (bin >= a.Nx) return;
    const size_t nx = (size_t)a.Nx;
    long long n = a.cnt_in[0], rej = a.cnt_in[1];
    double *const heap = a.heap + bin;
    double root = n > 0 ? heap[0] : 0.0;
    double ba = a.body[bin], br = a.body[nx + bin], bc = a.body[2 * nx + bin];
    const TmsBinLike lk(a, bin);
    const double *__restrict__ rows = a.rows + bin;
    for (int s0 = 0; s0 < a.B; s0 += TM_LOO_UNROLL) {
        double v[TM_LOO_UNROLL];
#pragma unroll
        for (int k = 0; k < TM_LOO_UNROLL; k++)
            v[k] = (s0 + k < a.B) ? rows[(size_t)(s0 + k) * nx] : 1.0;       // (a rejected sample's row is loaded and dropped)
#pragma unroll
        for (int k = 0; k < TM_LOO_UNROLL; k++) {
            if (s0 + k >= a.B) break;
            if (a.status[s0 + k] != 0) { rej++; continue; }
            tml_top_push(heap, nx, a.cap, n, -lk.l(v[k]), &root, &ba, &br, &bc);
            n++;
        }
    }

    a.body[bin] = ba; a.body[nx + bin] = br; a.body[2 * nx + bin] = bc;
    if (bin == 0) { a.cnt_out[0] = n; a.cnt_out[1] = rej; }
}

__global__ __launch_bounds__(TM_LOO_THREADS) void tamcmc_loo_finalize_kernel(const TmLooArgs a)
{
    __shared__ double s[TM_LOO_MAX_TAIL], t[TM_LOO_MAX_TAIL];
    __shared__ double theta[TM_LOO_MAX_THETA], ell[TM_LOO_MAX_THETA];
    const int bin = (int)blockIdx.x, lane = (int)threadIdx.x;
    const size_t nx = (size_t)a.Nx;
    const int cnt = a.n < (long long)a.cap ? (int)a.n : a.cap;               // >= 1: the host does not launch for n = 0
    const int ncand = cnt - 1;                                               // <= M <= TM_LOO_MAX_TAIL
    const double *heap = a.heap + bin;
    const double root = heap[0];
    tml_load_sorted(heap, nx, ncand, s);
    TmlWave w;
    const TmlBin r = tml_finalize(w, s, ncand, root, a.n >= (long long)a.cap, a.n, a.body[bin], a.body[nx + bin] - a.body[2 * nx + bin], t, theta, ell);
    if (lane == 0) {
        a.elpd[bin] = r.elpd_loo; a.khat[bin] = r.pareto_k; a.cutoff[bin] = r.cutoff; a.tail_len[bin] = r.tail_len;
    }
}

int tm_launch_loo_tail(const TmLooArgs &a, void *stream)
{
    if (a.cap < 2 || a.cap > TM_LOO_MAX_TAIL + 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_loo_tail_kernel, dim3(tms_blocks(a.Nx, TM_LOO_THREADS)), dim3(TM_LOO_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_loo_finalize(const TmLooArgs &a, void *stream)
{
    if (a.cap < 2 || a.cap > TM_LOO_MAX_TAIL + 1 || a.n < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_loo_finalize_kernel, dim3((unsigned)a.Nx), dim3(TM_LOO_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
