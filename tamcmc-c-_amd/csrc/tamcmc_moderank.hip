// tamcmc_moderank.hip -- the kernels behind tamcmc_moderank_* (tamcmc_moderank.h): the sorted keys of a column and of its
// folded values, the four rank-normalised series of a column, and their means.  The lag products and the finish of the
// series are tamcmc_modediag.hip's kernels, launched on the series table as it is.  fp64 and 64-bit integer VALU; no
// MFMA, no atomics, no waiting across workgroups.
//
//   sort       one workgroup of 1024 threads per column: a bitonic network on the column's keys, padded to a power of two
//              with the largest key.  Stages whose distance is below the tile (8192 keys, 64 KiB of LDS) run in LDS, a tile
//              at a time; the wider stages run on the column's key buffer in device memory, which at 65 536 rows is 512 KiB
//              and stays in L2.  The workgroup waits for itself between stages (__syncthreads, which also orders its own
//              global stores and loads); no other workgroup reads the buffer before the launch has ended.  With `fold` the
//              keys are those of |v - med|, med read from the value launch's sorted keys.
//   transform  one thread per (column, sample): the two bounds of key(v_t) in the sorted column and of key(f_t) in the sorted
//              folded column by binary search (17 steps at 65 536 rows, the loads of the two bounds independent), z of
//              either rank, the two tail indicators; four coalesced stores.  No LDS.
//   mean       one thread per series: Welford's mean in t order, 8 loads in flight.  No LDS.
#include <hip/hip_runtime.h>
#include <cmath>

// no FMA contraction anywhere in this file
#pragma clang fp contract(off)

#include "tamcmc_ess.h"
#include "tamcmc_moderank.h"

__global__ __launch_bounds__(TM_MR_SORT_THREADS) void tamcmc_moderank_sort_kernel(const TmMrArgs a, const int fold)
{
    __shared__ uint64_t s_k[TM_MR_TILE];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (c >= a.w) return;
    const double *__restrict__ v = a.table + (size_t)a.sel[c] * (size_t)a.max_samples;
    uint64_t *keys = a.keys + ((size_t)(fold ? a.w : 0) + (size_t)c) * (size_t)a.P;
    const double med = fold ? tmr_median(a.keys + (size_t)c * (size_t)a.P, a.n) : 0.0;
    const long long P = a.P;
    const int T = (int)tmr_tile(P);
    // every stage up to block size T, tile by tile, straight from the table
    for (long long base = 0; base < P; base += T) {
        for (int i = tid; i < T; i += TM_MR_SORT_THREADS) {
            const long long t = base + i;
            uint64_t key = ~(uint64_t)0;
            if (t < a.n) key = tmq_key(fold ? tmr_fold(v[t], med) : v[t]);
            s_k[i] = key;
        }
        __syncthreads();
        for (long long k = 2; k <= T; k <<= 1)
            for (int j = (int)(k >> 1); j >= 1; j >>= 1) {
                tmr_tile_stage(s_k, T, base, k, j, tid, TM_MR_SORT_THREADS);
                __syncthreads();
            }
        for (int i = tid; i < T; i += TM_MR_SORT_THREADS) keys[base + i] = s_k[i];
        __syncthreads();
    }
    // the wider blocks: distances >= T on the key buffer, the rest of each block's stages tile by tile
    for (long long k = 2 * (long long)T; k <= P; k <<= 1) {
        for (long long j = k >> 1; j >= T; j >>= 1) {
            tmr_wide_stage(keys, P, k, j, tid, TM_MR_SORT_THREADS);
            __syncthreads();
        }
        for (long long base = 0; base < P; base += T) {
            for (int i = tid; i < T; i += TM_MR_SORT_THREADS) s_k[i] = keys[base + i];
            __syncthreads();
            for (int j = T >> 1; j >= 1; j >>= 1) {
                tmr_tile_stage(s_k, T, base, k, j, tid, TM_MR_SORT_THREADS);
                __syncthreads();
            }
            for (int i = tid; i < T; i += TM_MR_SORT_THREADS) keys[base + i] = s_k[i];
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(TM_MR_THREADS) void tamcmc_moderank_transform_kernel(const TmMrArgs a)
{
    const int c = blockIdx.y;
    const long long t = (long long)blockIdx.x * TM_MR_THREADS + threadIdx.x;
    if (c >= a.w || t >= a.n) return;
    const size_t n = (size_t)a.n, P = (size_t)a.P, w = (size_t)a.w;
    const uint64_t *__restrict__ sv = a.keys + (size_t)c * P, *__restrict__ sf = a.keys + (w + (size_t)c) * P;
    const double med = tmr_median(sv, a.n), Q05 = tmq_unkey(sv[a.r05]), Q95 = tmq_unkey(sv[a.r95]);
    const double v = a.table[(size_t)a.sel[c] * (size_t)a.max_samples + (size_t)t];
    const double f = tmr_fold(v, med);
    double *s = a.series + (size_t)TM_MR_NSERIES * (size_t)c * n + (size_t)t;
#pragma nounroll
    for (int fold = 0; fold < 2; fold++) {                                   // TM_MR_Z, then TM_MR_ZFOLD
        const long long r = tmr_rank2(fold ? sf : sv, a.n, tmq_key(fold ? f : v));
        s[(size_t)fold * n] = tmr_z(r, a.n);
        if (a.rank2) a.rank2[((size_t)fold * w + (size_t)c) * n + (size_t)t] = r;
    }
    s[(size_t)TM_MR_I05 * n] = tmr_indicator(v, Q05);
    s[(size_t)TM_MR_I95 * n] = tmr_indicator(v, Q95);
    if (t == 0) {
        a.medq[c] = med;
        a.medq[w + (size_t)c] = Q05;
        a.medq[2 * w + (size_t)c] = Q95;
    }
}

__global__ __launch_bounds__(TM_MR_MEAN_THREADS) void tamcmc_moderank_mean_kernel(const TmMrArgs a)
{
    const int s = (int)(blockIdx.x * TM_MR_MEAN_THREADS + threadIdx.x);
    if (s >= TM_MR_NSERIES * a.w) return;
    const double *__restrict__ x = a.series + (size_t)s * (size_t)a.n;
    double mean = 0.0, M2 = 0.0;
    for (long long i0 = 0; i0 < a.n; i0 += TM_MR_MEAN_UNROLL) {
        double y[TM_MR_MEAN_UNROLL];
#pragma unroll
        for (int u = 0; u < TM_MR_MEAN_UNROLL; u++) y[u] = x[i0 + u < a.n ? i0 + u : a.n - 1];   // (past the end: the last value again, not taken)
#pragma unroll
        for (int u = 0; u < TM_MR_MEAN_UNROLL; u++) {
            if (i0 + u >= a.n) break;
            tme_welford(&mean, &M2, i0 + u + 1, y[u]);
        }
    }
    a.mean[s] = mean;
}

static bool mr_args_ok(const TmMrArgs &a)
{
    return a.w >= 1 && a.n >= 4 && a.n <= a.max_samples && a.P == tmr_padded(a.n) && a.r05 >= 0 && a.r05 < a.n && a.r95 >= 0 && a.r95 < a.n &&
           (long long)a.w * TM_MR_NSERIES <= 0x7fffffffLL;
}

int tm_launch_moderank_sort(const TmMrArgs &a, int fold, void *stream)
{
    if (!mr_args_ok(a)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_moderank_sort_kernel, dim3((unsigned)a.w), dim3(TM_MR_SORT_THREADS), 0, (hipStream_t)stream, a, fold);
    return (int)hipGetLastError();
}

int tm_launch_moderank_transform(const TmMrArgs &a, void *stream)
{
    if (!mr_args_ok(a) || a.w > 65535) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.n + TM_MR_THREADS - 1) / TM_MR_THREADS), (unsigned)a.w);
    hipLaunchKernelGGL(tamcmc_moderank_transform_kernel, grid, dim3(TM_MR_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_moderank_mean(const TmMrArgs &a, void *stream)
{
    if (!mr_args_ok(a)) return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((TM_MR_NSERIES * a.w + TM_MR_MEAN_THREADS - 1) / TM_MR_MEAN_THREADS);
    hipLaunchKernelGGL(tamcmc_moderank_mean_kernel, dim3(blocks), dim3(TM_MR_MEAN_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
