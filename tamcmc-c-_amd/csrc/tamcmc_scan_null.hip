// tamcmc_scan_null.hip -- the Monte-Carlo null of the sliding-window scan (tamcmc_scan_null.h): per chunk of replicates two kernels.
//
//   extremes  one workgroup per (replicate, tile of TM_SCAN_TILE positions).  The variates of the tile's bins and of the halo
//             the widest window of its last position reaches into -- bins [j0, min(j0 + TM_SCAN_TILE + W_{K-1} - 1, Nx)) -- are
//             generated straight into LDS (tmn_variate: a function of seed, replicate and bin alone, so the halo needs no
//             neighbour).  Thread t owns the positions j0 + t, j0 + t + 256, ... in ascending order and runs the scan sums
//             kernel's walk: ONE ascending sum from q[j], taken off for width k when it has added W_k terms.  Instead of
//             storing it keeps per width the running maximum and minimum with their first positions (strict compares in
//             ascending position), reduces them over the wave by shuffles and over the four waves through LDS with
//             tmn_takes -- a total order on (sum, position), so the result does not depend on the reduction's shape -- and
//             writes one partial per (replicate, tile, width, side).  A width with no position in the tile writes position -1.
//   combine   one thread per (replicate, width, side): tmn_combine over the tiles in tile order.
//   variates  one thread per bin: tmn_variate into global memory, for tests and plots.
// A replicate's extremes depend on nothing but (seed, global replicate, Nx, the width): bit for bit independent of the chunk,
// of how the replicates were split over runs, of first_replicate and of which other widths are in the list.  Everything is
// compiled without FMA contraction; no atomics, no scratch.
#include <hip/hip_runtime.h>
#include <cmath>

#pragma clang fp contract(off)

#include "tamcmc_scan_null.h"

// grid: n x tiles workgroups, replicate blockIdx.x / tiles of the chunk
__global__ __launch_bounds__(TM_NULL_THREADS) void tamcmc_scan_null_extremes_kernel(const TmNullArgs a)
{
    __shared__ double q[TM_SCAN_LDS_DOUBLES];
    __shared__ double red_val[TM_NULL_WAVES][TM_SCAN_MAX_WIDTHS][2];
    __shared__ int red_pos[TM_NULL_WAVES][TM_SCAN_MAX_WIDTHS][2];
    const int tid = (int)threadIdx.x;
    const unsigned tiles = (unsigned)a.tiles;
    const unsigned slot = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const unsigned long long rep = a.rep0 + slot;
    const long long nx = a.Nx;
    const long long j0 = (long long)tile * TM_SCAN_TILE;
    int wmax = a.W[0];
#pragma unroll
    for (int k = 1; k < TM_SCAN_MAX_WIDTHS; k++) wmax = k < a.K ? a.W[k] : wmax;
    const long long e = j0 + TM_SCAN_TILE + wmax - 1;
    const int nb = (int)((e < nx ? e : nx) - j0);             // <= TM_SCAN_LDS_DOUBLES
    const bool gauss = a.gauss != 0;
    for (int b = tid; b < nb; b += TM_NULL_THREADS) q[b] = tmn_variate(gauss, a.p, a.seed, rep, (uint32_t)(j0 + b));
    __syncthreads();

    double mx[TM_SCAN_MAX_WIDTHS], mn[TM_SCAN_MAX_WIDTHS];
    int mxp[TM_SCAN_MAX_WIDTHS], mnp[TM_SCAN_MAX_WIDTHS];    // positions within the tile, -1: none
#pragma unroll
    for (int k = 0; k < TM_SCAN_MAX_WIDTHS; k++) { mx[k] = -(double)INFINITY; mn[k] = (double)INFINITY; mxp[k] = -1; mnp[k] = -1; }
    for (int t = tid; t < TM_SCAN_TILE; t += TM_NULL_THREADS) {
        const long long j = j0 + t;
        if (j + a.W[0] > nx) break;
        const double *qq = q + t;
        double sum = qq[0];
        int terms = 1;
#pragma unroll
        for (int k = 0; k < TM_SCAN_MAX_WIDTHS; k++) {
            if (k >= a.K) break;
            const int W = a.W[k];
            if (j + W > nx) break;                            // (and so for every wider one)
            for (; terms < W; terms++) sum += qq[terms];
            if (mxp[k] < 0 || sum > mx[k]) { mx[k] = sum; mxp[k] = t; }
            if (mnp[k] < 0 || sum < mn[k]) { mn[k] = sum; mnp[k] = t; }
        }
    }

    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < TM_SCAN_MAX_WIDTHS; k++) {
        if (k >= a.K) break;                                  // (uniform)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double v = __shfl_xor(mx[k], d);
            const int vp = __shfl_xor(mxp[k], d);
            if (tmn_takes(true, v, vp, mx[k], mxp[k])) { mx[k] = v; mxp[k] = vp; }
            const double u = __shfl_xor(mn[k], d);
            const int up = __shfl_xor(mnp[k], d);
            if (tmn_takes(false, u, up, mn[k], mnp[k])) { mn[k] = u; mnp[k] = up; }
        }
        if (lane == 0) {
            red_val[wave][k][0] = mx[k]; red_pos[wave][k][0] = mxp[k];
            red_val[wave][k][1] = mn[k]; red_pos[wave][k][1] = mnp[k];
        }
    }
    __syncthreads();
    if (tid < 2 * a.K) {
        const int k = tid >> 1, side = tid & 1;
        double best = red_val[0][k][side];
        int at = red_pos[0][k][side];
        for (int w = 1; w < TM_NULL_WAVES; w++)
            if (tmn_takes(side == 0, red_val[w][k][side], red_pos[w][k][side], best, at)) { best = red_val[w][k][side]; at = red_pos[w][k][side]; }
        const size_t o = ((size_t)blockIdx.x * (size_t)a.K + (size_t)k) * 2 + (size_t)side;
        a.part_val[o] = best;
        a.part_pos[o] = at < 0 ? -1 : j0 + at;
    }
}

// one thread per (replicate of the chunk, width, side)
__global__ __launch_bounds__(TM_NULL_THREADS) void tamcmc_scan_null_combine_kernel(const TmNullArgs a)
{
    const long long g = (long long)blockIdx.x * TM_NULL_THREADS + threadIdx.x;
    const long long per = 2LL * a.K;
    if (g >= (long long)a.n * per) return;
    const long long r = g / per, ks = g % per;
    const size_t first = (size_t)r * (size_t)a.tiles * (size_t)per + (size_t)ks;
    double v;
    long long at;
    tmn_combine((ks & 1) == 0, a.tiles, (size_t)per, a.part_val + first, a.part_pos + first, &v, &at);
    a.ext_val[g] = v;
    a.ext_pos[g] = at;
}

__global__ __launch_bounds__(TM_NULL_THREADS) void tamcmc_scan_null_variates_kernel(const TmNullArgs a, const unsigned long long rep, double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * TM_NULL_THREADS + threadIdx.x;
    if (i < a.Nx) out[i] = tmn_variate(a.gauss != 0, a.p, a.seed, rep, (uint32_t)i);
}

static bool null_args_ok(const TmNullArgs &a)
{
    if (a.K < 1 || a.K > TM_SCAN_MAX_WIDTHS || a.Nx < 1 || a.Nx > 0x7FFFFFFFLL || a.p < 1) return false;
    for (int k = 0; k < a.K; k++)
        if (a.W[k] < 1 || a.W[k] > TM_WIN_MAX_BINS || a.W[k] > a.Nx || (k > 0 && a.W[k] <= a.W[k - 1])) return false;
    return true;
}

int tm_launch_scan_null(const TmNullArgs &a, void *stream)
{
    if (!null_args_ok(a) || a.n < 1 || a.tiles != tmn_tiles(a.Nx, a.W[0]) || (long long)a.n > tmn_chunk(a.tiles, a.K) || !a.part_val ||
        !a.part_pos || !a.ext_val || !a.ext_pos)
        return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tamcmc_scan_null_extremes_kernel, dim3((unsigned)((long long)a.n * a.tiles)), dim3(TM_NULL_THREADS), 0, st, a);
    const long long threads = (long long)a.n * 2 * a.K;
    hipLaunchKernelGGL(tamcmc_scan_null_combine_kernel, dim3((unsigned)((threads + TM_NULL_THREADS - 1) / TM_NULL_THREADS)), dim3(TM_NULL_THREADS), 0, st, a);
    return (int)hipGetLastError();
}

int tm_launch_scan_null_variates(const TmNullArgs &a, unsigned long long rep, double *d_q, void *stream)
{
    if (!null_args_ok(a) || !d_q) return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((a.Nx + TM_NULL_THREADS - 1) / TM_NULL_THREADS);
    hipLaunchKernelGGL(tamcmc_scan_null_variates_kernel, dim3(blocks), dim3(TM_NULL_THREADS), 0, (hipStream_t)stream, a, rep, d_q);
    return (int)hipGetLastError();
}
