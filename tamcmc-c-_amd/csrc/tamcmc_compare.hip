// tamcmc_compare.hip -- the kernels of the comparison of fits (tamcmc_compare.h; definitions in include/tamcmc_accel_compare.h).
//
//   bootstrap  one workgroup per (tile of TM_CMP_TILE units, group of TM_CMP_PAIRS pairs of replicates).  Thread t owns the
//              units j0 + t + 256 u, u = 0 ... 7: it forms their D_k = elpd[k] - elpd[0] once, keeps them in registers and
//              works through the group's pairs: per unit one Philox call and two logarithms give the variates of replicates
//              2 m and 2 m + 1, added in ascending u to A and B_1 ... B_{K-1} of either replicate.  The 2 K sums go over the
//              wave by a butterfly, over the four waves through LDS in wave order, and one partial per (replicate, tile, column)
//              is written.  The kernel is bound by the software fp64 log and Philox's integer multiplies: the tile is eight
//              units a thread so that the 2 K butterflies of a pair stay small beside its sixteen logarithms.
//   finish     one thread per (replicate of the chunk, fit k >= 1): A and B_k over the tiles in tile order, z = tmc_z.
//   variates   one thread per unit: tmc_variate into global memory, for tests.
//   prepare    one thread per unit: P_k = tmc_P of an included unit, P_0 = -1 of an excluded one.
//   stack sums one workgroup per tile of TM_CMP_STACK_TILE units: thread t owns the units j0 + t + 256 u, u = 0 ... 15, and adds
//              P_k / den and log(den) at the state's w in ascending u; butterfly, waves in order, one partial row per tile.
//              Returns at once when the state is frozen.
//   update     one workgroup of K + 1 waves: wave c adds column c of the partial rows, lane l the tiles l, l + 64, ... in
//              ascending order, then the butterfly; thread 0 runs tmc_em_step.
// A replicate's z depends on (seed, global replicate, the inputs) alone; everything is compiled without FMA contraction; no
// atomics, no scratch.
#include <hip/hip_runtime.h>
#include <cmath>

#pragma clang fp contract(off)

#include "tamcmc_compare.h"

__device__ __forceinline__ double tmc_wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// grid: (tiles, groups of pairs)
__global__ __launch_bounds__(TM_CMP_THREADS) void tamcmc_compare_bootstrap_kernel(const TmCmpArgs a)
{
    __shared__ double red[TM_CMP_WAVES][2][TM_CMP_MAX_FITS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K;
    const long long N = a.N;
    const long long i0 = (long long)blockIdx.x * TM_CMP_TILE + tid;
    double D[TM_CMP_UPT][TM_CMP_MAX_FITS - 1];
    unsigned inc = 0u;
#pragma unroll
    for (int u = 0; u < TM_CMP_UPT; u++) {
        const long long i = i0 + (long long)u * TM_CMP_THREADS;
        const bool in = i < N;
        const double e0 = in ? a.elpd[i] : 0.0;
        bool ok = in && tmc_finite(e0);
#pragma unroll
        for (int k = 1; k < TM_CMP_MAX_FITS; k++) {
            double v = e0;
            if (k < K && in) v = a.elpd[(size_t)k * (size_t)N + (size_t)i];
            ok = ok && tmc_finite(v);
            D[u][k - 1] = v - e0;
        }
        inc |= ok ? 1u << u : 0u;
    }

    const long long slots = tmc_slots(a.g0, a.n);
    const long long s0 = (long long)blockIdx.y * TM_CMP_PAIRS;
    const long long s1 = s0 + TM_CMP_PAIRS < slots ? s0 + TM_CMP_PAIRS : slots;
    const unsigned long long pair0 = a.g0 >> 1;
    for (long long s = s0; s < s1; s++) {
        double A0 = 0.0, A1 = 0.0, B0[TM_CMP_MAX_FITS - 1], B1[TM_CMP_MAX_FITS - 1];
#pragma unroll
        for (int k = 0; k < TM_CMP_MAX_FITS - 1; k++) { B0[k] = 0.0; B1[k] = 0.0; }
#pragma unroll
        for (int u = 0; u < TM_CMP_UPT; u++) {
            if (!((inc >> u) & 1u)) continue;
            double e0, e1;
            tmc_variates2(a.seed, pair0 + (unsigned long long)s, (uint32_t)(i0 + (long long)u * TM_CMP_THREADS), &e0, &e1);
            A0 += e0;
            A1 += e1;
#pragma unroll
            for (int k = 0; k < TM_CMP_MAX_FITS - 1; k++) {
                if (k + 1 >= K) break;
                B0[k] += e0 * D[u][k];
                B1[k] += e1 * D[u][k];
            }
        }
        A0 = tmc_wave_sum(A0);
        A1 = tmc_wave_sum(A1);
        if (lane == 0) { red[wave][0][0] = A0; red[wave][1][0] = A1; }
#pragma unroll
        for (int k = 0; k < TM_CMP_MAX_FITS - 1; k++) {
            if (k + 1 >= K) break;                            // (uniform)
            const double b0 = tmc_wave_sum(B0[k]), b1 = tmc_wave_sum(B1[k]);
            if (lane == 0) { red[wave][0][k + 1] = b0; red[wave][1][k + 1] = b1; }
        }
        __syncthreads();
        if (tid < 2 * K) {
            const int half = tid / K, col = tid % K;
            double v = red[0][half][col];
            for (int w = 1; w < TM_CMP_WAVES; w++) v += red[w][half][col];
            a.part[(((size_t)s * 2 + (size_t)half) * (size_t)a.tiles + (size_t)blockIdx.x) * (size_t)K + (size_t)col] = v;
        }
        __syncthreads();
    }
}

// one thread per (replicate of the chunk, fit k >= 1)
__global__ __launch_bounds__(TM_CMP_THREADS) void tamcmc_compare_finish_kernel(const TmCmpArgs a)
{
    const long long t = (long long)blockIdx.x * TM_CMP_THREADS + threadIdx.x;
    const int K = a.K;
    if (t >= (long long)a.n * (K - 1)) return;
    const long long r = t / (K - 1);
    const int k = (int)(t % (K - 1)) + 1;
    const unsigned long long g = a.g0 + (unsigned long long)r;
    const size_t slot = (size_t)((g >> 1) - (a.g0 >> 1)), half = (size_t)(g & 1);
    const double *p = a.part + (slot * 2 + half) * (size_t)a.tiles * (size_t)K;
    double A = 0.0, B = 0.0;
    for (int tile = 0; tile < a.tiles; tile++) { A += p[(size_t)tile * (size_t)K]; B += p[(size_t)tile * (size_t)K + (size_t)k]; }
    a.z[t] = tmc_z(a.Np, A, B);
}

__global__ __launch_bounds__(TM_CMP_THREADS) void tamcmc_compare_variates_kernel(const TmCmpArgs a, const unsigned long long g, double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * TM_CMP_THREADS + threadIdx.x;
    if (i < a.N) out[i] = tmc_variate(a.seed, g, (uint32_t)i);
}

__global__ __launch_bounds__(TM_CMP_THREADS) void tamcmc_compare_prepare_kernel(const TmCmpStackArgs a)
{
    const long long i = (long long)blockIdx.x * TM_CMP_THREADS + threadIdx.x;
    if (i >= a.N) return;
    const int K = a.K;
    if (!tmc_included(K, a.elpd, a.N, i)) {
        for (int k = 0; k < K; k++) a.P[(size_t)k * (size_t)a.N + (size_t)i] = k == 0 ? -1.0 : 0.0;
        return;
    }
    double vmax = a.elpd[i];
    for (int k = 1; k < K; k++) { const double v = a.elpd[(size_t)k * (size_t)a.N + (size_t)i]; vmax = v > vmax ? v : vmax; }
    for (int k = 0; k < K; k++) a.P[(size_t)k * (size_t)a.N + (size_t)i] = tmc_P(a.scale, a.elpd[(size_t)k * (size_t)a.N + (size_t)i], vmax);
}

// grid: stacking tiles; TABLE: P is read from the table, otherwise formed from elpd
template <bool TABLE>
__global__ __launch_bounds__(TM_CMP_THREADS) void tamcmc_compare_stack_sums_kernel(const TmCmpStackArgs a)
{
    __shared__ double red[TM_CMP_WAVES][TM_CMP_STACK_COLS];
    if (a.state->frozen) return;                              // (uniform)
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K;
    const long long N = a.N;
    double w[TM_CMP_MAX_FITS], acc[TM_CMP_MAX_FITS], accl = 0.0;
#pragma unroll
    for (int k = 0; k < TM_CMP_MAX_FITS; k++) { w[k] = k < K ? a.state->w[k] : 0.0; acc[k] = 0.0; }
    const long long i0 = (long long)blockIdx.x * TM_CMP_STACK_TILE + tid;
    for (int u = 0; u < TM_CMP_STACK_UPT; u++) {
        const long long i = i0 + (long long)u * TM_CMP_THREADS;
        if (i >= N) break;
        double P[TM_CMP_MAX_FITS];
        if (TABLE) {
            P[0] = a.P[i];
            if (P[0] < 0.0) continue;
#pragma unroll
            for (int k = 1; k < TM_CMP_MAX_FITS; k++) P[k] = k < K ? a.P[(size_t)k * (size_t)N + (size_t)i] : 0.0;
        } else {
            double v[TM_CMP_MAX_FITS];
            bool ok = true;
#pragma unroll
            for (int k = 0; k < TM_CMP_MAX_FITS; k++) {
                P[k] = 0.0;
                if (k >= K) break;
                v[k] = a.elpd[(size_t)k * (size_t)N + (size_t)i];
                ok = ok && tmc_finite(v[k]);
            }
            if (!ok) continue;
            double vmax = v[0];
#pragma unroll
            for (int k = 1; k < TM_CMP_MAX_FITS; k++) {
                if (k >= K) break;
                vmax = v[k] > vmax ? v[k] : vmax;
            }
#pragma unroll
            for (int k = 0; k < TM_CMP_MAX_FITS; k++) {
                if (k >= K) break;
                P[k] = tmc_P(a.scale, v[k], vmax);
            }
        }
        double den = w[0] * P[0];
#pragma unroll
        for (int k = 1; k < TM_CMP_MAX_FITS; k++) {
            if (k >= K) break;
            den += w[k] * P[k];
        }
#pragma unroll
        for (int k = 0; k < TM_CMP_MAX_FITS; k++) {
            if (k >= K) break;
            acc[k] += P[k] / den;
        }
        accl += log(den);
    }
#pragma unroll
    for (int k = 0; k < TM_CMP_MAX_FITS; k++) {
        if (k >= K) break;
        const double v = tmc_wave_sum(acc[k]);
        if (lane == 0) red[wave][k] = v;
    }
    accl = tmc_wave_sum(accl);
    if (lane == 0) red[wave][TM_CMP_MAX_FITS] = accl;
    __syncthreads();
    if (tid < TM_CMP_STACK_COLS && (tid < K || tid == TM_CMP_MAX_FITS)) {
        double v = red[0][tid];
        for (int wv = 1; wv < TM_CMP_WAVES; wv++) v += red[wv][tid];
        a.part[(size_t)blockIdx.x * TM_CMP_STACK_COLS + (size_t)tid] = v;
    }
}

// one workgroup of TM_CMP_STACK_COLS waves
__global__ __launch_bounds__(TM_CMP_STACK_COLS * 64) void tamcmc_compare_stack_update_kernel(const TmCmpStackArgs a)
{
    __shared__ double sum[TM_CMP_STACK_COLS];
    if (a.state->frozen) return;                              // (uniform)
    const int tid = (int)threadIdx.x, lane = tid & 63, col = tid >> 6;
    const int K = a.K;
    double v = 0.0;
    if (col < K || col == TM_CMP_MAX_FITS)
        for (int t = lane; t < a.tiles; t += 64) v += a.part[(size_t)t * TM_CMP_STACK_COLS + (size_t)col];
    v = tmc_wave_sum(v);
    if (lane == 0) sum[col] = v;
    __syncthreads();
    if (tid == 0) {
        double s[TM_CMP_MAX_FITS];
        for (int k = 0; k < TM_CMP_MAX_FITS; k++) s[k] = k < K ? sum[k] : 0.0;
        tmc_em_step(K, a.Np, s, sum[TM_CMP_MAX_FITS], a.tol, a.max_iter, a.state);
    }
}

static bool cmp_args_ok(const TmCmpArgs &a)
{
    return a.K >= 2 && a.K <= TM_CMP_MAX_FITS && a.N >= 1 && a.N <= 0x7FFFFFFFLL && a.elpd && a.tiles == tmc_tiles(a.N);
}

int tm_launch_compare_bootstrap(const TmCmpArgs &a, void *stream)
{
    if (!cmp_args_ok(a) || a.n < 1 || a.n > TM_CMP_CHUNK_MAX || a.Np < 1 || !a.part || !a.z) return (int)hipErrorInvalidValue;
    const long long groups = (tmc_slots(a.g0, a.n) + TM_CMP_PAIRS - 1) / TM_CMP_PAIRS;
    if (groups > 65535 || groups * a.tiles * TM_CMP_THREADS > ((long long)1 << 31)) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tamcmc_compare_bootstrap_kernel, dim3((unsigned)a.tiles, (unsigned)groups), dim3(TM_CMP_THREADS), 0, st, a);
    const long long threads = (long long)a.n * (a.K - 1);
    hipLaunchKernelGGL(tamcmc_compare_finish_kernel, dim3((unsigned)((threads + TM_CMP_THREADS - 1) / TM_CMP_THREADS)), dim3(TM_CMP_THREADS), 0, st, a);
    return (int)hipGetLastError();
}

int tm_launch_compare_variates(const TmCmpArgs &a, unsigned long long g, double *d_e, void *stream)
{
    if (!cmp_args_ok(a) || !d_e) return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((a.N + TM_CMP_THREADS - 1) / TM_CMP_THREADS);
    hipLaunchKernelGGL(tamcmc_compare_variates_kernel, dim3(blocks), dim3(TM_CMP_THREADS), 0, (hipStream_t)stream, a, g, d_e);
    return (int)hipGetLastError();
}

static bool stack_args_ok(const TmCmpStackArgs &a)
{
    return a.K >= 2 && a.K <= TM_CMP_MAX_FITS && a.N >= 1 && a.N <= 0x7FFFFFFFLL && a.Np >= 1 && a.elpd && a.part && a.state &&
           a.tiles == tmc_stack_tiles(a.N) && a.max_iter >= 1;
}

int tm_launch_compare_prepare(const TmCmpStackArgs &a, void *stream)
{
    if (!stack_args_ok(a) || !a.P) return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((a.N + TM_CMP_THREADS - 1) / TM_CMP_THREADS);
    hipLaunchKernelGGL(tamcmc_compare_prepare_kernel, dim3(blocks), dim3(TM_CMP_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_compare_iterations(const TmCmpStackArgs &a, int n, void *stream)
{
    if (!stack_args_ok(a) || n < 1) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    for (int it = 0; it < n; it++) {
        if (a.P) hipLaunchKernelGGL(tamcmc_compare_stack_sums_kernel<true>, dim3((unsigned)a.tiles), dim3(TM_CMP_THREADS), 0, st, a);
        else hipLaunchKernelGGL(tamcmc_compare_stack_sums_kernel<false>, dim3((unsigned)a.tiles), dim3(TM_CMP_THREADS), 0, st, a);
        hipLaunchKernelGGL(tamcmc_compare_stack_update_kernel, dim3(1), dim3(TM_CMP_STACK_COLS * 64), 0, st, a);
    }
    return (int)hipGetLastError();
}
