// tamcmc_modediag.hip -- the kernels behind tamcmc_modediag_* (tamcmc_modediag.h): lag products, their finish, and the sums
// of products between columns, all on the mode table's stored rows (column-major, a column contiguous in t, columns
// max_samples doubles apart).  fp64 VALU throughout; no MFMA (it would add several t at a time, in an order the definition
// does not allow), no atomics, no sum split over threads.
//
//   lag      one wave per (column, block of 256 lags), lane i owning 4 consecutive lags with their accumulators in registers.
//            The column is read coalesced along t, centred on the fly and staged in LDS in tiles of 1024 samples behind the
//            1024 values before them; the next tile's values are requested before the current tile is walked.  Within a tile
//            d_t is one LDS address for the whole wave and a lane's past values are 4 doubles from its neighbour's
//            (tmd_lag_tile).  16 KiB of LDS.
//   finish   one thread per column: the Welford moments of the two halves of the CENTRED values d_t, walked together (two
//            independent recurrences, 8 loads of each in flight), tme_rhat, and tme_finish on the column's lag products.
//            R-hat does not change when a constant is taken off the series, and Welford's mean update rounds at the size of
//            the mean: on d_t that is the column's spread, on v_t it would be the column's value (a frequency is hundreds
//            of standard deviations).  No LDS.
//   cov      256 threads per pair of 32-column strips of the upper triangle, a thread owning 2 x 2 pairs: four independent
//            fma chains fed by two 16-byte LDS reads per sample.  The strips are staged t-major in stages of 64 samples, read
//            coalesced along t (a wave takes 64 consecutive samples of one column), the next stage requested before the
//            current one is walked.  (i, j) and (j, i) are stored from the same register.  34 KiB of LDS.
#include <hip/hip_runtime.h>
#include <cmath>

// no FMA contraction anywhere in this file: the only fused operations are the ones written out (tme_acc, tmd_cov_acc)
#pragma clang fp contract(off)

#include "tamcmc_ess.h"
#include "tamcmc_modediag.h"

__global__ __launch_bounds__(TM_MD_LANES) void tamcmc_modediag_lag_kernel(const TmMdArgs a)
{
    __shared__ double s_d[TM_MD_HALO + TM_MD_TILE];
    constexpr int PER = TM_MD_TILE / TM_MD_LANES;
    const int col = blockIdx.x, lane = threadIdx.x;
    if (col >= a.n_cols) return;
    const int k0 = (int)blockIdx.y * TM_MD_BLOCK_LAGS + lane * TM_MD_G;
    const int ng = a.L + 1 - k0 < TM_MD_G ? a.L + 1 - k0 : TM_MD_G;          // (<= 0: the lane only helps staging)
    const double *__restrict__ v = a.table + (size_t)col * (size_t)a.max_samples;
    const double mean = a.mean[col];
    double A[TM_MD_G], pre[PER];
#pragma unroll
    for (int j = 0; j < TM_MD_G; j++) A[j] = 0.0;
    for (int j = lane; j < TM_MD_HALO; j += TM_MD_LANES) s_d[j] = 0.0;
    // the tile at t0 into registers: sample t0 + r * 64 + lane in pre[r]
    auto fetch = [&](const long long t0) {
#pragma unroll
        for (int r = 0; r < PER; r++) {
            const long long t = t0 + r * TM_MD_LANES + lane;
            pre[r] = t < a.n ? v[t] : 0.0;
        }
    };
    fetch(0);
    for (long long t0 = 0; t0 < a.n; t0 += TM_MD_TILE) {
        const int m = tmd_tile_len(a.n, t0);
        __syncthreads();                                                     // the tile before this one has been walked
        if (t0 > 0) {
            double keep[TM_MD_HALO / TM_MD_LANES];
#pragma unroll
            for (int r = 0; r < TM_MD_HALO / TM_MD_LANES; r++) keep[r] = s_d[tmd_halo_src(r * TM_MD_LANES + lane)];
            __syncthreads();
#pragma unroll
            for (int r = 0; r < TM_MD_HALO / TM_MD_LANES; r++) s_d[r * TM_MD_LANES + lane] = keep[r];
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < PER; r++)
            if (r * TM_MD_LANES + lane < m) s_d[TM_MD_HALO + r * TM_MD_LANES + lane] = tmd_centre(pre[r], mean);
        __syncthreads();
        if (t0 + TM_MD_TILE < a.n) fetch(t0 + TM_MD_TILE);                   // in flight while this tile is walked
        if (ng > 0) tmd_lag_tile<TM_MD_G>(s_d + TM_MD_HALO, t0, m, k0, ng, A);
    }
#pragma unroll
    for (int j = 0; j < TM_MD_G; j++)
        if (j < ng) a.acc[(size_t)(k0 + j) * (size_t)a.n_cols + col] = A[j];
}

__global__ __launch_bounds__(TM_MD_FIN_THREADS) void tamcmc_modediag_finish_kernel(const TmMdArgs a)
{
    const int col = (int)(blockIdx.x * TM_MD_FIN_THREADS + threadIdx.x);
    if (col >= a.n_cols) return;
    const size_t nc = (size_t)a.n_cols;
    const long long h = a.n / 2;
    const double *__restrict__ v1 = a.table + (size_t)col * (size_t)a.max_samples, *__restrict__ v2 = v1 + (a.n - h);
    const double mean = a.mean[col];
    double m1 = 0.0, q1 = 0.0, m2 = 0.0, q2 = 0.0;
    for (long long i0 = 0; i0 < h; i0 += TM_MD_FIN_UNROLL) {
        double x1[TM_MD_FIN_UNROLL], x2[TM_MD_FIN_UNROLL];
#pragma unroll
        for (int u = 0; u < TM_MD_FIN_UNROLL; u++) {
            const long long i = i0 + u < h ? i0 + u : h - 1;                  // (past the half: its last value again, not taken)
            x1[u] = tmd_centre(v1[i], mean);
            x2[u] = tmd_centre(v2[i], mean);
        }
#pragma unroll
        for (int u = 0; u < TM_MD_FIN_UNROLL; u++) {
            if (i0 + u >= h) break;
            tme_welford(&m1, &q1, i0 + u + 1, x1[u]);
            tme_welford(&m2, &q2, i0 + u + 1, x2[u]);
        }
    }
    const TmeFinish f = tme_finish(a.acc + col, nc, a.L, (double)a.n, a.tau_floor);
    a.fin[TM_MD_TAU * nc + col] = f.tau;
    a.fin[TM_MD_ESS * nc + col] = f.ess;
    a.fin[TM_MD_RHAT * nc + col] = tme_rhat(m1, q1, m2, q2, h);
    a.cut[col] = f.cut;
}

__global__ __launch_bounds__(TM_MD_CTHREADS) void tamcmc_modediag_cov_kernel(const TmMdCovArgs a)
{
    __shared__ __attribute__((aligned(16))) double s_a[TM_MD_CS][TM_MD_CROW], s_b[TM_MD_CS][TM_MD_CROW];
    constexpr int WAVES = TM_MD_CTHREADS / 64, PER = TM_MD_CT / WAVES;       // a wave stages PER columns of either strip
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = tid >> 4, tx = tid & 15;
    int bi, bj;
    tmd_tile_pair((int)blockIdx.x, tmd_cov_strips(a.n_sel), &bi, &bj);
    const int i0 = bi * TM_MD_CT + 2 * ty, j0 = bj * TM_MD_CT + 2 * tx;      // the thread's pairs: (i0, i0 + 1) x (j0, j0 + 1)
    // the columns this thread stages: column wave + WAVES r of either strip (-1 past the selection), sample `lane` of a stage
    int ca[PER], cb[PER];
    double ma[PER], mb[PER], pa[PER], pb[PER];
#pragma unroll
    for (int r = 0; r < PER; r++) {
        const int ci = bi * TM_MD_CT + wave + WAVES * r, cj = bj * TM_MD_CT + wave + WAVES * r;
        ca[r] = ci < a.n_sel ? a.sel[ci] : -1;
        cb[r] = cj < a.n_sel ? a.sel[cj] : -1;
        ma[r] = ca[r] >= 0 ? a.mean[ca[r]] : 0.0;
        mb[r] = cb[r] >= 0 ? a.mean[cb[r]] : 0.0;
    }
    // sample t of those columns into pa / pb (what is not there: the mean, which centres to +0.0)
#define TM_MD_COV_FETCH(t_)                                                                                       \
    _Pragma("unroll") for (int r = 0; r < PER; r++) {                                                             \
        pa[r] = (ca[r] >= 0 && (t_) < a.n) ? a.table[(size_t)ca[r] * (size_t)a.max_samples + (size_t)(t_)] : ma[r]; \
        pb[r] = (cb[r] >= 0 && (t_) < a.n) ? a.table[(size_t)cb[r] * (size_t)a.max_samples + (size_t)(t_)] : mb[r]; \
    }
    double S00 = 0.0, S01 = 0.0, S10 = 0.0, S11 = 0.0;
    TM_MD_COV_FETCH((long long)lane)
    for (long long t0 = 0; t0 < a.n; t0 += TM_MD_CS) {
        const int m = a.n - t0 < TM_MD_CS ? (int)(a.n - t0) : TM_MD_CS;
        __syncthreads();                                                     // the stage before this one has been walked
#pragma unroll
        for (int r = 0; r < PER; r++) {
            s_a[lane][wave + WAVES * r] = tmd_centre(pa[r], ma[r]);
            s_b[lane][wave + WAVES * r] = tmd_centre(pb[r], mb[r]);
        }
        __syncthreads();
        if (t0 + TM_MD_CS < a.n) { TM_MD_COV_FETCH(t0 + TM_MD_CS + lane) }   // in flight while this stage is walked
#pragma unroll 8
        for (int s = 0; s < m; s++) {
            const double x0 = s_a[s][2 * ty], x1 = s_a[s][2 * ty + 1], y0 = s_b[s][2 * tx], y1 = s_b[s][2 * tx + 1];
            S00 = tmd_cov_acc(S00, x0, y0);
            S01 = tmd_cov_acc(S01, x0, y1);
            S10 = tmd_cov_acc(S10, x1, y0);
            S11 = tmd_cov_acc(S11, x1, y1);
        }
    }
    const size_t ns = (size_t)a.n_sel;
    if (tmd_cov_owns(i0, j0, a.n_sel)) { a.S[(size_t)i0 * ns + j0] = S00; a.S[(size_t)j0 * ns + i0] = S00; }
    if (tmd_cov_owns(i0, j0 + 1, a.n_sel)) { a.S[(size_t)i0 * ns + j0 + 1] = S01; a.S[(size_t)(j0 + 1) * ns + i0] = S01; }
    if (tmd_cov_owns(i0 + 1, j0, a.n_sel)) { a.S[(size_t)(i0 + 1) * ns + j0] = S10; a.S[(size_t)j0 * ns + i0 + 1] = S10; }
    if (tmd_cov_owns(i0 + 1, j0 + 1, a.n_sel)) { a.S[(size_t)(i0 + 1) * ns + j0 + 1] = S11; a.S[(size_t)(j0 + 1) * ns + i0 + 1] = S11; }
}

static bool md_args_ok(const TmMdArgs &a)
{
    return a.n_cols >= 1 && a.L >= 1 && a.L <= TM_MD_MAX_LAG && (a.L & 1) == 1 && a.n >= 4 && a.L <= a.n - 1 && a.n <= a.max_samples;
}

int tm_launch_modediag_lag(const TmMdArgs &a, void *stream)
{
    if (!md_args_ok(a)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)a.n_cols, (unsigned)tmd_lag_blocks(a.L));
    hipLaunchKernelGGL(tamcmc_modediag_lag_kernel, grid, dim3(TM_MD_LANES), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_modediag_finish(const TmMdArgs &a, void *stream)
{
    if (!md_args_ok(a)) return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((a.n_cols + TM_MD_FIN_THREADS - 1) / TM_MD_FIN_THREADS);
    hipLaunchKernelGGL(tamcmc_modediag_finish_kernel, dim3(blocks), dim3(TM_MD_FIN_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_modediag_cov(const TmMdCovArgs &a, void *stream)
{
    if (a.n_sel < 1 || a.n_sel > TM_MD_MAX_COLS || a.n_sel > a.n_cols || a.n < 2 || a.n > a.max_samples) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_modediag_cov_kernel, dim3((unsigned)tmd_cov_blocks(a.n_sel)), dim3(TM_MD_CTHREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
