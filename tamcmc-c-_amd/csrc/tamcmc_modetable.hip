// tamcmc_modetable.hip -- the kernels of the posterior mode table (tamcmc_modetable.h).
//
//   derive     one wave per sample.  The params row goes into LDS; lane 0 derives the chain's scalars, the whole wave the
//              inclination and the m-ratio tables (tm_derive_chain_tables shuffles), then lane j derives multiplet j
//              (j + 64, ... for chains with more than 64, up to TM_MAXMULT) with tm_derive_mult and writes its columns.
//              These are the device functions of tamcmc_derive.h that the setup and backward kernels call, compiled here
//              as there without floating-point contraction: the window indices come out of the same non-fused operations.
//              Status: the maximum of the multiplets' status (an empty window: TAMCMC_CHAIN_EMPTY_WINDOW), else
//              TAMCMC_CHAIN_NAN when any column is a NaN or the square of a width is infinite (an AppWidth exponent out of
//              range, Gamma = exp(364): every column is finite, but the setup kernel's Gamma^2 is not and the eval kernels'
//              Lorentzian is inf / inf).
//   fold       one thread per column walks the block's accepted samples in push order: Welford mean and sum of squared
//              deviations, minimum, maximum (tm_mt_fold_one), and appends the value to the column-major table.  Nothing
//              is shared between threads, so no result bit depends on the block size or on how the samples were pushed.
//   quantiles  one workgroup per column: the radix selection of tamcmc_modetable.h on the keys of tamcmc_quantile.h,
//              TM_MT_QBITS bits per pass, a 256-cell histogram per rank in LDS (32-bit counters: a column holds fewer than
//              2^31 samples, no flush), thread q narrows rank q between two passes.  The value stored is the order
//              statistic itself.
#include <hip/hip_runtime.h>
#include <cmath>

#pragma clang fp contract(off)      // the derivation's window arithmetic and the fold's recurrences: never fused
#include "tamcmc_modetable.h"
#include "tamcmc_derive.h"

__global__ __launch_bounds__(TM_MT_THREADS) void tamcmc_modetable_derive_kernel(const TmMtDeriveArgs a)
{
    extern __shared__ double s_p[];          // this sample's params row
    __shared__ TmChain C;
    __shared__ int s_status[2];              // maximum of the multiplets' status; any column a NaN or a width^2 infinite
    const TmLayout &L = a.L;
    const int lane = threadIdx.x, sample = blockIdx.x;
    if (sample >= a.B) return;
    for (int e = lane; e < L.Nparams; e += TM_MT_THREADS) s_p[e] = a.params[(size_t)sample * L.Nparams + e];
    if (lane < 2) s_status[lane] = 0;
    __syncthreads();
    const double *p = s_p;
    if (lane == 0) tm_derive_chain_scalars(L, p, C);
    __syncthreads();
    tm_derive_chain_tables(L, p, C, lane);   // the whole wave
    __syncthreads();

    double *row = a.rows + (size_t)sample * (size_t)a.n_cols;
    int st = 0;
    bool nan = false;
    if (lane == 0) {
        const double inc = tm_chain_inc(L, p);
        row[TM_MT_INCLINATION] = inc; row[TM_MT_ETA] = C.eta; row[TM_MT_A3] = C.a3; row[TM_MT_ASYMMETRY] = C.asym;
        nan = !(inc == inc) || !(C.eta == C.eta) || !(C.a3 == C.a3) || !(C.asym == C.asym);
    }
    for (int j = lane; j < L.n_mult; j += TM_MT_THREADS) {
        TmMultFull M;                        // in registers: every array index inside is a compile-time constant
        tm_derive_mult(L, C, p, j, M);
        double *o = row + tm_mt_mult_first(L, j);
        double height = 0.0;
#pragma unroll
        for (int k = 0; k < TM_MAXM; k++)
            if (k < M.ncomp) height = height + M.h[k];
        const double amp = sqrt((3.141592653589793 * height) * M.W);
        const double split = (M.l == 0) ? 0.0 : M.f_s;
        o[0] = M.f; o[1] = M.W; o[2] = height; o[3] = amp; o[4] = split;
        o[5] = (double)M.imin; o[6] = (double)M.imax;
        nan = nan || !(M.f == M.f) || !(M.W == M.W) || !(height == height) || !(amp == amp) || !(split == split);
        nan = nan || M.W * M.W == __builtin_inf();     // the g2 of the setup kernel
#pragma unroll
        for (int k = 0; k < TM_MAXM; k++) {
            if (k < M.ncomp) {
                o[TM_MT_MULT_FIXED + k] = M.nu[k];
                o[TM_MT_MULT_FIXED + M.ncomp + k] = M.h[k];
                nan = nan || !(M.nu[k] == M.nu[k]) || !(M.h[k] == M.h[k]);
            }
        }
        st = M.status > st ? M.status : st;
    }
    if (st != 0) atomicMax(&s_status[0], st);
    if (nan) atomicMax(&s_status[1], 1);
    __syncthreads();
    if (lane == 0) a.status[sample] = s_status[0] != 0 ? s_status[0] : s_status[1];   // s_status[1]: 1 = TAMCMC_CHAIN_NAN
}

__global__ __launch_bounds__(TM_MT_FOLD_THREADS) void tamcmc_modetable_fold_kernel(const TmMtFoldArgs a)
{
    const int col = (int)(blockIdx.x * TM_MT_FOLD_THREADS + threadIdx.x);
    if (col >= a.n_cols) return;
    const size_t nc = (size_t)a.n_cols;
    double *__restrict__ st = a.state + col;
    double mean = st[TM_MT_MEAN * nc], M2 = st[TM_MT_M2 * nc], mn = st[TM_MT_MIN * nc], mx = st[TM_MT_MAX * nc];
    double *__restrict__ tab = a.table ? a.table + (size_t)col * (size_t)a.max_samples : nullptr;
    long long n = a.n_before;
    // TM_MT_FOLD_UNROLL samples are requested before the first of them is folded: the recurrence is serial, the loads are not
    for (int k0 = 0; k0 < a.B; k0 += TM_MT_FOLD_UNROLL) {
        double v[TM_MT_FOLD_UNROLL];
        int take[TM_MT_FOLD_UNROLL];
#pragma unroll
        for (int i = 0; i < TM_MT_FOLD_UNROLL; i++) {
            const int k = k0 + i < a.B ? k0 + i : a.B - 1;      // (a sample past the block: the last one again, not taken)
            take[i] = k0 + i < a.B ? a.accept[k] : 0;
            v[i] = a.rows[(size_t)k * nc + col];
        }
#pragma unroll
        for (int i = 0; i < TM_MT_FOLD_UNROLL; i++) {
            if (take[i] == 0) continue;
            n++;
            tm_mt_fold_one(mean, M2, mn, mx, n, v[i]);
            if (tab != nullptr && n <= a.max_samples) tab[n - 1] = v[i];
        }
    }
    st[TM_MT_MEAN * nc] = mean; st[TM_MT_M2 * nc] = M2; st[TM_MT_MIN * nc] = mn; st[TM_MT_MAX * nc] = mx;
}

__global__ __launch_bounds__(TM_MT_QTHREADS) void tamcmc_modetable_quantile_kernel(const TmMtQuantArgs a)
{
    __shared__ uint32_t s_hist[TM_Q_MAXQ][1 << TM_MT_QBITS];
    __shared__ uint64_t s_prefix[TM_Q_MAXQ], s_below[TM_Q_MAXQ], s_rank[TM_Q_MAXQ];
    const int col = blockIdx.x, tid = threadIdx.x;
    if (col >= a.n_cols) return;
    const size_t nc = (size_t)a.n_cols;
    const double *__restrict__ v = a.table + (size_t)col * (size_t)a.max_samples;
    const uint64_t kmin = tmq_key(a.state[TM_MT_MIN * nc + col]), R = tmq_key(a.state[TM_MT_MAX * nc + col]) - kmin;
    for (int i = tid; i < TM_Q_MAXQ << TM_MT_QBITS; i += TM_MT_QTHREADS) (&s_hist[0][0])[i] = 0;
    if (tid < TM_Q_MAXQ) { s_prefix[tid] = 0; s_below[tid] = 0; s_rank[tid] = tid < a.Nq ? a.ranks[tid] : 0; }
    __syncthreads();
    for (int u = tmq_bit_length(R); u > 0;) {                  // (workgroup-uniform)
        const int d = tmq_digits(u, TM_MT_QBITS);
        uint64_t pre[TM_Q_MAXQ];
#pragma unroll
        for (int q = 0; q < TM_Q_MAXQ; q++) pre[q] = s_prefix[q];
        for (long long i = tid; i < a.n; i += TM_MT_QTHREADS) {
            const uint64_t D = tmq_key(v[i]) - kmin;
#pragma unroll
            for (int q = 0; q < TM_Q_MAXQ; q++) {
                unsigned cell;
                if (q < a.Nq && tmq_match(D, pre[q], u, d, &cell)) atomicAdd(&s_hist[q][cell], 1u);
            }
        }
        __syncthreads();
        if (tid < a.Nq) tmq_narrow(&s_prefix[tid], &s_below[tid], s_rank[tid], &s_hist[tid][0], 1, d);
        __syncthreads();
        u -= d;
    }
    if (tid < a.Nq) a.out[(size_t)tid * nc + col] = tmq_unkey(kmin + s_prefix[tid]);
}

int tm_launch_modetable_derive(const TmMtDeriveArgs &a, size_t lds_bytes, void *stream)
{
    hipLaunchKernelGGL(tamcmc_modetable_derive_kernel, dim3(a.B), dim3(TM_MT_THREADS), lds_bytes, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_modetable_fold(const TmMtFoldArgs &a, void *stream)
{
    const unsigned blocks = (unsigned)((a.n_cols + TM_MT_FOLD_THREADS - 1) / TM_MT_FOLD_THREADS);
    hipLaunchKernelGGL(tamcmc_modetable_fold_kernel, dim3(blocks), dim3(TM_MT_FOLD_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_modetable_quantiles(const TmMtQuantArgs &a, void *stream)
{
    hipLaunchKernelGGL(tamcmc_modetable_quantile_kernel, dim3(a.n_cols), dim3(TM_MT_QTHREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
