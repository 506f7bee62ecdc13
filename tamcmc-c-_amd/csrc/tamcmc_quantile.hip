// tamcmc_quantile.hip -- stage 2 of a block of samples while a summary object selects quantiles (tamcmc_quantile.h): count
// the block's model rows into per-bin histograms of the next few key bits, and, between passes, narrow every bracket.
//
// Histogram kernel.  One thread owns one bin and walks the block's rows as the fold kernel does (tms_walk,
// tamcmc_summary_walk.h, TM_Q_UNROLL loads in flight).  A workgroup is one wave.  The block's counts go into 16-bit LDS
// counters laid out [quantile][cell][thread]: a thread only ever touches its own column, so there is no barrier, no atomic
// and no bank conflict (64 threads x 2 bytes = 32 consecutive banks, two threads per word).  The sample loop is cut into
// runs of TM_Q_RUN = 65535 samples, each followed by a flush, so a counter cannot wrap.  A flush adds the thread's column
// into the global uint32 histogram [Nq][2^bits][Nx]: coalesced over the wave, owner-only read-modify-write, cells the run
// left at zero are not touched.  No per-sample update goes to global memory.
// LDS: Nq x 2^bits columns of 128 bytes, at most 8 x 64 x 128 = 64 KiB; the kernel is instantiated for 64, 128, 256 and
// 512 columns (8 ... 64 KiB) and the launch picks the smallest that holds Nq << bits, for the sake of occupancy.
//
// A sample outside the envelope (D > R: the caller pushed rows other than the fold pass's) sets a flag word with a plain
// store -- every writer stores the same value.  {accepted, rejected} are counted as the fold kernel counts them.
//
// Narrow and init kernels: one thread per bin, a loop over the quantiles.
#include <hip/hip_runtime.h>

#include "tamcmc_quantile.h"
#include "tamcmc_summary.h"

template <int COLS>
__global__ __launch_bounds__(TM_Q_THREADS) void tamcmc_quantile_hist_kernel(const TmQuantArgs a)
{
    __shared__ uint16_t lds[COLS * TM_Q_THREADS];
    const int bin = (int)(blockIdx.x * TM_Q_THREADS + threadIdx.x);
    if (bin >= a.Nx) return;
    const size_t nx = (size_t)a.Nx;
    const int u = (int)a.u[bin];
    const int d = tmq_digits(u, a.bits);
    const int ncell = 1 << a.bits, used = 1 << d;
    const uint64_t kmin = a.kmin[bin], R = a.R[bin];
    uint64_t prefix[TM_Q_MAXQ];
#pragma unroll
    for (int j = 0; j < TM_Q_MAXQ; j++) prefix[j] = j < a.Nq ? a.prefix[(size_t)j * nx + bin] : (uint64_t)0;
    TmsCount cnt{a.cnt_in[0], a.cnt_in[1]};
    bool outside = false;
    uint16_t *const col = lds + threadIdx.x;
    uint32_t *const hist = a.hist + bin;

    for (long long r0 = 0; r0 < (long long)a.B; r0 += TM_Q_RUN) {
        const int b0 = (int)r0, b1 = a.B - b0 > TM_Q_RUN ? b0 + TM_Q_RUN : a.B;
        if (u > 0)
            for (int j = 0; j < a.Nq; j++)
                for (int c = 0; c < used; c++) col[(j * ncell + c) * TM_Q_THREADS] = 0;
        cnt = tms_walk<TM_Q_UNROLL>(a.rows + bin, a.status, b0, b1, nx, cnt, [&](const double v, long long) {
            const uint64_t D = tmq_key(v) - kmin;
            if (D > R) { outside = true; return; }
            if (u == 0) return;
#pragma unroll
            for (int j = 0; j < TM_Q_MAXQ; j++) {
                unsigned cell;
                if (j < a.Nq && tmq_match(D, prefix[j], u, d, &cell)) col[(j * ncell + (int)cell) * TM_Q_THREADS]++;
            }
        });
        if (u > 0)
            for (int j = 0; j < a.Nq; j++)
                for (int c = 0; c < used; c++) {
                    const uint32_t m = col[(j * ncell + c) * TM_Q_THREADS];
                    if (m) hist[(size_t)(j * ncell + c) * nx] += m;
                }
    }
    if (outside) *a.flag = 1u;
    if (bin == 0) { a.cnt_out[0] = cnt.n; a.cnt_out[1] = cnt.rej; }
}

__global__ __launch_bounds__(TM_Q_NARROW_THREADS) void tamcmc_quantile_narrow_kernel(const TmQuantArgs a)
{
    const int bin = (int)(blockIdx.x * TM_Q_NARROW_THREADS + threadIdx.x);
    if (bin >= a.Nx) return;
    const size_t nx = (size_t)a.Nx;
    const int u = (int)a.u[bin];
    if (u == 0) return;
    const int d = tmq_digits(u, a.bits);
    const int ncell = 1 << a.bits;
    for (int j = 0; j < a.Nq; j++) {
        uint64_t p = a.prefix[(size_t)j * nx + bin], b = a.below[(size_t)j * nx + bin];
        tmq_narrow(&p, &b, a.ranks[j], a.hist + (size_t)(j * ncell) * nx + bin, nx, d);
        a.prefix[(size_t)j * nx + bin] = p;
        a.below[(size_t)j * nx + bin] = b;
    }
    a.u[bin] = (uint32_t)(u - d);
}

__global__ __launch_bounds__(TM_Q_NARROW_THREADS) void tamcmc_quantile_init_kernel(const TmQuantArgs a)
{
    const int bin = (int)(blockIdx.x * TM_Q_NARROW_THREADS + threadIdx.x);
    if (bin >= a.Nx) return;
    const size_t nx = (size_t)a.Nx;
    const uint64_t kmin = tmq_key(a.fold_state[TM_SUM_MIN_M * nx + bin]);
    const uint64_t R = tmq_key(a.fold_state[TM_SUM_MAX_M * nx + bin]) - kmin;
    a.kmin[bin] = kmin;
    a.R[bin] = R;
    a.u[bin] = (uint32_t)tmq_bit_length(R);
    for (int j = 0; j < a.Nq; j++) {
        a.prefix[(size_t)j * nx + bin] = 0;
        a.below[(size_t)j * nx + bin] = 0;
    }
}

int tm_launch_quantile_init(const TmQuantArgs &a, void *stream)
{
    hipLaunchKernelGGL(tamcmc_quantile_init_kernel, dim3(tms_blocks(a.Nx, TM_Q_NARROW_THREADS)), dim3(TM_Q_NARROW_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_quantile_narrow(const TmQuantArgs &a, void *stream)
{
    hipLaunchKernelGGL(tamcmc_quantile_narrow_kernel, dim3(tms_blocks(a.Nx, TM_Q_NARROW_THREADS)), dim3(TM_Q_NARROW_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_quantile_hist(const TmQuantArgs &a, void *stream)
{
    if (a.Nq < 1 || a.Nq > TM_Q_MAXQ || a.bits < 1 || a.bits > TM_Q_MAXBITS) return (int)hipErrorInvalidValue;
    const int cols = a.Nq << a.bits;
    const dim3 grid(tms_blocks(a.Nx, TM_Q_THREADS)), block(TM_Q_THREADS);
    if (cols <= 64) hipLaunchKernelGGL(tamcmc_quantile_hist_kernel<64>, grid, block, 0, (hipStream_t)stream, a);
    else if (cols <= 128) hipLaunchKernelGGL(tamcmc_quantile_hist_kernel<128>, grid, block, 0, (hipStream_t)stream, a);
    else if (cols <= 256) hipLaunchKernelGGL(tamcmc_quantile_hist_kernel<256>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(tamcmc_quantile_hist_kernel<512>, grid, block, 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
