// tamcmc_scan.hip -- the sliding-window predictive scan of a summary object (tamcmc_scan.h): behind the window kernels of
// every fold-mode block (where those are on), on the same rows and the same stream, per chunk of the block three kernels.
//
//   sums    one workgroup per (sample, tile of TM_SCAN_TILE positions).  The residuals of the tile's bins and of the halo
//           the widest window of its last position reaches into -- bins [j0, min(j0 + TM_SCAN_TILE + W_{K-1} - 1, Nx)) -- are
//           read coalesced (64-bit row offsets), formed once (tms_resid) and stored into LDS, 20 KiB.  Thread t owns the
//           positions j0 + t, j0 + t + 256, ...: it runs ONE ascending sum from q[j] and stores it for width k when it has
//           added W_k terms -- tmw_sum's additions in tmw_sum's order, for every width.  The widths come from the launch
//           arguments in a uniform loop; neighbouring lanes read neighbouring doubles, so the LDS reads are free of
//           conflicts.  A sample that is not OK is skipped by its whole workgroup; a position with j + W_k > Nx is not written.
//   tails   one thread per (sample, position), positions fastest, the width in blockIdx.y: the shape is uniform over the
//           workgroup and every lane runs the same trip counts.  log P and log Q of the sum by tmw_chi / tmw_gauss.
//   fold    one thread per (width, position): the window fold kernel's walk with (double)W_k for the length, counting on
//           from the pair the block's fold launch read plus the accepted samples of the block's earlier chunks.  The walk
//           is a copy of tamcmc_window.hip's, statement for statement: moved into a shared function it compiled the window
//           fold kernel to other instructions and one more SGPR, and that file's kernels are to stay as measured.
// Sums and tails are not fused: the sums kernel's lane holds eight positions of one sample and all widths, the tails want
// one (width, position) per lane with a uniform shape.
// A (sample, width, position)'s sum and tails depend on nothing but that sample's row, and a position's state on nothing but
// the order of the samples: every result is bit for bit independent of the block size, of the chunks, of how the samples
// were split over pushes and of which other widths are in the list.  Everything is compiled without FMA contraction; no atomics.
#include <hip/hip_runtime.h>
#include <cmath>

#pragma clang fp contract(off)

#include "tamcmc_summary_walk.h"
#include "tamcmc_scan.h"

#define TM_SCAN_UNROLL 4          // as TM_WIN_UNROLL of tamcmc_window.hip

// grid: nsamp x tiles workgroups, sample s0 + blockIdx.x / tiles of the block (slot blockIdx.x / tiles of the chunk)
__global__ __launch_bounds__(TM_SCAN_THREADS) void tamcmc_summary_scan_sums_kernel(const TmScanArgs a, const int s0, const int tiles)
{
    __shared__ double q[TM_SCAN_LDS_DOUBLES];
    const int tid = (int)threadIdx.x;
    const int slot = (int)(blockIdx.x / (unsigned)tiles);
    const int s = s0 + slot;
    if (a.status[s] != 0) return;                             // the whole workgroup: nobody reads this sample's scratch
    const long long nx = a.Nx;
    const long long j0 = (long long)(blockIdx.x % (unsigned)tiles) * TM_SCAN_TILE;
    int wmax = a.W[0];
#pragma unroll
    for (int k = 1; k < TM_SCAN_MAX_WIDTHS; k++) wmax = k < a.K ? a.W[k] : wmax;
    const long long e = j0 + TM_SCAN_TILE + wmax - 1;
    const int nb = (int)((e < nx ? e : nx) - j0);             // <= TM_SCAN_LDS_DOUBLES
    const bool gauss = a.likelihood_case != 0;
    const double *__restrict__ row = a.rows + (size_t)s * (size_t)nx;
    for (int b = tid; b < nb; b += TM_SCAN_THREADS) {
        const long long g = j0 + b;
        const double M = row[g], y = a.y[g];
        q[b] = tms_resid(gauss, y, M, gauss ? sqrt(a.isig2[g]) : 0.0);
    }
    __syncthreads();
    double *__restrict__ out = a.scratch + 2 * (size_t)a.C * (size_t)a.total + (size_t)slot * (size_t)a.total;
    for (int t = tid; t < TM_SCAN_TILE; t += TM_SCAN_THREADS) {
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
            out[(size_t)a.off[k] + (size_t)j] = sum;
        }
    }
}

// grid: x over nsamp x n_pos_k threads from sample s0 on, y = the width
__global__ __launch_bounds__(TM_SCAN_THREADS) void tamcmc_summary_scan_tails_kernel(const TmScanArgs a, const int s0, const int nsamp)
{
    const int k = (int)blockIdx.y;
    // width k's launch arguments: k is uniform over the workgroup, so these are scalar loads from the argument segment at
    // an offset held in a scalar register (indexing with a lane's value would put the arguments into scratch)
    const TmWinShape sh = a.shape[k];
    const long long off = a.off[k];
    const unsigned long long npos = (unsigned long long)(a.Nx - sh.len + 1);
    const unsigned long long idx = (unsigned long long)blockIdx.x * TM_SCAN_THREADS + threadIdx.x;
    if (idx / npos >= (unsigned long long)nsamp) return;
    const int slot = (int)(idx / npos);
    if (a.status[s0 + slot] != 0) return;
    const size_t plane = (size_t)a.C * (size_t)a.total;
    double *__restrict__ at = a.scratch + (size_t)slot * (size_t)a.total + (size_t)off + (size_t)(idx % npos);
    double lP, lQ;
    if (a.likelihood_case != 0) tmw_gauss(sh, at[2 * plane], &lP, &lQ);
    else tmw_chi(sh, a.p, at[2 * plane], &lP, &lQ);
    at[0] = lP;
    at[plane] = lQ;
}

// the chunk's samples are s0 ... s0 + nsamp - 1 of the block
__global__ __launch_bounds__(TM_SCAN_THREADS) void tamcmc_summary_scan_fold_kernel(const TmScanArgs a, const int s0, const int nsamp)
{
    const long long g = (long long)blockIdx.x * TM_SCAN_THREADS + threadIdx.x;
    if (g >= a.total) return;
    int W = a.W[0];
#pragma unroll
    for (int k = 1; k < TM_SCAN_MAX_WIDTHS; k++) W = k < a.K && g >= a.off[k] ? a.W[k] : W;
    long long n = a.cnt_in[0];
    for (int i = 0; i < s0; i++) n += a.status[i] == 0 ? 1 : 0;              // the block's earlier chunks (uniform)
    const size_t total = (size_t)a.total, plane = (size_t)a.C * total;
    double *__restrict__ st = a.state + g;
    double ca = st[TM_PRED_CDF_A * total], cr = st[TM_PRED_CDF_R * total], cc = st[TM_PRED_CDF_C * total];
    double sa = st[TM_PRED_SF_A * total], sr = st[TM_PRED_SF_R * total], sc = st[TM_PRED_SF_C * total];
    double mean = st[TM_PRED_MEAN_RESID * total];
    const double dlen = (double)W;
    const double *__restrict__ src = a.scratch + g;
    const int32_t *__restrict__ status = a.status + s0;

    for (int c0 = 0; c0 < nsamp; c0 += TM_SCAN_UNROLL) {
        double vP[TM_SCAN_UNROLL], vQ[TM_SCAN_UNROLL], vS[TM_SCAN_UNROLL];
#pragma unroll
        for (int k = 0; k < TM_SCAN_UNROLL; k++) {            // (a rejected sample's words are loaded and dropped)
            const bool in = c0 + k < nsamp;
            const size_t o = (size_t)(in ? c0 + k : 0) * total;
            vP[k] = src[o]; vQ[k] = src[plane + o]; vS[k] = src[2 * plane + o];
        }
#pragma unroll
        for (int k = 0; k < TM_SCAN_UNROLL; k++) {
            if (c0 + k >= nsamp) break;
            if (status[c0 + k] != 0) continue;
            n++;
            tmp_lse_step(&ca, &cr, &cc, vP[k]);
            tmp_lse_step(&sa, &sr, &sc, vQ[k]);
            mean += (vS[k] / dlen - mean) / (double)n;
        }
    }

    st[TM_PRED_CDF_A * total] = ca; st[TM_PRED_CDF_R * total] = cr; st[TM_PRED_CDF_C * total] = cc;
    st[TM_PRED_SF_A * total] = sa; st[TM_PRED_SF_R * total] = sr; st[TM_PRED_SF_C * total] = sc;
    st[TM_PRED_MEAN_RESID * total] = mean;
}

int tm_launch_scan(const TmScanArgs &a, void *stream)
{
    if (a.K < 1 || a.K > TM_SCAN_MAX_WIDTHS || a.B < 1 || a.C < 1 || a.total < 1) return (int)hipErrorInvalidValue;
    long long total = 0;
    for (int k = 0; k < a.K; k++) {
        if (a.W[k] < 1 || a.W[k] > TM_WIN_MAX_BINS || a.W[k] > a.Nx || (k > 0 && a.W[k] <= a.W[k - 1]) || a.off[k] != total ||
            a.shape[k].len != a.W[k])
            return (int)hipErrorInvalidValue;
        if (a.likelihood_case == 0 && (a.p < 1 || (long long)a.p * a.W[k] > TM_WIN_MAX_SHAPE)) return (int)hipErrorInvalidValue;
        total += tmsc_positions(a.Nx, a.W[k]);
    }
    if (total != a.total) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const long long npos0 = tmsc_positions(a.Nx, a.W[0]);     // the narrowest width has the most positions
    const long long tiles = (npos0 + TM_SCAN_TILE - 1) / TM_SCAN_TILE;
    // samples per launch: the chunk, and at most 2^30 threads of the sums and the tails kernel
    long long per = ((long long)1 << 30) / (tiles * TM_SCAN_THREADS);
    const long long per_t = ((long long)1 << 30) / npos0;
    per = per < per_t ? per : per_t;
    per = per < a.C ? per : a.C;
    per = per < 1 ? 1 : per;
    for (long long s0 = 0; s0 < a.B; s0 += per) {
        const long long ns = a.B - s0 < per ? a.B - s0 : per;
        hipLaunchKernelGGL(tamcmc_summary_scan_sums_kernel, dim3((unsigned)(ns * tiles)), dim3(TM_SCAN_THREADS), 0, st, a, (int)s0, (int)tiles);
        const unsigned blocks = (unsigned)((ns * npos0 + TM_SCAN_THREADS - 1) / TM_SCAN_THREADS);
        hipLaunchKernelGGL(tamcmc_summary_scan_tails_kernel, dim3(blocks, (unsigned)a.K), dim3(TM_SCAN_THREADS), 0, st, a, (int)s0, (int)ns);
        hipLaunchKernelGGL(tamcmc_summary_scan_fold_kernel, dim3(tms_blocks(a.total, TM_SCAN_THREADS)), dim3(TM_SCAN_THREADS), 0, st, a, (int)s0, (int)ns);
    }
    return (int)hipGetLastError();
}
