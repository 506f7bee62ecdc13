// tamcmc_window.hip -- the windowed posterior predictive check of a summary object (tamcmc_window.h): behind the fold
// kernel of every fold-mode block (and behind the predictive kernel where that is on), on the same rows and the same
// stream, three kernels.
//
//   sums    one workgroup per (sample, tile of whole windows).  The tile's bins of the sample's row are read coalesced
//           (64-bit row offsets), turned into q_i = y_i / M_is (chi(2,2p)) or r_i = (y_i - M_is) sqrt(isig2_i)
//           (chi_square: tms_resid) and stored into LDS, every window in a slot of its own of W | 1 doubles; then one thread per
//           window adds its slot up in ascending order.  A tile starts at a window start and holds min(256, 4096 / W)
//           windows, so no window straddles two tiles; 34 KiB of LDS.  The odd slot stride puts the 32 lanes of a
//           half-wave on 32 different bank pairs.  A sample that is not OK is skipped by its whole workgroup.
//   tails   one thread per (sample, window), windows fastest: log P and log Q of the sum by tmw_chi / tmw_gauss.  Every
//           lane of a wave is busy whatever W is -- at W = 512 a tile of the sums kernel holds 8 windows, and evaluating
//           the tails there would run the 510-step loop of tmp_chi_p on 8 lanes of 256.  All full windows share one
//           shape, so the loops' trip counts are wave-uniform except in waves that hold window 0 or the last window; the
//           loop itself is tmp_chi_p's, one select per step.
//   fold    one thread per window, shaped like tamcmc_summary_predictive_kernel: it loads the window's seven state
//           words, walks the block's samples ONE AT A TIME IN PUSH ORDER over the scratch (coalesced over windows),
//           skips samples that are not OK (wave-uniform) and stores the state back, counting on from the pair the
//           block's fold launch read.  No atomics, no cross-lane work.
// A (sample, window)'s sum and tails depend on nothing but that sample's row, and a window's state on nothing but the
// order of the samples: every result is bit for bit independent of the block size and of how the samples were split
// over pushes.  Everything is compiled without FMA contraction.
#include <hip/hip_runtime.h>
#include <cmath>

#pragma clang fp contract(off)

#include "tamcmc_summary_walk.h"
#include "tamcmc_window.h"

#define TM_WIN_UNROLL 4           // samples whose three scratch words the fold kernel requests before it uses the first

// the shape of window w, by selects: indexing the launch arguments with a lane's value would put them into scratch
static __device__ inline TmWinShape window_shape(const TmWinArgs &a, const int w)
{
    const int kind = tmw_kind(w, a.n_windows);
    TmWinShape s;
    s.len = kind == 0 ? a.shape[0].len : (kind == 2 ? a.shape[2].len : a.shape[1].len);
    s.a = kind == 0 ? a.shape[0].a : (kind == 2 ? a.shape[2].a : a.shape[1].a);
    s.nterms = kind == 0 ? a.shape[0].nterms : (kind == 2 ? a.shape[2].nterms : a.shape[1].nterms);
    s.pad = 0;
    s.lf_am1 = kind == 0 ? a.shape[0].lf_am1 : (kind == 2 ? a.shape[2].lf_am1 : a.shape[1].lf_am1);
    s.lf_a = kind == 0 ? a.shape[0].lf_a : (kind == 2 ? a.shape[2].lf_a : a.shape[1].lf_a);
    s.cq = kind == 0 ? a.shape[0].cq : (kind == 2 ? a.shape[2].cq : a.shape[1].cq);
    s.cp = kind == 0 ? a.shape[0].cp : (kind == 2 ? a.shape[2].cp : a.shape[1].cp);
    s.c = kind == 0 ? a.shape[0].c : (kind == 2 ? a.shape[2].c : a.shape[1].c);
    return s;
}

// grid: nsamp x tiles workgroups, sample s0 + blockIdx.x / tiles, tile blockIdx.x % tiles; wpt windows per tile
__global__ __launch_bounds__(TM_WIN_THREADS) void tamcmc_summary_window_sums_kernel(const TmWinArgs a, const int s0, const int tiles, const int wpt)
{
    __shared__ double q[TM_WIN_LDS_DOUBLES];
    const int tid = (int)threadIdx.x;
    const int s = s0 + (int)(blockIdx.x / (unsigned)tiles);
    if (a.status[s] != 0) return;                             // the whole workgroup: nobody reads this sample's scratch
    const int w0 = (int)(blockIdx.x % (unsigned)tiles) * wpt;
    const int nw = a.n_windows - w0 < wpt ? a.n_windows - w0 : wpt;
    const long long nx = a.Nx;
    const long long b0 = tmw_begin(w0, a.W, a.first);
    const int nb = (int)(tmw_end(w0 + nw - 1, a.W, a.first, nx) - b0);     // <= wpt * W <= TM_WIN_TILE_BINS
    const int Wp = a.W | 1;
    const bool gauss = a.likelihood_case != 0;
    const double *__restrict__ row = a.rows + (size_t)s * (size_t)nx;
    for (int b = tid; b < nb; b += TM_WIN_THREADS) {
        const long long g = b0 + b;
        // window g lies in, counted from the tile's first, and its place there
        const int rest = (int)(g - a.first);
        const int j = rest < 0 ? 0 : 1 + rest / a.W - w0;
        const int i = rest < 0 ? (int)g : rest % a.W;
        const double M = row[g], y = a.y[g];
        q[j * Wp + i] = tms_resid(gauss, y, M, gauss ? sqrt(a.isig2[g]) : 0.0);
    }
    __syncthreads();
    if (tid >= nw) return;
    const int w = w0 + tid;
    const int len = (int)(tmw_end(w, a.W, a.first, nx) - tmw_begin(w, a.W, a.first));
    const size_t plane = (size_t)a.Bcap * (size_t)a.n_windows;
    a.scratch[2 * plane + (size_t)s * (size_t)a.n_windows + (size_t)w] = tmw_sum(q + tid * Wp, len);
}

// grid: nsamp x n_windows threads from sample s0 on
__global__ __launch_bounds__(TM_WIN_THREADS) void tamcmc_summary_window_tails_kernel(const TmWinArgs a, const int s0, const int nsamp)
{
    const unsigned idx = blockIdx.x * TM_WIN_THREADS + threadIdx.x;
    const unsigned nwin = (unsigned)a.n_windows;
    if (idx / nwin >= (unsigned)nsamp) return;
    const int s = s0 + (int)(idx / nwin), w = (int)(idx % nwin);
    if (a.status[s] != 0) return;
    const size_t plane = (size_t)a.Bcap * (size_t)a.n_windows;
    double *__restrict__ at = a.scratch + (size_t)s * (size_t)a.n_windows + (size_t)w;
    const TmWinShape sh = window_shape(a, w);
    double lP, lQ;
    if (a.likelihood_case != 0) tmw_gauss(sh, at[2 * plane], &lP, &lQ);
    else tmw_chi(sh, a.p, at[2 * plane], &lP, &lQ);
    at[0] = lP;
    at[plane] = lQ;
}

__global__ __launch_bounds__(TM_WIN_THREADS) void tamcmc_summary_window_fold_kernel(const TmWinArgs a)
{
    const int w = (int)(blockIdx.x * TM_WIN_THREADS + threadIdx.x);
    if (w >= a.n_windows) return;
    const size_t nwin = (size_t)a.n_windows, plane = (size_t)a.Bcap * nwin;
    long long n = a.cnt_in[0];
    double *__restrict__ st = a.state + w;
    double ca = st[TM_PRED_CDF_A * nwin], cr = st[TM_PRED_CDF_R * nwin], cc = st[TM_PRED_CDF_C * nwin];
    double sa = st[TM_PRED_SF_A * nwin], sr = st[TM_PRED_SF_R * nwin], sc = st[TM_PRED_SF_C * nwin];
    double mean = st[TM_PRED_MEAN_RESID * nwin];
    const double dlen = (double)(tmw_end(w, a.W, a.first, a.Nx) - tmw_begin(w, a.W, a.first));
    const double *__restrict__ src = a.scratch + w;

    for (int s0 = 0; s0 < a.B; s0 += TM_WIN_UNROLL) {
        double vP[TM_WIN_UNROLL], vQ[TM_WIN_UNROLL], vS[TM_WIN_UNROLL];
#pragma unroll
        for (int k = 0; k < TM_WIN_UNROLL; k++) {             // (a rejected sample's words are loaded and dropped)
            const bool in = s0 + k < a.B;
            const size_t o = (size_t)(in ? s0 + k : 0) * nwin;
            vP[k] = src[o]; vQ[k] = src[plane + o]; vS[k] = src[2 * plane + o];
        }
#pragma unroll
        for (int k = 0; k < TM_WIN_UNROLL; k++) {
            if (s0 + k >= a.B) break;
            if (a.status[s0 + k] != 0) continue;
            n++;
            tmp_lse_step(&ca, &cr, &cc, vP[k]);
            tmp_lse_step(&sa, &sr, &sc, vQ[k]);
            mean += (vS[k] / dlen - mean) / (double)n;
        }
    }

    st[TM_PRED_CDF_A * nwin] = ca; st[TM_PRED_CDF_R * nwin] = cr; st[TM_PRED_CDF_C * nwin] = cc;
    st[TM_PRED_SF_A * nwin] = sa; st[TM_PRED_SF_R * nwin] = sr; st[TM_PRED_SF_C * nwin] = sc;
    st[TM_PRED_MEAN_RESID * nwin] = mean;
}

int tm_launch_window(const TmWinArgs &a, void *stream)
{
    if (a.W < 1 || a.W > TM_WIN_MAX_BINS || a.first < 1 || a.first > a.W || a.n_windows < 1 || a.B < 1 || a.B > a.Bcap) return (int)hipErrorInvalidValue;
    if (a.likelihood_case == 0 && (a.p < 1 || (long long)a.p * a.W > TM_WIN_MAX_SHAPE)) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    int wpt = TM_WIN_TILE_BINS / a.W;
    wpt = wpt > TM_WIN_THREADS ? TM_WIN_THREADS : wpt;
    const long long tiles = ((long long)a.n_windows + wpt - 1) / wpt;
    // samples per launch: at most 2^23 workgroups of the sums kernel and 2^31 threads of the tails kernel
    long long per = ((long long)1 << 23) / tiles;
    const long long per_t = ((long long)1 << 31) / a.n_windows;
    per = per < per_t ? per : per_t;
    per = per < 1 ? 1 : per;
    for (long long s0 = 0; s0 < a.B; s0 += per) {
        const long long ns = a.B - s0 < per ? a.B - s0 : per;
        hipLaunchKernelGGL(tamcmc_summary_window_sums_kernel, dim3((unsigned)(ns * tiles)), dim3(TM_WIN_THREADS), 0, st, a, (int)s0, (int)tiles, wpt);
        const unsigned blocks = (unsigned)((ns * a.n_windows + TM_WIN_THREADS - 1) / TM_WIN_THREADS);
        hipLaunchKernelGGL(tamcmc_summary_window_tails_kernel, dim3(blocks), dim3(TM_WIN_THREADS), 0, st, a, (int)s0, (int)ns);
    }
    hipLaunchKernelGGL(tamcmc_summary_window_fold_kernel, dim3(tms_blocks(a.n_windows, TM_WIN_THREADS)), dim3(TM_WIN_THREADS), 0, st, a);
    return (int)hipGetLastError();
}
