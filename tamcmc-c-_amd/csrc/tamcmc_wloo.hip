// tamcmc_wloo.hip -- stage 2 of a block of samples while a summary object is in window-LOO mode (tamcmc_wloo.h): PSIS-LOO
// and LOO-PIT with a window of bins left out instead of one bin.  The per-window results come from the finalize kernel of
// tamcmc_loo.hip and the prepare kernel of tamcmc_loopit.hip, launched with n_windows in the place of Nx; what is here forms
// the per-sample window sums and walks them.
//
//   sums    one workgroup per (sample, tile of whole windows), staged through LDS as tamcmc_summary_window_sums_kernel does:
//           the tile's bins of the sample's row are read coalesced (64-bit row offsets), turned into l_is (tms_like) and
//           stored into LDS, every window in a slot of its own of W | 1 doubles; then one thread per window adds its slot up
//           in ascending order (tmw_sum) and writes S_ws to the scratch [sample][window].  In the sub-mode the same LDS is
//           then filled a second time, with tms_resid, and the residual sum goes to the logP plane -- two buffers would not
//           fit into 64 KiB, and the row's second read comes from cache.  A tile starts at a window start and holds
//           min(256, 4096 / W) windows; 34 KiB of LDS.  A sample that is not OK is skipped by its whole workgroup.
//   tail    one thread per window walks the block's samples over the scratch (coalesced over windows, TM_WLOO_UNROLL
//           loads requested before the first is used), skips and counts samples that are not OK and calls tml_top_push with
//           x = -S: the heap [slot][n_windows] and the body sum in registers, as tamcmc_loo_tail_kernel.
//   tails   (sub-mode) one thread per (sample, window), windows fastest: log P and log Q of the residual sum by tmw_chi /
//           tmw_gauss, as tamcmc_summary_window_tails_kernel; log P replaces the sum it was formed from.
//   pit     (sub-mode) one thread per window, samples ONE AT A TIME IN PUSH ORDER over the three scratch planes: x = -S and
//           z; a lane whose sample is of the tail searches its window's sorted column (tlp_find: fixed trip count, every
//           index clamped into the column); then the four sums (tlp_add).  The not-found flag is a plain store of 1.
// No atomics and no cross-lane arithmetic in any per-window state; everything is compiled without FMA contraction.  A
// (sample, window)'s sums and tails depend on nothing but that sample's row, and a window's state on nothing but the order
// of the samples: every result is bit for bit independent of the block size and of how the pass was split over pushes.
#include <hip/hip_runtime.h>
#include <cmath>

#pragma clang fp contract(off)

#include "tamcmc_wloo.h"

// the shape of window w, by selects as tamcmc_window.hip's window_shape (indexing the launch arguments with a lane's value
// would put them into scratch)
static __device__ inline TmWinShape wloo_shape(const TmWlooArgs &a, const int w)
{
    const int kind = tmw_kind(w, a.n_windows);
    const TmWinShape &f = a.shape[0], &m = a.shape[1], &l = a.shape[2];
    TmWinShape s;
    s.len = kind == 0 ? f.len : (kind == 2 ? l.len : m.len);
    s.a = kind == 0 ? f.a : (kind == 2 ? l.a : m.a);
    s.nterms = kind == 0 ? f.nterms : (kind == 2 ? l.nterms : m.nterms);
    s.pad = 0;
    s.lf_am1 = kind == 0 ? f.lf_am1 : (kind == 2 ? l.lf_am1 : m.lf_am1);
    s.lf_a = kind == 0 ? f.lf_a : (kind == 2 ? l.lf_a : m.lf_a);
    s.cq = kind == 0 ? f.cq : (kind == 2 ? l.cq : m.cq);
    s.cp = kind == 0 ? f.cp : (kind == 2 ? l.cp : m.cp);
    s.c = kind == 0 ? f.c : (kind == 2 ? l.c : m.c);
    return s;
}

// grid: nsamp x tiles workgroups, sample s0 + blockIdx.x / tiles, tile blockIdx.x % tiles; wpt windows per tile
template <bool PIT>
__global__ __launch_bounds__(TM_WIN_THREADS) void tamcmc_wloo_sums_kernel(const TmWlooArgs a, const int s0, const int tiles, const int wpt)
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
    const int w = w0 + tid;
    const int len = tid < nw ? (int)(tmw_end(w, a.W, a.first, nx) - tmw_begin(w, a.W, a.first)) : 0;
    const size_t at = (size_t)s * (size_t)a.n_windows + (size_t)w;
#pragma unroll
    for (int pass = 0; pass < (PIT ? 2 : 1); pass++) {
        if (pass) __syncthreads();                            // the first sums have left the slots
        for (int b = tid; b < nb; b += TM_WIN_THREADS) {
            const long long g = b0 + b;
            // window g lies in, counted from the tile's first, and its place there
            const int rest = (int)(g - a.first);
            const int j = rest < 0 ? 0 : 1 + rest / a.W - w0;
            const int i = rest < 0 ? (int)g : rest % a.W;
            const double M = row[g], y = a.y[g];
            q[j * Wp + i] = pass == 0 ? tms_like(gauss, y, M, gauss ? a.isig2[g] : 0.0, a.like_p)
                                      : tms_resid(gauss, y, M, gauss ? sqrt(a.isig2[g]) : 0.0);
        }
        __syncthreads();
        if (tid < nw) {
            const double sum = tmw_sum(q + tid * Wp, len);
            if (pass == 0) a.sum[at] = sum;
            else a.logP[at] = sum;
        }
    }
}

__global__ __launch_bounds__(TM_WLOO_THREADS) void tamcmc_wloo_tail_kernel(const TmWlooArgs a)
{
    const int w = (int)(blockIdx.x * TM_WLOO_THREADS + threadIdx.x);
    if (w >= a.n_windows) return;
    const size_t nw = (size_t)a.n_windows;
    long long n = a.cnt_in[0], rej = a.cnt_in[1];
    double *const heap = a.heap + w;
    double root = n > 0 ? heap[0] : 0.0;
    double ba = a.body[w], br = a.body[nw + w], bc = a.body[2 * nw + w];
    const double *__restrict__ src = a.sum + w;
    for (int s0 = 0; s0 < a.B; s0 += TM_WLOO_UNROLL) {
        double v[TM_WLOO_UNROLL];
#pragma unroll
        for (int k = 0; k < TM_WLOO_UNROLL; k++)
            v[k] = (s0 + k < a.B) ? src[(size_t)(s0 + k) * nw] : 0.0;          // (a rejected sample's word is loaded and dropped)
#pragma unroll
        for (int k = 0; k < TM_WLOO_UNROLL; k++) {
            if (s0 + k >= a.B) break;
            if (a.status[s0 + k] != 0) { rej++; continue; }
            tml_top_push(heap, nw, a.cap, n, -v[k], &root, &ba, &br, &bc);
            n++;
        }
    }

    a.body[w] = ba; a.body[nw + w] = br; a.body[2 * nw + w] = bc;
    if (w == 0) { a.cnt_out[0] = n; a.cnt_out[1] = rej; }
}

// grid: nsamp x n_windows threads from sample s0 on
__global__ __launch_bounds__(TM_WIN_THREADS) void tamcmc_wloo_tails_kernel(const TmWlooArgs a, const int s0, const int nsamp)
{
    const unsigned idx = blockIdx.x * TM_WIN_THREADS + threadIdx.x;
    const unsigned nwin = (unsigned)a.n_windows;
    if (idx / nwin >= (unsigned)nsamp) return;
    const int s = s0 + (int)(idx / nwin), w = (int)(idx % nwin);
    if (a.status[s] != 0) return;
    const size_t at = (size_t)s * (size_t)a.n_windows + (size_t)w;
    const TmWinShape sh = wloo_shape(a, w);
    double lP, lQ;
    if (a.likelihood_case != 0) tmw_gauss(sh, a.logP[at], &lP, &lQ);
    else tmw_chi(sh, a.p, a.logP[at], &lP, &lQ);
    a.logP[at] = lP;
    a.logQ[at] = lQ;
}

__global__ __launch_bounds__(TM_WLOO_THREADS) void tamcmc_wloo_pit_kernel(const TmWlooArgs a)
{
    const int w = (int)(blockIdx.x * TM_WLOO_THREADS + threadIdx.x);
    if (w >= a.n_windows) return;
    const size_t nw = (size_t)a.n_windows;
    int acc = 0, rej = 0;                                      // of this block
    double *__restrict__ st = a.state + w;
    TlpSums sm;
    sm.wa = st[TM_LOOPIT_W_A * nw]; sm.wr = st[TM_LOOPIT_W_R * nw]; sm.wc = st[TM_LOOPIT_W_C * nw];
    sm.aa = st[TM_LOOPIT_A_A * nw]; sm.ar = st[TM_LOOPIT_A_R * nw]; sm.ac = st[TM_LOOPIT_A_C * nw];
    sm.ba = st[TM_LOOPIT_B_A * nw]; sm.br = st[TM_LOOPIT_B_R * nw]; sm.bc = st[TM_LOOPIT_B_C * nw];
    sm.qa = st[TM_LOOPIT_W2_A * nw]; sm.qr = st[TM_LOOPIT_W2_R * nw]; sm.qc = st[TM_LOOPIT_W2_C * nw];
    const double xmax = a.xmax[w], c = a.c[w];                 // c = +inf where there is no tail rule: every sample is body
    const int first = a.first_slot[w];
    const int M = a.cap - 1;
    const double *__restrict__ col = a.heap + w;               // slot k at col[k * nw], sorted ascending over k = 1 ... M
    const double *__restrict__ lwt = a.lw + w;                 // the log weight of slot k at lwt[(k - 1) * nw]
    const double *__restrict__ pS = a.sum + w, *__restrict__ pP = a.logP + w, *__restrict__ pQ = a.logQ + w;
    int missed = 0;

    for (int s0 = 0; s0 < a.B; s0 += TM_WLOO_PIT_UNROLL) {
        double vS[TM_WLOO_PIT_UNROLL], vP[TM_WLOO_PIT_UNROLL], vQ[TM_WLOO_PIT_UNROLL];
#pragma unroll
        for (int k = 0; k < TM_WLOO_PIT_UNROLL; k++) {         // (a rejected sample's words are loaded and dropped)
            const size_t o = (size_t)(s0 + k < a.B ? s0 + k : 0) * nw;
            vS[k] = pS[o]; vP[k] = pP[o]; vQ[k] = pQ[o];
        }
#pragma unroll
        for (int k = 0; k < TM_WLOO_PIT_UNROLL; k++) {
            if (s0 + k >= a.B) break;
            if (a.status[s0 + k] != 0) { rej++; continue; }
            acc++;
            const double xk = -vS[k];
            double lwk = xk - xmax;
            if (lwk > c) {
                bool found;
                const int slot = tlp_find(col, nw, M, a.trips, xk, &found);
                lwk = lwt[(size_t)(slot - 1) * nw];
                missed |= (int)!found | (int)(slot < first);
            }
            tlp_add(&sm, lwk, vP[k], vQ[k]);
        }
    }

    st[TM_LOOPIT_W_A * nw] = sm.wa; st[TM_LOOPIT_W_R * nw] = sm.wr; st[TM_LOOPIT_W_C * nw] = sm.wc;
    st[TM_LOOPIT_A_A * nw] = sm.aa; st[TM_LOOPIT_A_R * nw] = sm.ar; st[TM_LOOPIT_A_C * nw] = sm.ac;
    st[TM_LOOPIT_B_A * nw] = sm.ba; st[TM_LOOPIT_B_R * nw] = sm.br; st[TM_LOOPIT_B_C * nw] = sm.bc;
    st[TM_LOOPIT_W2_A * nw] = sm.qa; st[TM_LOOPIT_W2_R * nw] = sm.qr; st[TM_LOOPIT_W2_C * nw] = sm.qc;
    if (missed) *a.flag = 1;
    if (w == 0) { a.cnt_out[0] = a.cnt_in[0] + acc; a.cnt_out[1] = a.cnt_in[1] + rej; }
}

static bool wloo_args_ok(const TmWlooArgs &a)
{
    if (a.W < 1 || a.W > TM_WIN_MAX_BINS || a.first < 1 || a.first > a.W || a.Nx < 1 || a.B < 1 || a.B > a.Bcap) return false;
    int f = a.first, len[3];
    if (tmw_partition(a.Nx, a.W, &f, len) != (long long)a.n_windows) return false;
    return a.cap >= 2 && a.cap <= TM_LOO_MAX_TAIL + 1;
}

// the sums kernel (and in the sub-mode the tails kernel) over the block, at most 2^23 workgroups of the first and 2^31
// threads of the second per launch
template <bool PIT>
static void wloo_launch_sums(const TmWlooArgs &a, hipStream_t st)
{
    int wpt = TM_WIN_TILE_BINS / a.W;
    wpt = wpt > TM_WIN_THREADS ? TM_WIN_THREADS : wpt;
    const long long tiles = ((long long)a.n_windows + wpt - 1) / wpt;
    long long per = ((long long)1 << 23) / tiles;
    const long long per_t = ((long long)1 << 31) / a.n_windows;
    per = per < per_t ? per : per_t;
    per = per < 1 ? 1 : per;
    for (long long s0 = 0; s0 < a.B; s0 += per) {
        const long long ns = a.B - s0 < per ? a.B - s0 : per;
        hipLaunchKernelGGL(tamcmc_wloo_sums_kernel<PIT>, dim3((unsigned)(ns * tiles)), dim3(TM_WIN_THREADS), 0, st, a, (int)s0, (int)tiles, wpt);
        if (PIT) {
            const unsigned blocks = (unsigned)((ns * a.n_windows + TM_WIN_THREADS - 1) / TM_WIN_THREADS);
            hipLaunchKernelGGL(tamcmc_wloo_tails_kernel, dim3(blocks), dim3(TM_WIN_THREADS), 0, st, a, (int)s0, (int)ns);
        }
    }
}

int tm_launch_wloo_tail(const TmWlooArgs &a, void *stream)
{
    if (!wloo_args_ok(a)) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    wloo_launch_sums<false>(a, st);
    hipLaunchKernelGGL(tamcmc_wloo_tail_kernel, dim3(tms_blocks(a.n_windows, TM_WLOO_THREADS)), dim3(TM_WLOO_THREADS), 0, st, a);
    return (int)hipGetLastError();
}

int tm_launch_wloo_pit(const TmWlooArgs &a, void *stream)
{
    if (!wloo_args_ok(a) || a.trips != tlp_trips(a.cap - 1)) return (int)hipErrorInvalidValue;
    if (a.likelihood_case == 0 && (a.p < 1 || (long long)a.p * a.W > TM_WIN_MAX_SHAPE)) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    wloo_launch_sums<true>(a, st);
    hipLaunchKernelGGL(tamcmc_wloo_pit_kernel, dim3(tms_blocks(a.n_windows, TM_WLOO_THREADS)), dim3(TM_WLOO_THREADS), 0, st, a);
    return (int)hipGetLastError();
}
