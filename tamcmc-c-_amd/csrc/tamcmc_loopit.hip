// tamcmc_loopit.hip -- the leave-one-out PIT of a summary object in LOO mode (tamcmc_loopit.h): the kernel that turns a
// complete LOO pass into a table of log weights, and stage 2 of a block of the third pass.
//
// Prepare kernel.  One wave per bin, shaped like the finalize kernel of tamcmc_loo.hip and built from its parts: the bin's
// heap column goes into LDS and is sorted by the same bitonic network (tml_load_sorted), tml_finalize runs once more and
// leaves the tail's log weights zt_(j) in its work array -- the same code on the same values as the finalize kernel, so
// the weights are those behind elpd_loo -- and the lanes then write, with stride 64: the sorted values back into heap slots
// 1 ... ncand, the log weight of every slot (tlp_tie_lw: equal values share the mean weight of their ranks), and per bin
// xmax, c and the first tail slot.  LDS as the finalize kernel: 2 x 16 KiB + 1.2 KiB.
//
// PIT kernel.  One thread owns one bin and walks the block's rows as the tail kernel does: rows are read coalesced with
// 64-bit row offsets, TM_LOOPIT_UNROLL loads requested before the first is used (past the block the last row is read again
// and dropped); the status words come from device memory and a sample that is not OK is skipped and counted.  The samples
// of a group are then taken one at a time, in push order, in a loop that is NOT unrolled -- unrolled, it is
// TM_LOOPIT_UNROLL copies of every transcendental of l, of the predictive tails and of the four recurrences: sample k is
// read from slot 0 and the rest move down a slot.  Per sample: x = -l and z; a lane whose sample is of the tail (z > c)
// searches its bin's sorted column (tlp_find: the trip count is the launch's, no branch inside, every index clamped into
// the column) while the other lanes wait, and a wave without such a lane skips the search; then the two predictive tails
// (tamcmc_predictive.h) and the four sums (tlp_add).  Advancing the searches of a group's samples together, so that
// TM_LOOPIT_UNROLL loads are in flight per lane, was measured and is slower.
// No LDS, no atomics, no cross-lane arithmetic: a bin's state is bit for bit independent of the block size and of how the
// pass was split over pushes.  The not-found flag is a plain store of 1.
#include <hip/hip_runtime.h>
#include <cmath>

#pragma clang fp contract(off)

#include "tamcmc_loopit.h"
#include "tamcmc_summary_walk.h"

__global__ __launch_bounds__(TM_LOO_THREADS) void tamcmc_loopit_prepare_kernel(const TmLooPitArgs a)
{
    __shared__ double s[TM_LOO_MAX_TAIL], t[TM_LOO_MAX_TAIL];
    __shared__ double theta[TM_LOO_MAX_THETA], ell[TM_LOO_MAX_THETA];
    const int bin = (int)blockIdx.x, lane = (int)threadIdx.x;
    const size_t nx = (size_t)a.Nx;
    const int cnt = a.n < (long long)a.cap ? (int)a.n : a.cap;               // >= 1
    const int ncand = cnt - 1;                                               // <= cap - 1 <= TM_LOO_MAX_TAIL
    const bool has_rule = a.n >= (long long)a.cap;
    double *heap = a.heap + bin;
    const double root = heap[0];
    tml_load_sorted(heap, nx, ncand, s);
    TmlWave w;
    const TmlBin r = tml_finalize(w, s, ncand, root, has_rule, a.n, a.body[bin], a.body[nx + bin] - a.body[2 * nx + bin], t, theta, ell);
    w.sync();
    const int L = (int)r.tail_len, nb = ncand - L;
    const double xmax = ncand > 0 ? s[ncand - 1] : root;
    for (int j = lane; j < ncand; j += TM_LOO_THREADS) {
        heap[(size_t)(j + 1) * nx] = s[j];
        a.lw[(size_t)j * nx + bin] = j < nb ? s[j] - xmax : tlp_tie_lw(s + nb, t, L, j - nb);
    }
    if (lane == 0) {
        a.xmax[bin] = xmax;
        a.c[bin] = has_rule ? fmax(root - xmax, log(DBL_MIN)) : (double)INFINITY;
        a.first[bin] = L > 0 ? nb + 1 : a.cap;
    }
}

__global__ __launch_bounds__(TM_LOOPIT_THREADS) void tamcmc_loopit_kernel(const TmLooPitArgs a)
{
    const int bin = (int)(blockIdx.x * TM_LOOPIT_THREADS + threadIdx.x);
    if (bin >= a.Nx) return;
    const size_t nx = (size_t)a.Nx;
    int acc = 0, rej = 0;                                      // of this block
    double *__restrict__ st = a.state + bin;
    TlpSums sm;
    sm.wa = st[TM_LOOPIT_W_A * nx]; sm.wr = st[TM_LOOPIT_W_R * nx]; sm.wc = st[TM_LOOPIT_W_C * nx];
    sm.aa = st[TM_LOOPIT_A_A * nx]; sm.ar = st[TM_LOOPIT_A_R * nx]; sm.ac = st[TM_LOOPIT_A_C * nx];
    sm.ba = st[TM_LOOPIT_B_A * nx]; sm.br = st[TM_LOOPIT_B_R * nx]; sm.bc = st[TM_LOOPIT_B_C * nx];
    sm.qa = st[TM_LOOPIT_W2_A * nx]; sm.qr = st[TM_LOOPIT_W2_R * nx]; sm.qc = st[TM_LOOPIT_W2_C * nx];
    const TmsBinLike lk(a, bin);
    const double y = lk.y;
    const bool gauss = lk.chi_square;
    const double isig = gauss ? sqrt(lk.isig2) : 0.0;
    const int p = a.p;
    const double dp = (double)p;
    const double xmax = a.xmax[bin], c = a.c[bin];             // c = +inf where there is no tail rule: every sample is body
    const int first = a.first[bin];
    const int M = a.cap - 1;
    const double *__restrict__ col = a.heap + bin;             // slot k at col[k * nx], sorted ascending over k = 1 ... M
    const double *__restrict__ lwt = a.lw + bin;               // the log weight of slot k at lwt[(k - 1) * nx]
    const double *__restrict__ rows = a.rows + bin;
    int missed = 0;

    for (int s0 = 0; s0 < a.B; s0 += TM_LOOPIT_UNROLL) {
        double v[TM_LOOPIT_UNROLL];
#pragma unroll
        for (int k = 0; k < TM_LOOPIT_UNROLL; k++)
            v[k] = rows[(size_t)(s0 + k < a.B ? s0 + k : a.B - 1) * nx];   // (a rejected sample's row is loaded and dropped)
#pragma unroll 1
        for (int k = 0; k < TM_LOOPIT_UNROLL && s0 + k < a.B; k++) {
            const double vk = v[0];
#pragma unroll
            for (int j = 0; j + 1 < TM_LOOPIT_UNROLL; j++) v[j] = v[j + 1];
            if (a.status[s0 + k] != 0) { rej++; continue; }
            acc++;
            const double xk = -lk.l(vk);
            double lwk = xk - xmax;
            if (lwk > c) {
                bool found;
                const int slot = tlp_find(col, nx, M, a.trips, xk, &found);
                lwk = lwt[(size_t)(slot - 1) * nx];
                missed |= (int)!found | (int)(slot < first);
            }
            double lP, lQ;
            if (gauss) tmp_gauss(tms_resid(true, y, vk, isig), &lP, &lQ);
            else if (p == 1) tmp_chi_p1(tms_resid(false, y, vk, isig), &lP, &lQ);
            else tmp_chi_p(p, a.lf_pm1, a.lf_p, a.nterms, dp * y / vk, &lP, &lQ);
            tlp_add(&sm, lwk, lP, lQ);
        }
    }

    st[TM_LOOPIT_W_A * nx] = sm.wa; st[TM_LOOPIT_W_R * nx] = sm.wr; st[TM_LOOPIT_W_C * nx] = sm.wc;
    st[TM_LOOPIT_A_A * nx] = sm.aa; st[TM_LOOPIT_A_R * nx] = sm.ar; st[TM_LOOPIT_A_C * nx] = sm.ac;
    st[TM_LOOPIT_B_A * nx] = sm.ba; st[TM_LOOPIT_B_R * nx] = sm.br; st[TM_LOOPIT_B_C * nx] = sm.bc;
    st[TM_LOOPIT_W2_A * nx] = sm.qa; st[TM_LOOPIT_W2_R * nx] = sm.qr; st[TM_LOOPIT_W2_C * nx] = sm.qc;
    if (missed) *a.flag = 1;
    if (bin == 0) { a.cnt_out[0] = a.cnt_in[0] + acc; a.cnt_out[1] = a.cnt_in[1] + rej; }
}

static bool loopit_args_ok(const TmLooPitArgs &a)
{
    if (a.cap < 2 || a.cap > TM_LOO_MAX_TAIL + 1 || a.n < 1 || a.Nx < 1) return false;
    if (a.likelihood_case == 0 && (a.p < 1 || a.p > TM_PRED_MAX_P)) return false;
    return a.trips == tlp_trips(a.cap - 1);
}

int tm_launch_loopit_prepare(const TmLooPitArgs &a, void *stream)
{
    if (!loopit_args_ok(a)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_loopit_prepare_kernel, dim3((unsigned)a.Nx), dim3(TM_LOO_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_loopit(const TmLooPitArgs &a, void *stream)
{
    if (!loopit_args_ok(a) || a.B < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_loopit_kernel, dim3(tms_blocks(a.Nx, TM_LOOPIT_THREADS)), dim3(TM_LOOPIT_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
