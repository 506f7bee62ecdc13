// tamcmc_summary_api.cpp -- posterior summaries of a stored chain (tamcmc_accel.h, tamcmc_summary.h): per-bin running
// statistics of the model and of the pointwise log-likelihood over the samples pushed so far.  A block of samples = the
// context's own launches (tamcmc_host.h: tm_enqueue) with a row map covering every chain (stage 1) +
// tamcmc_summary_fold_kernel (stage 2), both on the context's stream.  While the object selects quantiles
// (tamcmc_summary_quantiles_*, tamcmc_quantile.h) stage 2 is the histogram kernel instead and the fold state is frozen;
// in LOO mode (tamcmc_summary_loo_*, tamcmc_loo.h) it is the tail kernel, and after tamcmc_summary_loo_pit_begin the PIT
// kernel (tamcmc_loopit.h).  With the predictive check enabled
// (tamcmc_summary_predictive_*, tamcmc_predictive.h) a fold-mode block has a stage 3: tamcmc_summary_predictive_kernel on
// the same rows; the other two modes never touch its state.  With the windowed check enabled (tamcmc_summary_window_*,
// tamcmc_window.h) a stage 4 follows: the sums, tails and fold kernels of tamcmc_window.hip, again on the same rows.
// With the sliding-window scan enabled (tamcmc_summary_scan_*, tamcmc_scan.h) a stage 5 follows: the sums, tails and fold
// kernels of tamcmc_scan.hip per chunk of the block, on the same rows.
// In ESS mode (tamcmc_summary_ess_*, tamcmc_ess.h) stage 2 is the centre and lag kernels of tamcmc_ess.hip, once per chunk of
// the block; in band ESS mode (tamcmc_summary_bandess_*, tamcmc_bandess.h) the pack and lag kernels of tamcmc_bandess.hip, likewise.
// In window-LOO mode (tamcmc_summary_wloo_*, tamcmc_wloo.h) stage 2 is the sums and tail kernels of tamcmc_wloo.hip, and after
// tamcmc_summary_wloo_pit_begin its sums, tails and PIT kernels; the per-window results come from LOO mode's finalize and
// prepare kernels.
#include <algorithm>
#include <cmath>
#include <new>

#include "tamcmc_bandess.h"
#include "tamcmc_ess.h"
#include "tamcmc_host.h"
#include "tamcmc_loo.h"
#include "tamcmc_loopit.h"
#include "tamcmc_predictive.h"
#include "tamcmc_quantile.h"
#include "tamcmc_scan.h"
#include "tamcmc_summary.h"
#include "tamcmc_window.h"
#include "tamcmc_wloo.h"

// {accepted, rejected} of a pass on the device, [2][2] words: launch k reads pair k & 1 and writes the other, so no
// workgroup reads a word that another workgroup of the same launch writes (TmSummaryArgs::cnt_in / cnt_out).  read(): idle stream.
struct TmCountPair {
    long long *d = nullptr;
    int parity = 0;
    const long long *in() const { return d + 2 * parity; }
    long long *out() const { return d + 2 * (parity ^ 1); }
    void flip() { parity ^= 1; }         // after a launch that wrote out()
    int clear(hipStream_t stream) { TM_HIP(hipMemsetAsync(d, 0, 4 * sizeof(long long), stream)); parity = 0; return TAMCMC_OK; }
    int read(long long cnt[2]) const { TM_HIP(hipMemcpy(cnt, in(), 2 * sizeof(long long), hipMemcpyDeviceToHost)); return TAMCMC_OK; }
};

// What the three modes share: the counts of the fold pass, frozen by _begin, and those of the mode's pass under way.
struct TmMode {
    bool on = false;
    long long n_used = 0, n_rejected = 0;
    TmCountPair cnt;
};

// Quantile mode: the selection's state on the device and what the host remembers of it.
struct TmQuantMode : TmMode {
    int Nq = 0, bits = 0, passes = 0;
    int u0max = 0;                       // the largest number of unresolved bits over the bins, before the first step
    int64_t ranks[TM_Q_MAXQ] = {};
    char *d_state = nullptr;             // one allocation: kmin | R | prefix | below | ranks | cnt[2][2] | u | flag
    uint32_t *d_hist = nullptr;          // [Nq][2^bits][Nx]
    size_t hist_bytes = 0;
    uint64_t *kmin = nullptr, *R = nullptr, *prefix = nullptr, *below = nullptr, *d_ranks = nullptr;
    uint32_t *u = nullptr, *flag = nullptr;
};

// LOO mode: the top sets and the body sums of the pass on the device, and what the host remembers of the fold pass.
struct TmLooMode : TmMode {
    int cap = 0;                         // M + 1 heap slots per bin
    double *d_heap = nullptr;            // [cap][Nx]
    char *d_state = nullptr;             // one allocation: body[3][Nx] | elpd | khat | cutoff | cnt[2][2] | tail_len
    double *body = nullptr, *elpd = nullptr, *khat = nullptr, *cutoff = nullptr;
    int32_t *tail_len = nullptr;
    // the LOO-PIT sub-mode (tamcmc_loopit.h): its pass's counts, the table of log weights and the rest of its state
    bool pit = false;
    TmCountPair pit_cnt;
    double *d_lw = nullptr;              // [cap - 1][Nx]
    char *d_pit = nullptr;               // one allocation: sums[TM_LOOPIT_NSTATE][Nx] | xmax | c | cnt[2][2] | first | flag
    double *pit_sums = nullptr, *pit_xmax = nullptr, *pit_c = nullptr;
    int32_t *pit_first = nullptr, *pit_flag = nullptr;
    int p = 1, nterms = 0;               // as TmPredictive
    double lf_pm1 = 0.0, lf_p = 0.0;
};

// Window-LOO mode (tamcmc_wloo.h): LOO mode and its sub-mode over the windows of the windowed check.  The heap, body, results
// and the sub-mode's state are laid out as TmLooMode's with n_windows in the place of Nx.
struct TmWlooMode : TmMode {
    int W = 0, first = 0, n_windows = 0;
    int cap = 0;                         // M + 1 heap slots per window
    double *d_heap = nullptr;            // [cap][n_windows]
    char *d_state = nullptr;             // one allocation: body[3][nw] | elpd | khat | cutoff | cnt[2][2] | tail_len
    double *d_sum = nullptr;             // [B][n_windows]: the window sums of l of the block in flight
    double *body = nullptr, *elpd = nullptr, *khat = nullptr, *cutoff = nullptr;
    int32_t *tail_len = nullptr;
    bool pit = false;
    TmCountPair pit_cnt;
    double *d_lw = nullptr;              // [cap - 1][n_windows]
    char *d_pit = nullptr;               // one allocation: sums[TM_LOOPIT_NSTATE][nw] | xmax | c | cnt[2][2] | first slot | flag
    double *d_tails = nullptr;           // [2][B][n_windows]: logP (the residual sum before the tails kernel) | logQ
    double *pit_sums = nullptr, *pit_xmax = nullptr, *pit_c = nullptr;
    int32_t *pit_first = nullptr, *pit_flag = nullptr;
    int p = 1;
    TmWinShape shape[3] = {};            // first window, full windows, last window
};

// ESS mode: the lag products, the rings of centred values and the half-chain moments of the pass on the device, and what the
// host remembers of the fold pass.
struct TmEssMode : TmMode {
    int L = 0, R = 0;
    double *d_acc = nullptr;             // [2][L + 1][Nx]
    double *d_ring = nullptr;            // [2][R][Nx]
    char *d_state = nullptr;             // one allocation: half[4][Nx] | lppd | tau[2][Nx] | ess[2][Nx] | cnt[2][2] | cut[2][Nx]
    double *half = nullptr, *lppd = nullptr, *tau = nullptr, *ess = nullptr;
    int32_t *cut = nullptr;
};

// Band ESS mode: the thresholds, the bit-packed series (ring and head), the integer lag counts and the results of the pass
// on the device, and what the host remembers of the fold pass.
struct TmBandMode : TmMode {
    int K = 0, L = 0, RW = 0, HW = 0;
    uint32_t *d_C = nullptr;             // [K][L + 1][Nx]
    uint64_t *d_bits = nullptr;          // one allocation: ring[K][RW][Nx] | head[K][HW][Nx]
    uint64_t *head = nullptr;
    void *d_work = nullptr;              // [L + 1][Nx] of 8 bytes: the finish kernel's A_k or E_k of one threshold
    char *d_state = nullptr;             // one allocation: thr[K][Nx] | tau[K][Nx] | ess[K][Nx] | cnt[2][2] | cut[K][Nx]
    double *thr = nullptr, *tau = nullptr, *ess = nullptr;
    int32_t *cut = nullptr;
};

// The predictive check: a setting of the object (on from _enable until destroy), not a mode.
struct TmPredictive {
    bool on = false;
    double *d_state = nullptr;           // [TM_PRED_NSTATE][Nx]
    int p = 1, nterms = 0;               // chi(2,2p): (int)like_p and tmp_series_terms(p)
    double lf_pm1 = 0.0, lf_p = 0.0;     // log (p-1)!, log p!
    TmTimer timer;                       // the predictive kernel alone (tamcmc_summary_predictive_kernel_time)
};

// The windowed predictive check: a setting like TmPredictive, and independent of it.
struct TmWindow {
    bool on = false;
    double *d_state = nullptr;           // [TM_PRED_NSTATE][n_windows]
    double *d_scratch = nullptr;         // [3][B][n_windows]
    int W = 0, first = 0, n_windows = 0, p = 1;
    TmWinShape shape[3] = {};            // first window, full windows, last window
    TmTimer timer;                       // the three window kernels of a block together (tamcmc_summary_window_kernel_time)
};

// The sliding-window scan: a setting like TmWindow, and independent of it and of TmPredictive.
struct TmScan {
    bool on = false;
    double *d_state = nullptr;           // [TM_PRED_NSTATE][total]
    double *d_scratch = nullptr;         // [3][C][total]
    int K = 0, C = 0, p = 1;
    long long total = 0;                 // sum_k n_pos_k
    int32_t W[TM_SCAN_MAX_WIDTHS] = {};
    long long off[TM_SCAN_MAX_WIDTHS] = {};
    TmWinShape shape[TM_SCAN_MAX_WIDTHS] = {};
    TmTimer timer;                       // the scan kernels of a block together (tamcmc_summary_scan_kernel_time)
};

struct tamcmc_summary {
    tamcmc_ctx *c = nullptr;
    int B = 0;                           // samples per block
    bool counted = false;                // the context's count includes this object
    double *d_model = nullptr;           // [B][Nx] model rows of the block in flight (the context's d_model is not touched)
    double *d_state = nullptr;           // [TM_SUM_NSTATE][Nx]
    TmCountPair cnt;                     // of the fold pass
    int32_t *d_rows = nullptr;           // [B] the identity row map
    double *d_T = nullptr;               // [B] ones: samples are evaluated at temperature 1
    double *d_logL = nullptr;            // [B] / [B]: where a block's logL / status go when the caller wants none
    int32_t *d_status = nullptr;
    // host-pointer pushes: [params | logL | status] of a block, pinned and on the device, two of each (block k fills
    // slot k & 1 while block k - 1 may still be read by its copies)
    TmPinned stage[2];
    hipEvent_t ev_stage[2] = {nullptr, nullptr};
    // timing of the fold kernel alone (tamcmc_summary_profile)
    bool profile = false;
    TmTimer timer;
    TmQuantMode q;
    TmLooMode loo;
    TmTimer pit_timer;                   // the LOO-PIT kernel alone (tamcmc_summary_loo_pit_kernel_time)
    TmWlooMode wloo;
    TmTimer wpit_timer;                  // the blocks of window-LOO's PIT pass (tamcmc_summary_wloo_pit_kernel_time)
    TmEssMode ess;
    TmBandMode band;
    TmPredictive pred;
    TmWindow win;
    TmScan scan;
};

static size_t summary_stage_out(const tamcmc_summary *s) { return (size_t)s->B * (size_t)s->c->L.Nparams * sizeof(double); }
static size_t summary_stage_bytes(const tamcmc_summary *s) { return summary_stage_out(s) + (size_t)s->B * (sizeof(double) + sizeof(int32_t)); }

// what every push refuses (the context's state may have changed since the object was created)
static int summary_check(const tamcmc_summary *s, int32_t Nsamples, int32_t Nparams, const double *params)
{
    if (!s || !params || Nsamples < 1) return TAMCMC_E_INVALID;
    const tamcmc_ctx *c = s->c;
    if (Nparams != c->L.Nparams || c->in_flight || c->armed || c->nspec > 1) return TAMCMC_E_INVALID;
    return TAMCMC_OK;
}

// What most entry points open with: no object, or a context whose stream cannot be waited for, is refused; then the stream
// is idle.  (_create and _reset settle without waiting; _destroy and the _kernel_time functions have their own preludes.)
// fold_cnt: where the fold pass's counts go, read from the device, for the callers that want them.
static int summary_enter(tamcmc_summary *s, long long *fold_cnt = nullptr)
{
    if (!s || s->c->in_flight || s->c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(s->c->device));
    TM_HIP(tm_ctx_stream_sync(s->c));
    return fold_cnt ? s->cnt.read(fold_cnt) : TAMCMC_OK;
}

// the mode the object is in (at most one), or NULL in fold mode
static const TmMode *active_mode(const tamcmc_summary *s)
{
    if (s->q.on) return &s->q;
    if (s->loo.on) return &s->loo;
    if (s->ess.on) return &s->ess;
    if (s->wloo.on) return &s->wloo;
    return s->band.on ? &s->band : nullptr;
}

// the pass under way saw exactly the fold pass's samples (the stream must be idle)
static int pass_complete(const TmMode &m, bool *complete)
{
    long long cnt[2] = {0, 0};
    const int rc = m.cnt.read(cnt);
    *complete = rc == TAMCMC_OK && cnt[0] == m.n_used && cnt[1] == m.n_rejected;
    return rc;
}

// One stage of a block, or a result kernel, on the context's stream, between two events of `timer` while the object is
// profiled.  launch() returns a hipError_t; `wrote`, the count pair the launch writes, flips once it has succeeded.
template <class F>
static int timed_launch(tamcmc_summary *s, TmTimer &timer, const char *what, F &&launch, TmCountPair *wrote = nullptr)
{
    const hipStream_t stream = s->c->stream;
    if (s->profile) { const int rc = timer.begin(stream); if (rc != TAMCMC_OK) return rc; }
    const int hr = launch();
    if (hr != 0) return tm_launch_failed(what, hr);
    if (wrote) wrote->flip();
    return s->profile ? timer.end(stream) : TAMCMC_OK;
}

static TmQuantArgs quantile_args(const tamcmc_summary *s)
{
    const TmQuantMode &q = s->q;
    TmQuantArgs a{};
    a.rows = s->d_model; a.fold_state = s->d_state;
    a.kmin = q.kmin; a.R = q.R; a.u = q.u; a.prefix = q.prefix; a.below = q.below; a.ranks = q.d_ranks; a.hist = q.d_hist;
    a.cnt_in = q.cnt.in(); a.cnt_out = q.cnt.out(); a.flag = q.flag;
    a.Nx = s->c->L.Nx; a.Nq = q.Nq; a.bits = q.bits;
    return a;
}

// stage 2 of a block in quantile mode: the histogram kernel in the fold kernel's place
static int quantile_block(tamcmc_summary *s, int n, const int32_t *d_status)
{
    TmQuantArgs a = quantile_args(s);
    a.status = d_status; a.B = n;
    return timed_launch(s, s->timer, "summary quantile histogram", [&] { return tm_launch_quantile_hist(a, s->c->stream); }, &s->q.cnt);
}

// a pass starts from empty counts and a clear flag (the cells are cleared by whoever read them last)
static int quantile_pass_clear(tamcmc_summary *s, bool cells)
{
    TmQuantMode &q = s->q;
    TM_HIP(hipMemsetAsync(q.flag, 0, sizeof(uint32_t), s->c->stream));
    if (cells) TM_HIP(hipMemsetAsync(q.d_hist, 0, q.hist_bytes, s->c->stream));
    return q.cnt.clear(s->c->stream);
}

// the stream must be idle
static void quantile_free(tamcmc_summary *s)
{
    (void)hipFree(s->q.d_state); (void)hipFree(s->q.d_hist);
    s->q = TmQuantMode();
}

static TmLooArgs loo_args(const tamcmc_summary *s)
{
    const TmLooMode &m = s->loo;
    const tamcmc_ctx *c = s->c;
    TmLooArgs a{};
    a.rows = s->d_model; a.y = c->d_y; a.isig2 = c->d_isig2; a.heap = m.d_heap; a.body = m.body;
    a.cnt_in = m.cnt.in(); a.cnt_out = m.cnt.out();
    a.elpd = m.elpd; a.khat = m.khat; a.cutoff = m.cutoff; a.tail_len = m.tail_len;
    a.Nx = c->L.Nx; a.likelihood_case = c->L.likelihood_case; a.cap = m.cap; a.like_p = c->L.like_p;
    return a;
}

// stage 2 of a block in LOO mode: the tail kernel in the fold kernel's place
static int loo_block(tamcmc_summary *s, int n, const int32_t *d_status)
{
    TmLooArgs a = loo_args(s);
    a.status = d_status; a.B = n;
    return timed_launch(s, s->timer, "summary loo tail", [&] { return tm_launch_loo_tail(a, s->c->stream); }, &s->loo.cnt);
}

// a pass starts from empty counts and empty body sums (with no sample counted the heap holds nothing)
static int loo_pass_clear(tamcmc_summary *s)
{
    TmLooMode &m = s->loo;
    TM_HIP(hipMemsetAsync(m.body, 0, 3 * (size_t)s->c->L.Nx * sizeof(double), s->c->stream));
    return m.cnt.clear(s->c->stream);
}

// the stream must be idle
static void loo_free(tamcmc_summary *s)
{
    (void)hipFree(s->loo.d_state); (void)hipFree(s->loo.d_heap); (void)hipFree(s->loo.d_lw); (void)hipFree(s->loo.d_pit);
    s->loo = TmLooMode();
}

static TmLooPitArgs loopit_args(const tamcmc_summary *s)
{
    const TmLooMode &m = s->loo;
    const tamcmc_ctx *c = s->c;
    TmLooPitArgs a{};
    a.rows = s->d_model; a.y = c->d_y; a.isig2 = c->d_isig2; a.heap = m.d_heap; a.body = m.body;
    a.lw = m.d_lw; a.xmax = m.pit_xmax; a.c = m.pit_c; a.first = m.pit_first; a.state = m.pit_sums;
    a.cnt_in = m.pit_cnt.in(); a.cnt_out = m.pit_cnt.out(); a.flag = m.pit_flag;
    a.n = m.n_used;
    a.Nx = c->L.Nx; a.likelihood_case = c->L.likelihood_case; a.cap = m.cap;
    a.p = m.p; a.nterms = m.nterms; a.trips = tlp_trips(m.cap - 1);
    a.like_p = c->L.like_p; a.lf_pm1 = m.lf_pm1; a.lf_p = m.lf_p;
    return a;
}

// stage 2 of a block of the LOO-PIT pass: the PIT kernel in the tail kernel's place
static int loopit_block(tamcmc_summary *s, int n, const int32_t *d_status)
{
    TmLooPitArgs a = loopit_args(s);
    a.status = d_status; a.B = n;
    return timed_launch(s, s->pit_timer, "summary loo pit", [&] { return tm_launch_loopit(a, s->c->stream); }, &s->loo.pit_cnt);
}

// a LOO-PIT pass starts from empty counts, empty sums and a clear flag
static int loopit_pass_clear(tamcmc_summary *s)
{
    TmLooMode &m = s->loo;
    TM_HIP(hipMemsetAsync(m.pit_sums, 0, (size_t)TM_LOOPIT_NSTATE * (size_t)s->c->L.Nx * sizeof(double), s->c->stream));
    TM_HIP(hipMemsetAsync(m.pit_flag, 0, sizeof(int32_t), s->c->stream));
    return m.pit_cnt.clear(s->c->stream);
}

static TmWlooArgs wloo_args(const tamcmc_summary *s)
{
    const TmWlooMode &m = s->wloo;
    const tamcmc_ctx *c = s->c;
    const size_t plane = (size_t)s->B * (size_t)m.n_windows;
    TmWlooArgs a{};
    a.rows = s->d_model; a.y = c->d_y; a.isig2 = c->d_isig2;
    a.sum = m.d_sum; a.logP = m.d_tails; a.logQ = m.d_tails ? m.d_tails + plane : nullptr;
    a.heap = m.d_heap; a.body = m.body;
    a.lw = m.d_lw; a.xmax = m.pit_xmax; a.c = m.pit_c; a.first_slot = m.pit_first; a.state = m.pit_sums; a.flag = m.pit_flag;
    a.cnt_in = m.pit ? m.pit_cnt.in() : m.cnt.in(); a.cnt_out = m.pit ? m.pit_cnt.out() : m.cnt.out();
    a.Nx = c->L.Nx; a.Bcap = s->B; a.n_windows = m.n_windows; a.W = m.W; a.first = m.first;
    a.likelihood_case = c->L.likelihood_case; a.p = m.p; a.cap = m.cap; a.trips = tlp_trips(m.cap - 1);
    a.like_p = c->L.like_p;
    for (int k = 0; k < 3; k++) a.shape[k] = m.shape[k];
    return a;
}

// The finalize kernel of LOO mode and the prepare kernel of LOO-PIT over the windows: n_windows in the place of Nx.  (Neither
// kernel reads rows, y or the likelihood; the prepare launch's check of p is the per-bin check's, so it gets 1.)
static TmLooArgs wloo_finalize_args(const tamcmc_summary *s)
{
    const TmWlooMode &m = s->wloo;
    TmLooArgs a{};
    a.heap = m.d_heap; a.body = m.body;
    a.elpd = m.elpd; a.khat = m.khat; a.cutoff = m.cutoff; a.tail_len = m.tail_len;
    a.n = m.n_used; a.Nx = m.n_windows; a.likelihood_case = s->c->L.likelihood_case; a.cap = m.cap; a.like_p = s->c->L.like_p;
    return a;
}

static TmLooPitArgs wloo_prepare_args(const tamcmc_summary *s)
{
    const TmWlooMode &m = s->wloo;
    TmLooPitArgs a{};
    a.heap = m.d_heap; a.body = m.body;
    a.lw = m.d_lw; a.xmax = m.pit_xmax; a.c = m.pit_c; a.first = m.pit_first; a.state = m.pit_sums;
    a.n = m.n_used; a.Nx = m.n_windows; a.likelihood_case = s->c->L.likelihood_case; a.cap = m.cap;
    a.p = 1; a.trips = tlp_trips(m.cap - 1);
    return a;
}

// stage 2 of a block in window-LOO mode: the sums and tail kernels, or in the sub-mode the sums, tails and PIT kernels
static int wloo_block(tamcmc_summary *s, int n, const int32_t *d_status)
{
    TmWlooArgs a = wloo_args(s);
    a.status = d_status; a.B = n;
    if (s->wloo.pit)
        return timed_launch(s, s->wpit_timer, "summary wloo pit", [&] { return tm_launch_wloo_pit(a, s->c->stream); }, &s->wloo.pit_cnt);
    return timed_launch(s, s->timer, "summary wloo tail", [&] { return tm_launch_wloo_tail(a, s->c->stream); }, &s->wloo.cnt);
}

// a pass starts from empty counts and empty body sums (with no sample counted the heap holds nothing)
static int wloo_pass_clear(tamcmc_summary *s)
{
    TmWlooMode &m = s->wloo;
    TM_HIP(hipMemsetAsync(m.body, 0, 3 * (size_t)m.n_windows * sizeof(double), s->c->stream));
    return m.cnt.clear(s->c->stream);
}

// the sub-mode's pass starts from empty counts, empty sums and a clear flag
static int wloo_pit_pass_clear(tamcmc_summary *s)
{
    TmWlooMode &m = s->wloo;
    TM_HIP(hipMemsetAsync(m.pit_sums, 0, (size_t)TM_LOOPIT_NSTATE * (size_t)m.n_windows * sizeof(double), s->c->stream));
    TM_HIP(hipMemsetAsync(m.pit_flag, 0, sizeof(int32_t), s->c->stream));
    return m.pit_cnt.clear(s->c->stream);
}

// the stream must be idle
static void wloo_free(tamcmc_summary *s)
{
    TmWlooMode &m = s->wloo;
    (void)hipFree(m.d_state); (void)hipFree(m.d_heap); (void)hipFree(m.d_sum); (void)hipFree(m.d_lw); (void)hipFree(m.d_pit); (void)hipFree(m.d_tails);
    s->wloo = TmWlooMode();
}

static TmEssArgs ess_args(const tamcmc_summary *s)
{
    const TmEssMode &m = s->ess;
    const tamcmc_ctx *c = s->c;
    TmEssArgs a{};
    a.y = c->d_y; a.isig2 = c->d_isig2; a.mean_M = s->d_state + (size_t)TM_SUM_MEAN_M * (size_t)c->L.Nx; a.lppd = m.lppd;
    a.ring = m.d_ring; a.acc = m.d_acc; a.half = m.half; a.tau = m.tau; a.ess = m.ess; a.cut = m.cut;
    a.cnt_in = m.cnt.in(); a.cnt_out = m.cnt.out();
    a.n = m.n_used; a.h = m.n_used / 2;
    a.Nx = c->L.Nx; a.L = m.L; a.R = m.R; a.likelihood_case = c->L.likelihood_case; a.like_p = c->L.like_p;
    a.tau_floor = 1.0 / std::log10((double)m.n_used);
    return a;
}

// stage 2 of a block in ESS mode: per chunk of the block the centre kernel and the lag kernel in the fold kernel's place
static int ess_block(tamcmc_summary *s, int n, const int32_t *d_status)
{
    tamcmc_ctx *c = s->c;
    return timed_launch(s, s->timer, "summary ess chunk", [&] {
        int hr = 0;
        for (int k = 0; k < n && hr == 0; k += TM_ESS_CHUNK) {
            TmEssArgs a = ess_args(s);
            a.rows = s->d_model + (size_t)k * (size_t)c->L.Nx; a.status = d_status + k;
            a.B = n - k < TM_ESS_CHUNK ? n - k : TM_ESS_CHUNK;
            hr = tm_launch_ess_chunk(a, c->stream);
            if (hr == 0) s->ess.cnt.flip();                 // per chunk: timed_launch's `wrote` would flip once per block
        }
        return hr;
    });
}

// a pass starts from empty counts, lag products and half-chain moments (a ring slot is written before it is read)
static int ess_pass_clear(tamcmc_summary *s)
{
    TmEssMode &m = s->ess;
    const size_t nx = (size_t)s->c->L.Nx;
    TM_HIP(hipMemsetAsync(m.d_acc, 0, 2 * (size_t)(m.L + 1) * nx * sizeof(double), s->c->stream));
    TM_HIP(hipMemsetAsync(m.half, 0, (size_t)TM_ESS_NHALF * nx * sizeof(double), s->c->stream));
    return m.cnt.clear(s->c->stream);
}

// the stream must be idle
static void ess_free(tamcmc_summary *s)
{
    (void)hipFree(s->ess.d_state); (void)hipFree(s->ess.d_acc); (void)hipFree(s->ess.d_ring);
    s->ess = TmEssMode();
}

static TmBandArgs band_args(const tamcmc_summary *s)
{
    const TmBandMode &m = s->band;
    TmBandArgs a{};
    a.thr = m.thr; a.ring = m.d_bits; a.head = m.head; a.C = m.d_C; a.work = m.d_work; a.tau = m.tau; a.ess = m.ess; a.cut = m.cut;
    a.cnt_in = m.cnt.in(); a.cnt_out = m.cnt.out();
    a.n = m.n_used;
    a.Nx = s->c->L.Nx; a.L = m.L; a.RW = m.RW; a.HW = m.HW; a.K = m.K;
    a.tau_floor = 1.0 / std::log10((double)m.n_used);
    return a;
}

// stage 2 of a block in band ESS mode: per chunk of the block the pack kernel and the lag kernel in the fold kernel's place
static int band_block(tamcmc_summary *s, int n, const int32_t *d_status)
{
    tamcmc_ctx *c = s->c;
    return timed_launch(s, s->timer, "summary bandess chunk", [&] {
        int hr = 0;
        for (int k = 0; k < n && hr == 0; k += TM_ESS_CHUNK) {
            TmBandArgs a = band_args(s);
            a.rows = s->d_model + (size_t)k * (size_t)c->L.Nx; a.status = d_status + k;
            a.B = n - k < TM_ESS_CHUNK ? n - k : TM_ESS_CHUNK;
            hr = tm_launch_bandess_chunk(a, c->stream);
            if (hr == 0) s->band.cnt.flip();                // per chunk, as ess_block
        }
        return hr;
    });
}

static size_t band_bits_bytes(const TmBandMode &m, size_t nx) { return (size_t)m.K * (size_t)(m.RW + m.HW) * nx * sizeof(uint64_t); }

// a pass starts from empty counts and lag counts; the bits are cleared too, so that no launch reads a word never written
static int band_pass_clear(tamcmc_summary *s)
{
    TmBandMode &m = s->band;
    const size_t nx = (size_t)s->c->L.Nx;
    TM_HIP(hipMemsetAsync(m.d_C, 0, (size_t)m.K * (size_t)(m.L + 1) * nx * sizeof(uint32_t), s->c->stream));
    TM_HIP(hipMemsetAsync(m.d_bits, 0, band_bits_bytes(m, nx), s->c->stream));
    return m.cnt.clear(s->c->stream);
}

// the stream must be idle
static void band_free(tamcmc_summary *s)
{
    (void)hipFree(s->band.d_state); (void)hipFree(s->band.d_C); (void)hipFree(s->band.d_bits); (void)hipFree(s->band.d_work);
    s->band = TmBandMode();
}

// stage 3 of a fold-mode block: the predictive kernel on the same rows, counting on from the pair the fold launch read
static int predictive_block(tamcmc_summary *s, int n, const int32_t *d_status, const long long *cnt_in)
{
    tamcmc_ctx *c = s->c;
    TmPredArgs pa{};
    pa.rows = s->d_model; pa.status = d_status; pa.y = c->d_y; pa.isig2 = c->d_isig2; pa.state = s->pred.d_state;
    pa.cnt_in = cnt_in;
    pa.Nx = c->L.Nx; pa.B = n; pa.likelihood_case = c->L.likelihood_case; pa.p = s->pred.p; pa.nterms = s->pred.nterms;
    pa.lf_pm1 = s->pred.lf_pm1; pa.lf_p = s->pred.lf_p;
    return timed_launch(s, s->pred.timer, "summary predictive", [&] { return tm_launch_predictive(pa, c->stream); });
}

// stage 4: the windowed check's three kernels on the same rows, counting on from the same pair
static int window_block(tamcmc_summary *s, int n, const int32_t *d_status, const long long *cnt_in)
{
    tamcmc_ctx *c = s->c;
    const TmWindow &m = s->win;
    TmWinArgs wa{};
    wa.rows = s->d_model; wa.status = d_status; wa.y = c->d_y; wa.isig2 = c->d_isig2; wa.state = m.d_state; wa.scratch = m.d_scratch;
    wa.cnt_in = cnt_in;
    wa.Nx = c->L.Nx; wa.B = n; wa.Bcap = s->B; wa.n_windows = m.n_windows; wa.W = m.W; wa.first = m.first;
    wa.likelihood_case = c->L.likelihood_case; wa.p = m.p;
    for (int k = 0; k < 3; k++) wa.shape[k] = m.shape[k];
    return timed_launch(s, s->win.timer, "summary window", [&] { return tm_launch_window(wa, c->stream); });
}

// stage 5: the scan's kernels on the same rows, per chunk of the block, counting on from the same pair
static int scan_block(tamcmc_summary *s, int n, const int32_t *d_status, const long long *cnt_in)
{
    tamcmc_ctx *c = s->c;
    const TmScan &m = s->scan;
    TmScanArgs sa{};
    sa.rows = s->d_model; sa.status = d_status; sa.y = c->d_y; sa.isig2 = c->d_isig2; sa.state = m.d_state; sa.scratch = m.d_scratch;
    sa.cnt_in = cnt_in;
    sa.total = m.total; sa.Nx = c->L.Nx; sa.B = n; sa.C = m.C; sa.K = m.K;
    sa.likelihood_case = c->L.likelihood_case; sa.p = m.p;
    for (int k = 0; k < m.K; k++) { sa.W[k] = m.W[k]; sa.off[k] = m.off[k]; sa.shape[k] = m.shape[k]; }
    return timed_launch(s, s->scan.timer, "summary scan", [&] { return tm_launch_scan(sa, c->stream); });
}

// One block of n <= B samples, device pointers, enqueued on the context's stream.
static int summary_block(tamcmc_summary *s, int n, const double *d_params, double *d_logL, int32_t *d_status)
{
    tamcmc_ctx *c = s->c;
    int rc = tm_ensure_capacity(c, n, false);
    if (rc != TAMCMC_OK) return rc;
    if (!d_logL) d_logL = s->d_logL;
    if (!d_status) d_status = s->d_status;
    rc = tm_enqueue(c, n, d_params, s->d_T, d_logL, nullptr, d_status, s->d_rows, s->d_model);
    if (rc != TAMCMC_OK) return rc;
    if (s->q.on) return quantile_block(s, n, d_status);
    if (s->loo.on) return s->loo.pit ? loopit_block(s, n, d_status) : loo_block(s, n, d_status);
    if (s->ess.on) return ess_block(s, n, d_status);
    if (s->wloo.on) return wloo_block(s, n, d_status);
    if (s->band.on) return band_block(s, n, d_status);
    TmSummaryArgs a{};
    a.rows = s->d_model; a.status = d_status; a.y = c->d_y; a.isig2 = c->d_isig2; a.state = s->d_state;
    a.cnt_in = s->cnt.in(); a.cnt_out = s->cnt.out();
    a.Nx = c->L.Nx; a.B = n; a.likelihood_case = c->L.likelihood_case; a.like_p = c->L.like_p;
    rc = timed_launch(s, s->timer, "summary fold", [&] { return tm_launch_summary_fold(a, c->stream); }, &s->cnt);
    if (rc != TAMCMC_OK) return rc;
    if (s->pred.on) { rc = predictive_block(s, n, d_status, a.cnt_in); if (rc != TAMCMC_OK) return rc; }
    if (s->win.on) { rc = window_block(s, n, d_status, a.cnt_in); if (rc != TAMCMC_OK) return rc; }
    return s->scan.on ? scan_block(s, n, d_status, a.cnt_in) : TAMCMC_OK;
}

static int summary_clear(tamcmc_summary *s)
{
    const tamcmc_ctx *c = s->c;
    if (s->pred.on) TM_HIP(hipMemsetAsync(s->pred.d_state, 0, (size_t)TM_PRED_NSTATE * (size_t)c->L.Nx * sizeof(double), c->stream));
    if (s->win.on) TM_HIP(hipMemsetAsync(s->win.d_state, 0, (size_t)TM_PRED_NSTATE * (size_t)s->win.n_windows * sizeof(double), c->stream));
    if (s->scan.on) TM_HIP(hipMemsetAsync(s->scan.d_state, 0, (size_t)TM_PRED_NSTATE * (size_t)s->scan.total * sizeof(double), c->stream));
    TM_HIP(hipMemsetAsync(s->d_state, 0, (size_t)TM_SUM_NSTATE * (size_t)c->L.Nx * sizeof(double), c->stream));
    return s->cnt.clear(c->stream);
}

extern "C" int tamcmc_summary_create(tamcmc_summary **out, tamcmc_ctx *c, int32_t block_chains)
{
    if (!out) return TAMCMC_E_INVALID;
    *out = nullptr;
    if (!c || block_chains < 0 || c->in_flight || c->armed) return TAMCMC_E_INVALID;
    if (c->nspec > 1) return TAMCMC_E_INVALID;      // several spectra in one context: out of scope
    tamcmc_summary *s = new (std::nothrow) tamcmc_summary();
    if (!s) return TAMCMC_E_NOMEM;
    s->c = c;
    const size_t nx = (size_t)c->L.Nx;
    int B = block_chains;
    if (B == 0) B = tms_default_block((long long)nx);      // 64, lowered so that a block's rows take at most 64 MiB
    s->B = B;
    auto fail = [&](int code) { tamcmc_summary_destroy(s); return code; };
    if (hipSetDevice(c->device) != hipSuccess) return fail(TAMCMC_E_NODEVICE);
    const size_t b = (size_t)B;
    if (hipMalloc(&s->d_model, b * nx * sizeof(double)) != hipSuccess || hipMalloc(&s->d_state, TM_SUM_NSTATE * nx * sizeof(double)) != hipSuccess ||
        hipMalloc(&s->cnt.d, 4 * sizeof(long long)) != hipSuccess || hipMalloc(&s->d_rows, b * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&s->d_T, b * sizeof(double)) != hipSuccess || hipMalloc(&s->d_logL, b * sizeof(double)) != hipSuccess ||
        hipMalloc(&s->d_status, b * sizeof(int32_t)) != hipSuccess)
        return fail(TAMCMC_E_NOMEM);
    {
        std::vector<int32_t> rows(b);
        std::vector<double> ones(b, 1.0);
        for (size_t k = 0; k < b; k++) rows[k] = (int32_t)k;
        if (hipMemcpy(s->d_rows, rows.data(), b * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(s->d_T, ones.data(), b * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            return fail(TAMCMC_E_HIP);
    }
    if (tm_ctx_settle(c) != hipSuccess || summary_clear(s) != TAMCMC_OK) return fail(TAMCMC_E_HIP);
    c->enq_seq++;
    c->summaries++;
    s->counted = true;
    *out = s;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_destroy(tamcmc_summary *s)
{
    if (!s) return TAMCMC_OK;
    tamcmc_ctx *c = s->c;
    if (c->armed) return TAMCMC_E_INVALID;          // the stream cannot be waited for behind a closed gate: _fire or _disarm first
    (void)hipSetDevice(c->device);
    if (c->stream) (void)tm_ctx_stream_sync(c);
    if (s->counted) c->summaries--;
    quantile_free(s);
    loo_free(s);
    ess_free(s);
    band_free(s);
    wloo_free(s);
    (void)hipFree(s->d_model); (void)hipFree(s->d_state); (void)hipFree(s->cnt.d); (void)hipFree(s->d_rows);
    (void)hipFree(s->d_T); (void)hipFree(s->d_logL); (void)hipFree(s->d_status); (void)hipFree(s->pred.d_state);
    (void)hipFree(s->win.d_state); (void)hipFree(s->win.d_scratch);
    (void)hipFree(s->scan.d_state); (void)hipFree(s->scan.d_scratch);
    for (int p = 0; p < 2; p++) {
        s->stage[p].release();
        if (s->ev_stage[p]) (void)hipEventDestroy(s->ev_stage[p]);
    }
    s->timer.destroy();
    s->pit_timer.destroy();
    s->wpit_timer.destroy();
    s->pred.timer.destroy();
    s->win.timer.destroy();
    s->scan.timer.destroy();
    delete s;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_reset(tamcmc_summary *s)
{
    if (!s || s->c->in_flight || s->c->armed) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = s->c;
    TM_HIP(hipSetDevice(c->device));
    if (active_mode(s)) {                           // reset leaves quantile mode, LOO mode, ESS mode, band ESS mode and window-LOO mode
        TM_HIP(tm_ctx_stream_sync(c));
        quantile_free(s);
        loo_free(s);
        ess_free(s);
        band_free(s);
        wloo_free(s);
    }
    TM_HIP(tm_ctx_settle(c));
    c->enq_seq++;
    return summary_clear(s);
}

extern "C" int tamcmc_summary_push_device(tamcmc_summary *s, int32_t Nsamples, int32_t Nparams, const double *d_params,
                                          double *d_logL, int32_t *d_status)
{
    int rc = summary_check(s, Nsamples, Nparams, d_params);
    if (rc != TAMCMC_OK) return rc;
    TM_HIP(hipSetDevice(s->c->device));
    for (int32_t k = 0; k < Nsamples; k += s->B) {
        const int n = Nsamples - k < s->B ? Nsamples - k : s->B;
        rc = summary_block(s, n, d_params + (size_t)k * (size_t)Nparams, d_logL ? d_logL + k : nullptr, d_status ? d_status + k : nullptr);
        if (rc != TAMCMC_OK) return rc;
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_push(tamcmc_summary *s, int32_t Nsamples, int32_t Nparams, const double *params,
                                   double *logL, int32_t *status)
{
    int rc = summary_check(s, Nsamples, Nparams, params);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = s->c;
    TM_HIP(hipSetDevice(c->device));
    const size_t o_out = summary_stage_out(s), bytes = summary_stage_bytes(s), np = (size_t)Nparams;
    for (int p = 0; p < 2; p++) {
        if (s->stage[p].fits(bytes)) continue;
        rc = s->stage[p].reserve(bytes, TM_PIN_TWIN);
        if (rc != TAMCMC_OK) return rc;
        TM_HIP(hipEventCreateWithFlags(&s->ev_stage[p], hipEventDisableTiming));
    }
    // slot p's copies have landed: hand its block's logL / status out (polled: tm_poll_event)
    int pend_k[2] = {-1, -1}, pend_n[2] = {0, 0};
    auto collect = [&](int p) -> int {
        if (pend_k[p] < 0) return TAMCMC_OK;
        const int prc = tm_poll_event(s->ev_stage[p]);
        if (prc != TAMCMC_OK) return prc;
        const size_t n = (size_t)pend_n[p];
        if (logL) std::memcpy(logL + pend_k[p], s->stage[p].h + o_out, n * sizeof(double));
        if (status) std::memcpy(status + pend_k[p], s->stage[p].h + o_out + (size_t)s->B * sizeof(double), n * sizeof(int32_t));
        pend_k[p] = -1;
        return TAMCMC_OK;
    };
    // a failure waits for the stream before it returns: a copy from or into the pinned slots may still be pending
    auto fail = [&](int code) { (void)hipStreamSynchronize(c->stream); return code; };
    int slot = 0;
    for (int32_t k = 0; k < Nsamples; k += s->B, slot ^= 1) {
        const int n = Nsamples - k < s->B ? Nsamples - k : s->B;
        rc = collect(slot);
        if (rc != TAMCMC_OK) return fail(rc);
        char *const h = s->stage[slot].h, *const d = s->stage[slot].d;
        std::memcpy(h, params + (size_t)k * np, (size_t)n * np * sizeof(double));
        if (tm_ctx_settle(c) != hipSuccess ||
            hipMemcpyAsync(d, h, (size_t)n * np * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return fail(TAMCMC_E_HIP);
        rc = summary_block(s, n, reinterpret_cast<const double *>(d), reinterpret_cast<double *>(d + o_out),
                           reinterpret_cast<int32_t *>(d + o_out + (size_t)s->B * sizeof(double)));
        if (rc != TAMCMC_OK) return fail(rc);
        if (hipMemcpyAsync(h + o_out, d + o_out, bytes - o_out, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipEventRecord(s->ev_stage[slot], c->stream) != hipSuccess)
            return fail(TAMCMC_E_HIP);
        pend_k[slot] = k; pend_n[slot] = n;
    }
    // the older of the two pending blocks first: the stream runs them in order
    rc = collect(slot);
    if (rc == TAMCMC_OK) rc = collect(slot ^ 1);
    if (rc != TAMCMC_OK) return fail(rc);
    TM_HIP(hipGetLastError());
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_result(tamcmc_summary *s, tamcmc_summary_totals *totals,
                                     double *mean_M, double *var_M, double *min_M, double *max_M,
                                     double *mean_l, double *var_l, double *lppd)
{
    long long cnt[2] = {0, 0};
    const int rc = summary_enter(s, cnt);
    if (rc != TAMCMC_OK) return rc;
    const size_t nx = (size_t)s->c->L.Nx;
    std::vector<double> st;
    try { st.resize(TM_SUM_NSTATE * nx); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    TM_HIP(hipMemcpy(st.data(), s->d_state, st.size() * sizeof(double), hipMemcpyDeviceToHost));
    const long long n = cnt[0];
    const double nan = std::nan(""), dn = (double)n;
    long double lppd_total = 0.0L, p_waic = 0.0L;
    for (size_t i = 0; i < nx; i++) {
        const double vM = n >= 2 ? st[TM_SUM_M2_M * nx + i] / (dn - 1.0) : nan;
        const double vl = n >= 2 ? st[TM_SUM_M2_L * nx + i] / (dn - 1.0) : nan;
        const double lp = n >= 1 ? tm_lppd(st[TM_SUM_LSE_A * nx + i], st[TM_SUM_LSE_R * nx + i], dn) : nan;
        if (mean_M) mean_M[i] = n >= 1 ? st[TM_SUM_MEAN_M * nx + i] : nan;
        if (var_M) var_M[i] = vM;
        if (min_M) min_M[i] = n >= 1 ? st[TM_SUM_MIN_M * nx + i] : nan;
        if (max_M) max_M[i] = n >= 1 ? st[TM_SUM_MAX_M * nx + i] : nan;
        if (mean_l) mean_l[i] = n >= 1 ? st[TM_SUM_MEAN_L * nx + i] : nan;
        if (var_l) var_l[i] = vl;
        if (lppd) lppd[i] = lp;
        lppd_total += (long double)lp;          // in bin order
        p_waic += (long double)vl;
    }
    if (totals) {
        totals->n_used = n;
        totals->n_rejected = cnt[1];
        totals->lppd_total = (double)lppd_total;
        totals->p_waic = (double)p_waic;
        totals->waic = (double)(-2.0L * (lppd_total - p_waic));
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_profile(tamcmc_summary *s, int enable)
{
    if (!s || s->c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(s->c->device));
    TM_HIP(tm_ctx_stream_sync(s->c));
    s->profile = enable != 0;
    s->timer.used = 0;
    s->pit_timer.used = 0;
    s->wpit_timer.used = 0;
    s->pred.timer.used = 0;
    s->win.timer.used = 0;
    s->scan.timer.used = 0;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_kernel_time(tamcmc_summary *s, double *total_ms, int64_t *launches)
{
    if (!s || !total_ms || !launches || s->c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(s->c->device));
    TM_HIP(tm_ctx_stream_sync(s->c));
    return s->timer.total(total_ms, launches);
}

// ---- quantiles (tamcmc_quantile.h) ----

extern "C" int tamcmc_summary_quantiles_begin(tamcmc_summary *s, int32_t Nq, const double *q, int32_t bits_per_pass)
{
    if (!s || !q || Nq < 1 || Nq > TAMCMC_SUMMARY_MAX_QUANTILES || bits_per_pass < 0 || bits_per_pass > TM_Q_MAXBITS) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = s->c;
    if (active_mode(s)) return TAMCMC_E_INVALID;
    for (int j = 0; j < Nq; j++)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return TAMCMC_E_INVALID;        // (a NaN fails both comparisons)
    long long cnt[2] = {0, 0};
    const int rc = summary_enter(s, cnt);
    if (rc != TAMCMC_OK) return rc;
    if (cnt[0] < 1 || cnt[0] >= ((long long)1 << 32)) return TAMCMC_E_INVALID;
    TmQuantMode m;
    m.Nq = Nq;
    m.bits = bits_per_pass ? bits_per_pass : TM_Q_DEFAULT_BITS;
    m.n_used = cnt[0]; m.n_rejected = cnt[1];
    uint64_t ranks[TM_Q_MAXQ] = {};
    for (int j = 0; j < Nq; j++) {
        m.ranks[j] = tmq_rank(q[j], (int64_t)cnt[0]);
        ranks[j] = (uint64_t)m.ranks[j];
    }
    const size_t nx = (size_t)c->L.Nx, nq = (size_t)Nq;
    const size_t state_bytes = (2 * nx + 2 * nq * nx + TM_Q_MAXQ) * sizeof(uint64_t) + 4 * sizeof(long long) + (nx + 1) * sizeof(uint32_t);
    m.hist_bytes = (nq << m.bits) * nx * sizeof(uint32_t);
    if (hipMalloc(&m.d_state, state_bytes) != hipSuccess) { (void)hipGetLastError(); return TAMCMC_E_NOMEM; }
    if (hipMalloc(&m.d_hist, m.hist_bytes) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(m.d_state); return TAMCMC_E_NOMEM; }
    m.kmin = reinterpret_cast<uint64_t *>(m.d_state);
    m.R = m.kmin + nx;
    m.prefix = m.R + nx;
    m.below = m.prefix + nq * nx;
    m.d_ranks = m.below + nq * nx;
    m.cnt.d = reinterpret_cast<long long *>(m.d_ranks + TM_Q_MAXQ);
    m.u = reinterpret_cast<uint32_t *>(m.cnt.d + 4);
    m.flag = m.u + nx;
    m.on = true;
    s->q = m;
    auto fail = [&](int code) { (void)hipStreamSynchronize(c->stream); quantile_free(s); return code; };
    c->enq_seq++;
    if (hipMemcpyAsync(m.d_ranks, ranks, sizeof(ranks), hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(TAMCMC_E_HIP);
    if (quantile_pass_clear(s, true) != TAMCMC_OK) return fail(TAMCMC_E_HIP);
    const int hr = tm_launch_quantile_init(quantile_args(s), c->stream);
    if (hr != 0) { (void)tm_launch_failed("summary quantile init", hr); return fail(TAMCMC_E_HIP); }
    std::vector<uint32_t> u;
    try { u.resize(nx); } catch (const std::bad_alloc &) { return fail(TAMCMC_E_NOMEM); }
    if (hipMemcpyAsync(u.data(), m.u, nx * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)                    // (also: `ranks` is read before it goes out of scope)
        return fail(TAMCMC_E_HIP);
    for (size_t i = 0; i < nx; i++) s->q.u0max = (int)u[i] > s->q.u0max ? (int)u[i] : s->q.u0max;
    return TAMCMC_OK;
}

static int quantile_bits_left(const TmQuantMode &q)
{
    const int left = q.u0max - q.passes * q.bits;
    return left > 0 ? left : 0;
}

extern "C" int tamcmc_summary_quantiles_step(tamcmc_summary *s, int32_t *bits_left)
{
    if (!s || !s->q.on) return TAMCMC_E_INVALID;
    int rc = summary_enter(s);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = s->c;
    TmQuantMode &q = s->q;
    c->enq_seq++;
    if (quantile_bits_left(q) == 0) {                  // nothing to resolve: whatever was pushed is dropped
        rc = quantile_pass_clear(s, false);
        if (bits_left) *bits_left = 0;
        return rc;
    }
    bool complete = false;
    uint32_t flag = 0;
    rc = pass_complete(q, &complete);
    if (rc != TAMCMC_OK) return rc;
    TM_HIP(hipMemcpy(&flag, q.flag, sizeof(flag), hipMemcpyDeviceToHost));
    if (!complete || flag != 0) {                      // not the fold pass's samples: the pass is discarded
        rc = quantile_pass_clear(s, true);
        return rc != TAMCMC_OK ? rc : TAMCMC_E_INVALID;
    }
    const int hr = tm_launch_quantile_narrow(quantile_args(s), c->stream);
    if (hr != 0) return tm_launch_failed("summary quantile narrow", hr);
    q.passes++;
    rc = quantile_pass_clear(s, false);                // the narrow kernel cleared the cells it read; the others were never written
    if (bits_left) *bits_left = quantile_bits_left(q);
    return rc;
}

extern "C" int tamcmc_summary_quantiles_result(tamcmc_summary *s, int64_t *ranks, double *lo, double *hi)
{
    if (!s || !s->q.on) return TAMCMC_E_INVALID;
    const int rc = summary_enter(s);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = s->c;
    const TmQuantMode &q = s->q;
    if (ranks) for (int j = 0; j < q.Nq; j++) ranks[j] = q.ranks[j];
    if (!lo && !hi) return TAMCMC_OK;
    const size_t nx = (size_t)c->L.Nx, nq = (size_t)q.Nq;
    std::vector<uint64_t> kr, pre;
    std::vector<uint32_t> u;
    std::vector<double> env;
    try { kr.resize(2 * nx); pre.resize(nq * nx); u.resize(nx); env.resize(2 * nx); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    TM_HIP(hipMemcpy(kr.data(), q.kmin, 2 * nx * sizeof(uint64_t), hipMemcpyDeviceToHost));          // kmin | R
    TM_HIP(hipMemcpy(pre.data(), q.prefix, nq * nx * sizeof(uint64_t), hipMemcpyDeviceToHost));
    TM_HIP(hipMemcpy(u.data(), q.u, nx * sizeof(uint32_t), hipMemcpyDeviceToHost));
    TM_HIP(hipMemcpy(env.data(), s->d_state + (size_t)TM_SUM_MIN_M * nx, 2 * nx * sizeof(double), hipMemcpyDeviceToHost));   // min_M | max_M
    // the double of an offset: the envelope's own bits at its two ends
    auto value = [&](size_t i, uint64_t D) { return D == 0 ? env[i] : (D == kr[nx + i] ? env[nx + i] : tmq_unkey(kr[i] + D)); };
    for (size_t j = 0; j < nq; j++)
        for (size_t i = 0; i < nx; i++) {
            uint64_t dlo, dhi;
            tmq_bracket(pre[j * nx + i], (int)u[i], kr[nx + i], &dlo, &dhi);
            if (lo) lo[j * nx + i] = value(i, dlo);
            if (hi) hi[j * nx + i] = value(i, dhi);
        }
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_quantiles_end(tamcmc_summary *s)
{
    if (!s || !s->q.on) return TAMCMC_E_INVALID;
    const int rc = summary_enter(s);
    if (rc == TAMCMC_OK) quantile_free(s);
    return rc;
}

// What the PIT totals of the per-bin check, the windowed check and LOO-PIT share: the cell of a PIT value, and the
// Kolmogorov distance of a non-empty set of them from uniform, in long double (u is sorted in place).
static int tm_pit_cell(const double pv)
{
    const int cell = (int)std::floor(20.0 * pv);
    return cell > TAMCMC_SUMMARY_PIT_CELLS - 1 ? TAMCMC_SUMMARY_PIT_CELLS - 1 : (cell < 0 ? 0 : cell);
}

static double tm_ks_uniform(std::vector<double> &u)
{
    std::sort(u.begin(), u.end());
    const long double N = (long double)u.size();
    long double D = 0.0L;
    for (size_t k = 0; k < u.size(); k++) {
        const long double up = (long double)(k + 1) / N - (long double)u[k], dn = (long double)u[k] - (long double)k / N;
        D = up > D ? up : D;
        D = dn > D ? dn : D;
    }
    return (double)D;
}

// ---- PSIS-LOO (tamcmc_loo.h) ----

extern "C" int tamcmc_summary_loo_begin(tamcmc_summary *s)
{
    if (!s || active_mode(s)) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = s->c;
    long long cnt[2] = {0, 0};
    const int rc = summary_enter(s, cnt);
    if (rc != TAMCMC_OK) return rc;
    if (cnt[0] < 1) return TAMCMC_E_INVALID;
    const int64_t M = tml_tail_M((int64_t)cnt[0]);
    if (M > TAMCMC_SUMMARY_LOO_MAX_TAIL) return TAMCMC_E_INVALID;       // thin the chain
    TmLooMode m;
    m.cap = (int)M + 1;
    m.n_used = cnt[0]; m.n_rejected = cnt[1];
    const size_t nx = (size_t)c->L.Nx;
    const size_t state_bytes = 6 * nx * sizeof(double) + 4 * sizeof(long long) + nx * sizeof(int32_t);
    if (hipMalloc(&m.d_state, state_bytes) != hipSuccess) { (void)hipGetLastError(); return TAMCMC_E_NOMEM; }
    if (hipMalloc(&m.d_heap, (size_t)m.cap * nx * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(m.d_state); return TAMCMC_E_NOMEM; }
    m.body = reinterpret_cast<double *>(m.d_state);
    m.elpd = m.body + 3 * nx;
    m.khat = m.elpd + nx;
    m.cutoff = m.khat + nx;
    m.cnt.d = reinterpret_cast<long long *>(m.cutoff + nx);
    m.tail_len = reinterpret_cast<int32_t *>(m.cnt.d + 4);
    m.on = true;
    s->loo = m;
    c->enq_seq++;
    if (loo_pass_clear(s) != TAMCMC_OK) { (void)hipStreamSynchronize(c->stream); loo_free(s); return TAMCMC_E_HIP; }
    return TAMCMC_OK;
}

// What loo_result and wloo_result share once their pass is known to be complete: `finalize` enqueues the finalize kernel
// over m units (bins or windows), whose results lie at d_out (elpd | khat | cutoff, m doubles each) and d_tl; the arrays go
// to the host (any may be NULL) and the totals are summed in unit order in long double, lppd over all bins.
struct TmLooSums {
    double elpd, p, k_max;
    int64_t n_high, n_inf;
};

template <class F>
static int loo_collect(tamcmc_summary *s, const size_t m, const double *d_out, const int32_t *d_tl, const long long n_used, F &&finalize,
                       double *elpd_loo, double *pareto_k, double *cutoff, int32_t *tail_len, TmLooSums *sums)
{
    tamcmc_ctx *c = s->c;
    const size_t nx = (size_t)c->L.Nx;
    std::vector<double> out, lse;
    std::vector<int32_t> tl;
    try { out.resize(3 * m); lse.resize(2 * nx); tl.resize(m); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    const int rc = finalize();
    if (rc != TAMCMC_OK) return rc;
    TM_HIP(hipMemcpyAsync(out.data(), d_out, 3 * m * sizeof(double), hipMemcpyDeviceToHost, c->stream));      // elpd | khat | cutoff
    TM_HIP(hipMemcpyAsync(tl.data(), d_tl, m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    TM_HIP(hipMemcpyAsync(lse.data(), s->d_state + (size_t)TM_SUM_LSE_A * nx, 2 * nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));   // a | r
    TM_HIP(hipStreamSynchronize(c->stream));
    const double dn = (double)n_used;
    long double lppd_total = 0.0L, elpd_total = 0.0L;
    double k_max = std::nan("");
    int64_t n_high = 0, n_inf = 0;
    for (size_t i = 0; i < nx; i++) lppd_total += (long double)tm_lppd(lse[i], lse[nx + i], dn);      // as tamcmc_summary_result, in bin order
    for (size_t i = 0; i < m; i++) {
        const double k = out[m + i];
        elpd_total += (long double)out[i];
        if (!(k <= k_max)) k_max = std::isnan(k) ? k_max : k;                 // (a NaN k-hat is never the maximum)
        if (k > 0.7) n_high++;
        if (std::isinf(k) && k > 0.0) n_inf++;
    }
    if (elpd_loo) std::memcpy(elpd_loo, out.data(), m * sizeof(double));
    if (pareto_k) std::memcpy(pareto_k, out.data() + m, m * sizeof(double));
    if (cutoff) std::memcpy(cutoff, out.data() + 2 * m, m * sizeof(double));
    if (tail_len) std::memcpy(tail_len, tl.data(), m * sizeof(int32_t));
    sums->elpd = (double)elpd_total;
    sums->p = (double)(lppd_total - elpd_total);
    sums->k_max = k_max; sums->n_high = n_high; sums->n_inf = n_inf;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_loo_result(tamcmc_summary *s, tamcmc_summary_loo_totals *totals, double *elpd_loo, double *pareto_k,
                                         double *cutoff, int32_t *tail_len)
{
    if (!s || !s->loo.on) return TAMCMC_E_INVALID;
    int rc = summary_enter(s);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = s->c;
    TmLooMode &m = s->loo;
    c->enq_seq++;
    bool complete = false;
    rc = pass_complete(m, &complete);
    if (rc != TAMCMC_OK) return rc;
    if (!complete) {                                                    // not the fold pass's samples: the pass is discarded
        rc = loo_pass_clear(s);
        return rc != TAMCMC_OK ? rc : TAMCMC_E_INVALID;
    }
    TmLooArgs a = loo_args(s);
    a.n = m.n_used;
    TmLooSums f;
    rc = loo_collect(s, (size_t)c->L.Nx, m.elpd, m.tail_len, m.n_used,
                     [&] { return timed_launch(s, s->timer, "summary loo finalize", [&] { return tm_launch_loo_finalize(a, c->stream); }); },
                     elpd_loo, pareto_k, cutoff, tail_len, &f);
    if (rc != TAMCMC_OK) return rc;
    if (totals) {
        totals->n_used = m.n_used;
        totals->n_rejected = m.n_rejected;
        totals->elpd_loo = f.elpd;
        totals->p_loo = f.p;
        totals->looic = (double)(-2.0L * (long double)f.elpd);
        totals->k_max = f.k_max;
        totals->n_k_high = f.n_high;
        totals->n_k_inf = f.n_inf;
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_loo_end(tamcmc_summary *s)
{
    if (!s || !s->loo.on) return TAMCMC_E_INVALID;
    const int rc = summary_enter(s);
    if (rc == TAMCMC_OK) loo_free(s);
    return rc;
}

// ---- LOO-PIT (tamcmc_loopit.h) ----

extern "C" int tamcmc_summary_loo_pit_begin(tamcmc_summary *s)
{
    if (!s || !s->loo.on || s->loo.pit) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = s->c;
    const bool chi = c->L.likelihood_case == 0;
    if (chi && !(c->L.like_p >= 1.0 && c->L.like_p <= (double)TAMCMC_SUMMARY_PREDICTIVE_MAX_P)) return TAMCMC_E_INVALID;
    int rc = summary_enter(s);
    if (rc != TAMCMC_OK) return rc;
    TmLooMode &m = s->loo;
    bool complete = false;
    rc = pass_complete(m, &complete);
    if (rc != TAMCMC_OK) return rc;
    if (!complete) return TAMCMC_E_INVALID;                             // the pass under way stays as it is
    const size_t nx = (size_t)c->L.Nx;
    const size_t pit_bytes = ((size_t)TM_LOOPIT_NSTATE + 2) * nx * sizeof(double) + 4 * sizeof(long long) + (nx + 1) * sizeof(int32_t);
    double *d_lw = nullptr;
    char *d_pit = nullptr;
    if (hipMalloc(&d_lw, (size_t)(m.cap - 1) * nx * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return TAMCMC_E_NOMEM; }
    if (hipMalloc(&d_pit, pit_bytes) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(d_lw); return TAMCMC_E_NOMEM; }
    m.d_lw = d_lw; m.d_pit = d_pit;
    m.pit_sums = reinterpret_cast<double *>(d_pit);
    m.pit_xmax = m.pit_sums + (size_t)TM_LOOPIT_NSTATE * nx;
    m.pit_c = m.pit_xmax + nx;
    m.pit_cnt.d = reinterpret_cast<long long *>(m.pit_c + nx);
    m.pit_cnt.parity = 0;
    m.pit_first = reinterpret_cast<int32_t *>(m.pit_cnt.d + 4);
    m.pit_flag = m.pit_first + nx;
    m.p = chi ? (int)c->L.like_p : 1;
    m.nterms = tmp_series_terms(m.p);
    m.lf_pm1 = tmp_log_factorial(m.p - 1);
    m.lf_p = tmp_log_factorial(m.p);
    c->enq_seq++;
    TmLooPitArgs a = loopit_args(s);
    rc = timed_launch(s, s->timer, "summary loo pit prepare", [&] { return tm_launch_loopit_prepare(a, c->stream); });
    if (rc == TAMCMC_OK) rc = loopit_pass_clear(s);
    if (rc == TAMCMC_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = TAMCMC_E_HIP;
    if (rc != TAMCMC_OK) {              // (a launch that was refused wrote nothing: the top sets are as the LOO pass left them)
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(d_lw); (void)hipFree(d_pit);
        m.d_lw = nullptr; m.d_pit = nullptr;
        return rc;
    }
    m.pit = true;
    return TAMCMC_OK;
}

// What loo_pit_result and wloo_pit_result share once their pass is known to be complete: d_sums[TM_LOOPIT_NSTATE + 1][nx], the
// four sums and xmax of nx units (bins or windows); the five arrays (any may be NULL) and the totals in unit order.
static int loopit_collect(const double *d_sums, const size_t nx, const long long n_used, const long long n_rejected,
                          tamcmc_summary_loo_pit_totals *totals, double *loo_pit, double *loo_log_cdf, double *loo_log_sf,
                          double *is_ess, double *log_wsum)
{
    std::vector<double> st, u;
    try { st.resize(((size_t)TM_LOOPIT_NSTATE + 1) * nx); u.reserve(nx); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    TM_HIP(hipMemcpy(st.data(), d_sums, st.size() * sizeof(double), hipMemcpyDeviceToHost));         // sums | xmax
    const double nan = std::nan("");
    tamcmc_summary_loo_pit_totals t{};
    t.n_used = n_used; t.n_rejected = n_rejected;
    t.ks_D = nan; t.min_log_sf = nan; t.min_log_cdf = nan; t.min_is_ess = nan;
    t.bin_min_log_sf = -1; t.bin_min_log_cdf = -1; t.bin_min_is_ess = -1;
    for (size_t i = 0; i < nx; i++) {
        auto word = [&](int k) { return st[(size_t)k * nx + i]; };
        double lc = nan, ls = nan, ess = nan, lW = nan;
        if (std::isfinite(word(TM_LOOPIT_NSTATE))) {
            lW = tlp_lse(word(TM_LOOPIT_W_A), word(TM_LOOPIT_W_R), word(TM_LOOPIT_W_C));
            lc = tlp_lse(word(TM_LOOPIT_A_A), word(TM_LOOPIT_A_R), word(TM_LOOPIT_A_C)) - lW;
            ls = tlp_lse(word(TM_LOOPIT_B_A), word(TM_LOOPIT_B_R), word(TM_LOOPIT_B_C)) - lW;
            ess = std::exp(2.0 * lW - tlp_lse(word(TM_LOOPIT_W2_A), word(TM_LOOPIT_W2_R), word(TM_LOOPIT_W2_C)));
        }
        const double pv = lc < ls ? std::exp(lc) : -std::expm1(ls);                 // from the smaller tail
        if (loo_pit) loo_pit[i] = pv;
        if (loo_log_cdf) loo_log_cdf[i] = lc;
        if (loo_log_sf) loo_log_sf[i] = ls;
        if (is_ess) is_ess[i] = ess;
        if (log_wsum) log_wsum[i] = lW;
        if (t.bin_min_log_sf < 0 ? !std::isnan(ls) : ls < t.min_log_sf) { t.min_log_sf = ls; t.bin_min_log_sf = (int64_t)i; }   // the first bin wins a tie
        if (t.bin_min_log_cdf < 0 ? !std::isnan(lc) : lc < t.min_log_cdf) { t.min_log_cdf = lc; t.bin_min_log_cdf = (int64_t)i; }
        if (t.bin_min_is_ess < 0 ? !std::isnan(ess) : ess < t.min_is_ess) { t.min_is_ess = ess; t.bin_min_is_ess = (int64_t)i; }
        if (std::isnan(pv)) continue;
        t.pit_hist[tm_pit_cell(pv)]++;
        u.push_back(pv);
    }
    if (!u.empty()) t.ks_D = tm_ks_uniform(u);
    if (totals) *totals = t;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_loo_pit_result(tamcmc_summary *s, tamcmc_summary_loo_pit_totals *totals, double *loo_pit, double *loo_log_cdf,
                                             double *loo_log_sf, double *is_ess, double *log_wsum)
{
    if (!s || !s->loo.on || !s->loo.pit) return TAMCMC_E_INVALID;
    int rc = summary_enter(s);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = s->c;
    TmLooMode &m = s->loo;
    c->enq_seq++;
    long long cnt[2] = {0, 0};
    int32_t flag = 0;
    rc = m.pit_cnt.read(cnt);
    if (rc != TAMCMC_OK) return rc;
    TM_HIP(hipMemcpy(&flag, m.pit_flag, sizeof flag, hipMemcpyDeviceToHost));
    if (cnt[0] != m.n_used || cnt[1] != m.n_rejected || flag != 0) {    // not the LOO pass's samples: the PIT pass is discarded
        rc = loopit_pass_clear(s);
        return rc != TAMCMC_OK ? rc : TAMCMC_E_INVALID;
    }
    return loopit_collect(m.pit_sums, (size_t)c->L.Nx, m.n_used, m.n_rejected, totals, loo_pit, loo_log_cdf, loo_log_sf, is_ess, log_wsum);
}

extern "C" int tamcmc_summary_loo_pit_kernel_time(tamcmc_summary *s, double *total_ms, int64_t *launches)
{
    if (!s || !total_ms || !launches || !s->loo.on || !s->loo.pit || s->c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(s->c->device));
    TM_HIP(tm_ctx_stream_sync(s->c));
    return s->pit_timer.total(total_ms, launches);
}

// ---- window-LOO: PSIS-LOO and LOO-PIT with a window left out (tamcmc_wloo.h) ----

extern "C" int tamcmc_summary_wloo_begin(tamcmc_summary *s, int32_t W, int32_t first, int32_t *n_windows)
{
    if (!s || W < 1 || W > TAMCMC_SUMMARY_WINDOW_MAX_BINS || first < 0 || first > W || active_mode(s)) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = s->c;
    long long cnt[2] = {0, 0};
    const int rc = summary_enter(s, cnt);
    if (rc != TAMCMC_OK) return rc;
    if (cnt[0] < 1) return TAMCMC_E_INVALID;
    const int64_t M = tml_tail_M((int64_t)cnt[0]);
    if (M > TAMCMC_SUMMARY_LOO_MAX_TAIL) return TAMCMC_E_INVALID;       // thin the chain
    TmWlooMode m;
    int f = first, len[3];
    const size_t nw = (size_t)tmw_partition((long long)c->L.Nx, W, &f, len);
    m.W = W; m.first = f; m.n_windows = (int)nw;
    m.cap = (int)M + 1;
    m.n_used = cnt[0]; m.n_rejected = cnt[1];
    m.p = c->L.likelihood_case == 0 ? (int)c->L.like_p : 1;
    if (hipMalloc(&m.d_state, twl_state_bytes(nw)) != hipSuccess) { (void)hipGetLastError(); return TAMCMC_E_NOMEM; }
    if (hipMalloc(&m.d_heap, twl_heap_bytes(nw, (size_t)M)) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(m.d_state); return TAMCMC_E_NOMEM; }
    if (hipMalloc(&m.d_sum, twl_scratch_bytes(nw, (size_t)s->B)) != hipSuccess) {
        (void)hipGetLastError(); (void)hipFree(m.d_state); (void)hipFree(m.d_heap);
        return TAMCMC_E_NOMEM;
    }
    m.body = reinterpret_cast<double *>(m.d_state);
    m.elpd = m.body + 3 * nw;
    m.khat = m.elpd + nw;
    m.cutoff = m.khat + nw;
    m.cnt.d = reinterpret_cast<long long *>(m.cutoff + nw);
    m.tail_len = reinterpret_cast<int32_t *>(m.cnt.d + 4);
    m.on = true;
    s->wloo = m;
    c->enq_seq++;
    if (wloo_pass_clear(s) != TAMCMC_OK) { (void)hipStreamSynchronize(c->stream); wloo_free(s); return TAMCMC_E_HIP; }
    if (n_windows) *n_windows = (int32_t)nw;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_wloo_result(tamcmc_summary *s, tamcmc_summary_wloo_totals *totals, double *elpd_lwo, double *pareto_k,
                                          double *cutoff, int32_t *tail_len, int64_t *first_bin, int64_t *last_bin)
{
    if (!s || !s->wloo.on) return TAMCMC_E_INVALID;
    int rc = summary_enter(s);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = s->c;
    TmWlooMode &m = s->wloo;
    c->enq_seq++;
    bool complete = false;
    rc = pass_complete(m, &complete);
    if (rc != TAMCMC_OK) return rc;
    if (!complete) {                                                    // not the fold pass's samples: the pass is discarded
        rc = wloo_pass_clear(s);
        return rc != TAMCMC_OK ? rc : TAMCMC_E_INVALID;
    }
    const TmLooArgs a = wloo_finalize_args(s);
    TmLooSums f;
    rc = loo_collect(s, (size_t)m.n_windows, m.elpd, m.tail_len, m.n_used,
                     [&] { return timed_launch(s, s->timer, "summary wloo finalize", [&] { return tm_launch_loo_finalize(a, c->stream); }); },
                     elpd_lwo, pareto_k, cutoff, tail_len, &f);
    if (rc != TAMCMC_OK) return rc;
    for (long long w = 0; w < m.n_windows; w++) {
        if (first_bin) first_bin[w] = (int64_t)tmw_begin(w, m.W, m.first);
        if (last_bin) last_bin[w] = (int64_t)tmw_end(w, m.W, m.first, c->L.Nx) - 1;
    }
    if (totals) {
        totals->n_used = m.n_used;
        totals->n_rejected = m.n_rejected;
        totals->n_windows = m.n_windows; totals->W = m.W; totals->first = m.first;
        totals->elpd_lwo = f.elpd;
        totals->p_lwo = f.p;
        totals->k_max = f.k_max;
        totals->n_k_high = f.n_high;
        totals->n_k_inf = f.n_inf;
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_wloo_end(tamcmc_summary *s)
{
    if (!s || !s->wloo.on) return TAMCMC_E_INVALID;
    const int rc = summary_enter(s);
    if (rc == TAMCMC_OK) wloo_free(s);
    return rc;
}

extern "C" int tamcmc_summary_wloo_pit_begin(tamcmc_summary *s)
{
    if (!s || !s->wloo.on || s->wloo.pit) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = s->c;
    TmWlooMode &m = s->wloo;
    const bool chi = c->L.likelihood_case == 0;
    if (chi && !(c->L.like_p >= 1.0 && c->L.like_p <= (double)TAMCMC_SUMMARY_WINDOW_MAX_SHAPE && (int)c->L.like_p * m.W <= TAMCMC_SUMMARY_WINDOW_MAX_SHAPE))
        return TAMCMC_E_INVALID;
    int rc = summary_enter(s);
    if (rc != TAMCMC_OK) return rc;
    bool complete = false;
    rc = pass_complete(m, &complete);
    if (rc != TAMCMC_OK) return rc;
    if (!complete) return TAMCMC_E_INVALID;                             // the pass under way stays as it is
    const size_t nw = (size_t)m.n_windows;
    double *d_lw = nullptr, *d_tails = nullptr;
    char *d_pit = nullptr;
    if (hipMalloc(&d_lw, twl_lw_bytes(nw, (size_t)(m.cap - 1))) != hipSuccess) { (void)hipGetLastError(); return TAMCMC_E_NOMEM; }
    if (hipMalloc(&d_pit, twl_pit_state_bytes(nw)) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(d_lw); return TAMCMC_E_NOMEM; }
    if (hipMalloc(&d_tails, 2 * twl_scratch_bytes(nw, (size_t)s->B)) != hipSuccess) {
        (void)hipGetLastError(); (void)hipFree(d_lw); (void)hipFree(d_pit);
        return TAMCMC_E_NOMEM;
    }
    m.d_lw = d_lw; m.d_pit = d_pit; m.d_tails = d_tails;
    m.pit_sums = reinterpret_cast<double *>(d_pit);
    m.pit_xmax = m.pit_sums + (size_t)TM_LOOPIT_NSTATE * nw;
    m.pit_c = m.pit_xmax + nw;
    m.pit_cnt.d = reinterpret_cast<long long *>(m.pit_c + nw);
    m.pit_cnt.parity = 0;
    m.pit_first = reinterpret_cast<int32_t *>(m.pit_cnt.d + 4);
    m.pit_flag = m.pit_first + nw;
    int f = m.first, len[3];
    (void)tmw_partition((long long)c->L.Nx, m.W, &f, len);
    for (int k = 0; k < 3; k++) m.shape[k] = tmw_shape(len[k], m.p);
    c->enq_seq++;
    const TmLooPitArgs a = wloo_prepare_args(s);
    rc = timed_launch(s, s->timer, "summary wloo pit prepare", [&] { return tm_launch_loopit_prepare(a, c->stream); });
    if (rc == TAMCMC_OK) rc = wloo_pit_pass_clear(s);
    if (rc == TAMCMC_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = TAMCMC_E_HIP;
    if (rc != TAMCMC_OK) {              // (a launch that was refused wrote nothing: the top sets are as the LOO pass left them)
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(d_lw); (void)hipFree(d_pit); (void)hipFree(d_tails);
        m.d_lw = nullptr; m.d_pit = nullptr; m.d_tails = nullptr;
        return rc;
    }
    m.pit = true;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_wloo_pit_result(tamcmc_summary *s, tamcmc_summary_loo_pit_totals *totals, double *loo_pit, double *loo_log_cdf,
                                              double *loo_log_sf, double *is_ess, double *log_wsum)
{
    if (!s || !s->wloo.on || !s->wloo.pit) return TAMCMC_E_INVALID;
    int rc = summary_enter(s);
    if (rc != TAMCMC_OK) return rc;
    TmWlooMode &m = s->wloo;
    s->c->enq_seq++;
    long long cnt[2] = {0, 0};
    int32_t flag = 0;
    rc = m.pit_cnt.read(cnt);
    if (rc != TAMCMC_OK) return rc;
    TM_HIP(hipMemcpy(&flag, m.pit_flag, sizeof flag, hipMemcpyDeviceToHost));
    if (cnt[0] != m.n_used || cnt[1] != m.n_rejected || flag != 0) {    // not the LOO pass's samples: the PIT pass is discarded
        rc = wloo_pit_pass_clear(s);
        return rc != TAMCMC_OK ? rc : TAMCMC_E_INVALID;
    }
    return loopit_collect(m.pit_sums, (size_t)m.n_windows, m.n_used, m.n_rejected, totals, loo_pit, loo_log_cdf, loo_log_sf, is_ess, log_wsum);
}

extern "C" int tamcmc_summary_wloo_pit_kernel_time(tamcmc_summary *s, double *total_ms, int64_t *launches)
{
    if (!s || !total_ms || !launches || !s->wloo.on || !s->wloo.pit || s->c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(s->c->device));
    TM_HIP(tm_ctx_stream_sync(s->c));
    return s->wpit_timer.total(total_ms, launches);
}

// ---- posterior predictive check (tamcmc_predictive.h) ----

// A check is enabled on an object that holds no samples yet (otherwise: reset first).  Opens both _enable functions.
static int summary_enter_empty(tamcmc_summary *s)
{
    long long cnt[2] = {0, 0};
    const int rc = summary_enter(s, cnt);
    return rc != TAMCMC_OK ? rc : (cnt[0] != 0 || cnt[1] != 0 ? TAMCMC_E_INVALID : TAMCMC_OK);
}

extern "C" int tamcmc_summary_predictive_enable(tamcmc_summary *s)
{
    if (!s || s->pred.on || active_mode(s)) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = s->c;
    const bool chi = c->L.likelihood_case == 0;
    if (chi && !(c->L.like_p >= 1.0 && c->L.like_p <= (double)TAMCMC_SUMMARY_PREDICTIVE_MAX_P)) return TAMCMC_E_INVALID;
    const int rc = summary_enter_empty(s);
    if (rc != TAMCMC_OK) return rc;
    TmPredictive &m = s->pred;
    const size_t bytes = (size_t)TM_PRED_NSTATE * (size_t)c->L.Nx * sizeof(double);
    if (hipMalloc(&m.d_state, bytes) != hipSuccess) { (void)hipGetLastError(); m.d_state = nullptr; return TAMCMC_E_NOMEM; }
    m.p = chi ? (int)c->L.like_p : 1;
    m.nterms = tmp_series_terms(m.p);
    m.lf_pm1 = tmp_log_factorial(m.p - 1);
    m.lf_p = tmp_log_factorial(m.p);
    c->enq_seq++;
    if (hipMemsetAsync(m.d_state, 0, bytes, c->stream) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(m.d_state);
        m.d_state = nullptr;
        return TAMCMC_E_HIP;
    }
    m.on = true;
    return TAMCMC_OK;
}

// What the per-bin and the windowed check share on the host: from the state st[TM_PRED_NSTATE][m] of m items (bins or
// windows) and n accepted samples, the four arrays (any may be NULL) and the totals over the items, in item order.
struct TmTailTotals {
    long long n_used, n_rejected;
    double ks_D, min_log_sf, min_log_cdf;
    int64_t at_min_log_sf, at_min_log_cdf;
    int64_t pit_hist[TAMCMC_SUMMARY_PIT_CELLS];
};

static int tails_finish(const std::vector<double> &st, const size_t m, const long long n, double *pit, double *log_cdf, double *log_sf,
                        double *mean_resid, TmTailTotals *out)
{
    const double nan = std::nan("");
    std::vector<double> u;
    try { u.reserve(m); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    TmTailTotals t{};
    t.ks_D = nan; t.min_log_sf = nan; t.min_log_cdf = nan;
    t.at_min_log_sf = -1; t.at_min_log_cdf = -1;
    for (size_t i = 0; i < m; i++) {
        const double lc = tmp_lse_result(st[TM_PRED_CDF_A * m + i], st[TM_PRED_CDF_R * m + i], st[TM_PRED_CDF_C * m + i], n);
        const double ls = tmp_lse_result(st[TM_PRED_SF_A * m + i], st[TM_PRED_SF_R * m + i], st[TM_PRED_SF_C * m + i], n);
        const double pv = n >= 1 ? (lc < ls ? std::exp(lc) : -std::expm1(ls)) : nan;       // from the smaller tail
        if (pit) pit[i] = pv;
        if (log_cdf) log_cdf[i] = lc;
        if (log_sf) log_sf[i] = ls;
        if (mean_resid) mean_resid[i] = n >= 1 ? st[TM_PRED_MEAN_RESID * m + i] : nan;
        if (n < 1) continue;
        if (t.at_min_log_sf < 0 ? !std::isnan(ls) : ls < t.min_log_sf) { t.min_log_sf = ls; t.at_min_log_sf = (int64_t)i; }      // the first item wins a tie
        if (t.at_min_log_cdf < 0 ? !std::isnan(lc) : lc < t.min_log_cdf) { t.min_log_cdf = lc; t.at_min_log_cdf = (int64_t)i; }
        if (std::isnan(pv)) continue;
        t.pit_hist[tm_pit_cell(pv)]++;
        u.push_back(pv);
    }
    if (!u.empty()) t.ks_D = tm_ks_uniform(u);
    *out = t;
    return TAMCMC_OK;
}

// the fold pass's counts: frozen copies while a mode is on (its passes touch neither check's state)
static int fold_counts(const tamcmc_summary *s, long long cnt[2])
{
    const TmMode *m = active_mode(s);
    if (!m) return s->cnt.read(cnt);
    cnt[0] = m->n_used; cnt[1] = m->n_rejected;
    return TAMCMC_OK;
}

// _predictive_result, _window_result and _scan_result once their check is known to be on: d_state[TM_PRED_NSTATE][m], m bins,
// windows or positions; pitch: the doubles from one state word's block to the next, where that is not m (0: m)
static int tails_result(tamcmc_summary *s, const double *d_state, const size_t m, double *pit, double *log_cdf, double *log_sf,
                        double *mean_resid, TmTailTotals *out, const size_t pitch = 0)
{
    int rc = summary_enter(s);
    if (rc != TAMCMC_OK) return rc;
    long long cnt[2] = {0, 0};
    std::vector<double> st;
    try { st.resize(TM_PRED_NSTATE * m); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    rc = fold_counts(s, cnt);
    if (rc != TAMCMC_OK) return rc;
    if (pitch == 0 || pitch == m) TM_HIP(hipMemcpy(st.data(), d_state, st.size() * sizeof(double), hipMemcpyDeviceToHost));
    else TM_HIP(hipMemcpy2D(st.data(), m * sizeof(double), d_state, pitch * sizeof(double), m * sizeof(double), TM_PRED_NSTATE, hipMemcpyDeviceToHost));
    rc = tails_finish(st, m, cnt[0], pit, log_cdf, log_sf, mean_resid, out);
    out->n_used = cnt[0]; out->n_rejected = cnt[1];
    return rc;
}

extern "C" int tamcmc_summary_predictive_result(tamcmc_summary *s, tamcmc_summary_predictive_totals *totals,
                                                double *pit, double *log_cdf, double *log_sf, double *mean_resid)
{
    if (!s || !s->pred.on) return TAMCMC_E_INVALID;
    TmTailTotals f;
    const int rc = tails_result(s, s->pred.d_state, (size_t)s->c->L.Nx, pit, log_cdf, log_sf, mean_resid, &f);
    if (rc != TAMCMC_OK) return rc;
    if (totals) {
        tamcmc_summary_predictive_totals t{};
        t.n_used = f.n_used; t.n_rejected = f.n_rejected;
        t.ks_D = f.ks_D; t.min_log_sf = f.min_log_sf; t.min_log_cdf = f.min_log_cdf;
        t.bin_min_log_sf = f.at_min_log_sf; t.bin_min_log_cdf = f.at_min_log_cdf;
        std::memcpy(t.pit_hist, f.pit_hist, sizeof(t.pit_hist));
        *totals = t;
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_predictive_kernel_time(tamcmc_summary *s, double *total_ms, int64_t *launches)
{
    if (!s || !total_ms || !launches || !s->pred.on || s->c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(s->c->device));
    TM_HIP(tm_ctx_stream_sync(s->c));
    return s->pred.timer.total(total_ms, launches);
}

// ---- windowed posterior predictive check (tamcmc_window.h) ----

extern "C" int tamcmc_summary_window_enable(tamcmc_summary *s, int32_t W, int32_t first, int32_t *n_windows)
{
    if (!s || W < 1 || W > TAMCMC_SUMMARY_WINDOW_MAX_BINS || first < 0 || first > W) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = s->c;
    if (s->win.on || active_mode(s)) return TAMCMC_E_INVALID;
    const bool chi = c->L.likelihood_case == 0;
    if (chi && !(c->L.like_p >= 1.0 && c->L.like_p <= (double)TAMCMC_SUMMARY_WINDOW_MAX_SHAPE && (int)c->L.like_p * W <= TAMCMC_SUMMARY_WINDOW_MAX_SHAPE))
        return TAMCMC_E_INVALID;
    const int rc = summary_enter_empty(s);
    if (rc != TAMCMC_OK) return rc;
    TmWindow &m = s->win;
    int f = first, len[3];
    const long long nw = tmw_partition((long long)c->L.Nx, W, &f, len);
    const size_t state_bytes = (size_t)TM_PRED_NSTATE * (size_t)nw * sizeof(double);
    const size_t scratch_bytes = 3 * (size_t)s->B * (size_t)nw * sizeof(double);
    double *d_state = nullptr, *d_scratch = nullptr;
    if (hipMalloc(&d_state, state_bytes) != hipSuccess) { (void)hipGetLastError(); return TAMCMC_E_NOMEM; }
    if (hipMalloc(&d_scratch, scratch_bytes) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(d_state); return TAMCMC_E_NOMEM; }
    c->enq_seq++;
    if (hipMemsetAsync(d_state, 0, state_bytes, c->stream) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(d_state); (void)hipFree(d_scratch);
        return TAMCMC_E_HIP;
    }
    m.d_state = d_state; m.d_scratch = d_scratch;
    m.W = W; m.first = f; m.n_windows = (int)nw;
    m.p = chi ? (int)c->L.like_p : 1;
    for (int k = 0; k < 3; k++) m.shape[k] = tmw_shape(len[k], m.p);
    m.on = true;
    if (n_windows) *n_windows = (int32_t)nw;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_window_result(tamcmc_summary *s, tamcmc_summary_window_totals *totals,
                                            double *pit, double *log_cdf, double *log_sf, double *mean_resid)
{
    if (!s || !s->win.on) return TAMCMC_E_INVALID;
    const size_t nw = (size_t)s->win.n_windows;
    TmTailTotals f;
    const int rc = tails_result(s, s->win.d_state, nw, pit, log_cdf, log_sf, mean_resid, &f);
    if (rc != TAMCMC_OK) return rc;
    if (totals) {
        tamcmc_summary_window_totals t{};
        t.n_used = f.n_used; t.n_rejected = f.n_rejected;
        t.n_windows = (int64_t)nw; t.W = s->win.W; t.first = s->win.first;
        t.ks_D = f.ks_D; t.min_log_sf = f.min_log_sf; t.min_log_cdf = f.min_log_cdf;
        t.win_min_log_sf = f.at_min_log_sf; t.win_min_log_cdf = f.at_min_log_cdf;
        std::memcpy(t.pit_hist, f.pit_hist, sizeof(t.pit_hist));
        *totals = t;
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_window_kernel_time(tamcmc_summary *s, double *total_ms, int64_t *launches)
{
    if (!s || !total_ms || !launches || !s->win.on || s->c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(s->c->device));
    TM_HIP(tm_ctx_stream_sync(s->c));
    return s->win.timer.total(total_ms, launches);
}

// ---- sliding-window predictive scan (tamcmc_scan.h) ----

extern "C" int tamcmc_summary_scan_enable(tamcmc_summary *s, int32_t n_widths, const int32_t *W)
{
    if (!s || !W || n_widths < 1 || n_widths > TAMCMC_SUMMARY_SCAN_MAX_WIDTHS) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = s->c;
    if (s->scan.on || active_mode(s)) return TAMCMC_E_INVALID;
    for (int k = 0; k < n_widths; k++)
        if (W[k] < 1 || W[k] > TAMCMC_SUMMARY_WINDOW_MAX_BINS || W[k] > c->L.Nx || (k > 0 && W[k] <= W[k - 1])) return TAMCMC_E_INVALID;
    const bool chi = c->L.likelihood_case == 0;
    if (chi && !(c->L.like_p >= 1.0 && c->L.like_p <= (double)TAMCMC_SUMMARY_WINDOW_MAX_SHAPE &&
                 (int)c->L.like_p * W[n_widths - 1] <= TAMCMC_SUMMARY_WINDOW_MAX_SHAPE))
        return TAMCMC_E_INVALID;
    const int rc = summary_enter_empty(s);
    if (rc != TAMCMC_OK) return rc;
    TmScan m;
    m.K = n_widths;
    for (int k = 0; k < n_widths; k++) m.W[k] = W[k];
    m.total = tmsc_layout((long long)c->L.Nx, m.K, m.W, m.off);
    m.C = (int)tmsc_chunk((long long)s->B, m.total);
    m.p = chi ? (int)c->L.like_p : 1;
    for (int k = 0; k < n_widths; k++) m.shape[k] = tmw_shape(m.W[k], m.p);
    const size_t state_bytes = (size_t)TM_PRED_NSTATE * (size_t)m.total * sizeof(double);
    const size_t scratch_bytes = 3 * (size_t)m.C * (size_t)m.total * sizeof(double);
    if (hipMalloc(&m.d_state, state_bytes) != hipSuccess) { (void)hipGetLastError(); return TAMCMC_E_NOMEM; }
    if (hipMalloc(&m.d_scratch, scratch_bytes) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(m.d_state); return TAMCMC_E_NOMEM; }
    c->enq_seq++;
    if (hipMemsetAsync(m.d_state, 0, state_bytes, c->stream) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(m.d_state); (void)hipFree(m.d_scratch);
        return TAMCMC_E_HIP;
    }
    m.on = true;
    s->scan = m;
    return TAMCMC_OK;
}

// what _scan_result and _scan_regions share: width k's four arrays (any may be NULL) and its totals
static int scan_width_result(tamcmc_summary *s, int32_t k, double *pit, double *log_cdf, double *log_sf, double *mean_resid, TmTailTotals *f)
{
    if (!s || !s->scan.on || k < 0 || k >= s->scan.K) return TAMCMC_E_INVALID;
    const TmScan &m = s->scan;
    const size_t n_pos = (size_t)tmsc_positions((long long)s->c->L.Nx, m.W[k]);
    return tails_result(s, m.d_state + m.off[k], n_pos, pit, log_cdf, log_sf, mean_resid, f, (size_t)m.total);
}

extern "C" int tamcmc_summary_scan_result(tamcmc_summary *s, int32_t k, tamcmc_summary_scan_totals *totals,
                                          double *pit, double *log_cdf, double *log_sf, double *mean_resid)
{
    TmTailTotals f;
    const int rc = scan_width_result(s, k, pit, log_cdf, log_sf, mean_resid, &f);
    if (rc != TAMCMC_OK) return rc;
    if (totals) {
        tamcmc_summary_scan_totals t{};
        t.n_used = f.n_used; t.n_rejected = f.n_rejected;
        t.W = s->scan.W[k]; t.n_positions = (int64_t)tmsc_positions((long long)s->c->L.Nx, s->scan.W[k]);
        t.min_log_sf = f.min_log_sf; t.min_log_cdf = f.min_log_cdf;
        t.pos_min_log_sf = f.at_min_log_sf; t.pos_min_log_cdf = f.at_min_log_cdf;
        *totals = t;
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_scan_regions(tamcmc_summary *s, int32_t k, int32_t which, double log_below,
                                           int32_t max_regions, tamcmc_summary_scan_region *regions, int32_t *n_regions)
{
    if (!s || !s->scan.on || k < 0 || k >= s->scan.K || which < 0 || which > 1 || !n_regions || max_regions < 0 ||
        (max_regions > 0 && !regions) || log_below >= 0.0)
        return TAMCMC_E_INVALID;                    // (a NaN line passes: the default)
    const long long nx = (long long)s->c->L.Nx;
    const int W = s->scan.W[k];
    const long long n_pos = tmsc_positions(nx, W);
    std::vector<double> v, mr;
    std::vector<TmScanRegion> found;
    const long long room = max_regions < n_pos ? max_regions : n_pos;          // (there are at most n_pos regions)
    try { v.resize((size_t)n_pos); mr.resize((size_t)n_pos); found.resize((size_t)room); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    TmTailTotals f;
    const int rc = scan_width_result(s, k, nullptr, which == 1 ? v.data() : nullptr, which == 0 ? v.data() : nullptr, mr.data(), &f);
    if (rc != TAMCMC_OK) return rc;
    const double line = std::isnan(log_below) ? tmsc_default_line(W, nx) : log_below;
    const long long count = tmsc_regions(v.data(), mr.data(), n_pos, W, line, room, found.data());
    for (long long i = 0; i < count && i < room; i++) {
        const TmScanRegion &r = found[(size_t)i];
        tamcmc_summary_scan_region o{};
        o.pos_first = r.pos_first; o.pos_last = r.pos_last; o.bin_first = r.bin_first; o.bin_last = r.bin_last; o.pos_min = r.pos_min;
        o.min_log = r.min_log; o.mean_resid_at_min = r.mean_resid_at_min;
        regions[i] = o;
    }
    *n_regions = (int32_t)count;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_scan_kernel_time(tamcmc_summary *s, double *total_ms, int64_t *launches)
{
    if (!s || !total_ms || !launches || !s->scan.on || s->c->armed) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(s->c->device));
    TM_HIP(tm_ctx_stream_sync(s->c));
    return s->scan.timer.total(total_ms, launches);
}

// ---- effective sample size, MCSE and split R-hat (tamcmc_ess.h) ----

extern "C" int tamcmc_summary_ess_begin(tamcmc_summary *s, int32_t max_lag, int32_t *lag_used)
{
    if (!s || max_lag < 0 || max_lag > TAMCMC_SUMMARY_ESS_MAX_LAG) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = s->c;
    if (active_mode(s)) return TAMCMC_E_INVALID;
    long long cnt[2] = {0, 0};
    const int rc = summary_enter(s, cnt);
    if (rc != TAMCMC_OK) return rc;
    if (cnt[0] < 4) return TAMCMC_E_INVALID;
    const size_t nx = (size_t)c->L.Nx;
    std::vector<double> lse;
    try { lse.resize(2 * nx); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    TM_HIP(hipMemcpy(lse.data(), s->d_state + (size_t)TM_SUM_LSE_A * nx, 2 * nx * sizeof(double), hipMemcpyDeviceToHost));   // a | r
    const double dn = (double)cnt[0];
    for (size_t i = 0; i < nx; i++) lse[i] = tm_lppd(lse[i], lse[nx + i], dn);          // as tamcmc_summary_result
    TmEssMode m;
    m.L = tme_lag_limit(max_lag, cnt[0]);
    m.R = tme_ring_slots(m.L);
    m.n_used = cnt[0]; m.n_rejected = cnt[1];
    const size_t state_bytes = (TM_ESS_NHALF + 1 + 4) * nx * sizeof(double) + 4 * sizeof(long long) + 2 * nx * sizeof(int32_t);
    if (hipMalloc(&m.d_state, state_bytes) != hipSuccess) { (void)hipGetLastError(); return TAMCMC_E_NOMEM; }
    if (hipMalloc(&m.d_acc, 2 * (size_t)(m.L + 1) * nx * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(m.d_state); return TAMCMC_E_NOMEM; }
    if (hipMalloc(&m.d_ring, 2 * (size_t)m.R * nx * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError(); (void)hipFree(m.d_state); (void)hipFree(m.d_acc);
        return TAMCMC_E_NOMEM;
    }
    m.half = reinterpret_cast<double *>(m.d_state);
    m.lppd = m.half + TM_ESS_NHALF * nx;
    m.tau = m.lppd + nx;
    m.ess = m.tau + 2 * nx;
    m.cnt.d = reinterpret_cast<long long *>(m.ess + 2 * nx);
    m.cut = reinterpret_cast<int32_t *>(m.cnt.d + 4);
    m.on = true;
    s->ess = m;
    c->enq_seq++;
    if (hipMemcpy(m.lppd, lse.data(), nx * sizeof(double), hipMemcpyHostToDevice) != hipSuccess || ess_pass_clear(s) != TAMCMC_OK) {
        (void)hipStreamSynchronize(c->stream);
        ess_free(s);
        return TAMCMC_E_HIP;
    }
    if (lag_used) *lag_used = m.L;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_ess_result(tamcmc_summary *s, tamcmc_summary_ess_totals *totals,
                                         double *ess_M, double *tau_M, double *mcse_M, double *rhat_M, int32_t *cut_M,
                                         double *ess_l, double *r_eff, int32_t *cut_l)
{
    if (!s || !s->ess.on) return TAMCMC_E_INVALID;
    int rc = summary_enter(s);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = s->c;
    TmEssMode &m = s->ess;
    c->enq_seq++;
    bool complete = false;
    rc = pass_complete(m, &complete);
    if (rc != TAMCMC_OK) return rc;
    if (!complete) {                                                    // not the fold pass's samples: the pass is discarded
        rc = ess_pass_clear(s);
        return rc != TAMCMC_OK ? rc : TAMCMC_E_INVALID;
    }
    const size_t nx = (size_t)c->L.Nx;
    std::vector<double> out, half, m2;
    std::vector<int32_t> cut;
    try { out.resize(4 * nx); half.resize(TM_ESS_NHALF * nx); m2.resize(nx); cut.resize(2 * nx); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    const TmEssArgs a = ess_args(s);
    rc = timed_launch(s, s->timer, "summary ess finish", [&] { return tm_launch_ess_finish(a, c->stream); });
    if (rc != TAMCMC_OK) return rc;
    TM_HIP(hipMemcpyAsync(out.data(), m.tau, 4 * nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));        // tau[2] | ess[2]
    TM_HIP(hipMemcpyAsync(cut.data(), m.cut, 2 * nx * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    TM_HIP(hipMemcpyAsync(half.data(), m.half, half.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TM_HIP(hipMemcpyAsync(m2.data(), s->d_state + (size_t)TM_SUM_M2_M * nx, nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TM_HIP(hipStreamSynchronize(c->stream));
    const double dn = (double)m.n_used, nan = std::nan("");
    const double *tau = out.data(), *ess = out.data() + 2 * nx;
    tamcmc_summary_ess_totals t{};
    t.n_used = m.n_used; t.n_rejected = m.n_rejected; t.lag = m.L;
    t.min_ess_M = nan; t.min_ess_l = nan; t.max_rhat = nan;
    t.bin_min_ess_M = -1; t.bin_min_ess_l = -1; t.bin_max_rhat = -1;
    for (size_t i = 0; i < nx; i++) {
        const double eM = ess[i], el = ess[nx + i];
        const double var_M = m2[i] / (dn - 1.0);                        // the frozen var_M of tamcmc_summary_result
        const double rh = tme_rhat(half[TM_ESS_H1_MEAN * nx + i], half[TM_ESS_H1_M2 * nx + i], half[TM_ESS_H2_MEAN * nx + i],
                                   half[TM_ESS_H2_M2 * nx + i], m.n_used / 2);
        if (ess_M) ess_M[i] = eM;
        if (tau_M) tau_M[i] = tau[i];
        if (mcse_M) mcse_M[i] = std::sqrt(var_M / eM);
        if (rhat_M) rhat_M[i] = rh;
        if (cut_M) cut_M[i] = cut[i];
        if (ess_l) ess_l[i] = el;
        if (r_eff) r_eff[i] = el / dn;
        if (cut_l) cut_l[i] = cut[nx + i];
        // the first bin wins a tie, a NaN is skipped
        if (t.bin_min_ess_M < 0 ? !std::isnan(eM) : eM < t.min_ess_M) { t.min_ess_M = eM; t.bin_min_ess_M = (int64_t)i; }
        if (t.bin_min_ess_l < 0 ? !std::isnan(el) : el < t.min_ess_l) { t.min_ess_l = el; t.bin_min_ess_l = (int64_t)i; }
        if (t.bin_max_rhat < 0 ? !std::isnan(rh) : rh > t.max_rhat) { t.max_rhat = rh; t.bin_max_rhat = (int64_t)i; }
        if (cut[i] == m.L + 1) t.n_truncated_M++;
        if (cut[nx + i] == m.L + 1) t.n_truncated_l++;
        if (rh > 1.01) t.n_rhat_high++;
    }
    if (totals) *totals = t;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_ess_acov(tamcmc_summary *s, int32_t which, double *acov)
{
    if (!s || !s->ess.on || !acov || which < 0 || which > 1) return TAMCMC_E_INVALID;
    bool complete = false;
    int rc = summary_enter(s);
    if (rc == TAMCMC_OK) rc = pass_complete(s->ess, &complete);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = s->c;
    if (!complete) return TAMCMC_E_INVALID;                             // (the pass stays: tamcmc_summary_ess_result discards it)
    const size_t len = (size_t)(s->ess.L + 1) * (size_t)c->L.Nx;
    TM_HIP(hipMemcpy(acov, s->ess.d_acc + (size_t)which * len, len * sizeof(double), hipMemcpyDeviceToHost));
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_ess_end(tamcmc_summary *s)
{
    if (!s || !s->ess.on) return TAMCMC_E_INVALID;
    const int rc = summary_enter(s);
    if (rc == TAMCMC_OK) ess_free(s);
    return rc;
}

// ---- ESS and MCSE of the credible-band edges (tamcmc_bandess.h) ----

extern "C" int tamcmc_summary_bandess_begin(tamcmc_summary *s, int32_t K, const double *thr, int32_t max_lag, int32_t *lag_used)
{
    if (!s || K < 1 || K > TAMCMC_SUMMARY_MAX_QUANTILES || !thr || max_lag < 0 || max_lag > TAMCMC_SUMMARY_ESS_MAX_LAG) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = s->c;
    if (active_mode(s)) return TAMCMC_E_INVALID;
    long long cnt[2] = {0, 0};
    const int rc = summary_enter(s, cnt);
    if (rc != TAMCMC_OK) return rc;
    if (cnt[0] < 4 || cnt[0] >= TM_BANDESS_MAX_N) return TAMCMC_E_INVALID;      // (2^20 samples and more: thin the chain)
    const size_t nx = (size_t)c->L.Nx, k = (size_t)K;
    TmBandMode m;
    m.K = K;
    m.L = tme_lag_limit(max_lag, cnt[0]);
    m.RW = tmb_ring_words(m.L);
    m.HW = tmb_head_words(m.L);
    m.n_used = cnt[0]; m.n_rejected = cnt[1];
    const size_t state_bytes = 3 * k * nx * sizeof(double) + 4 * sizeof(long long) + k * nx * sizeof(int32_t);
    if (hipMalloc(&m.d_state, state_bytes) != hipSuccess) { (void)hipGetLastError(); return TAMCMC_E_NOMEM; }
    if (hipMalloc(&m.d_C, k * (size_t)(m.L + 1) * nx * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(m.d_state); return TAMCMC_E_NOMEM; }
    if (hipMalloc(&m.d_bits, band_bits_bytes(m, nx)) != hipSuccess) {
        (void)hipGetLastError(); (void)hipFree(m.d_state); (void)hipFree(m.d_C);
        return TAMCMC_E_NOMEM;
    }
    if (hipMalloc(&m.d_work, (size_t)(m.L + 1) * nx * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError(); (void)hipFree(m.d_state); (void)hipFree(m.d_C); (void)hipFree(m.d_bits);
        return TAMCMC_E_NOMEM;
    }
    m.head = m.d_bits + k * (size_t)m.RW * nx;
    m.thr = reinterpret_cast<double *>(m.d_state);
    m.tau = m.thr + k * nx;
    m.ess = m.tau + k * nx;
    m.cnt.d = reinterpret_cast<long long *>(m.ess + k * nx);
    m.cut = reinterpret_cast<int32_t *>(m.cnt.d + 4);
    m.on = true;
    s->band = m;
    c->enq_seq++;
    if (hipMemcpy(m.thr, thr, k * nx * sizeof(double), hipMemcpyHostToDevice) != hipSuccess || band_pass_clear(s) != TAMCMC_OK) {
        (void)hipStreamSynchronize(c->stream);
        band_free(s);
        return TAMCMC_E_HIP;
    }
    if (lag_used) *lag_used = m.L;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_bandess_result(tamcmc_summary *s, tamcmc_summary_bandess_totals *totals,
                                             int32_t *count_le, double *p_hat, double *ess, double *tau, double *mcse_p, int32_t *cut)
{
    if (!s || !s->band.on) return TAMCMC_E_INVALID;
    int rc = summary_enter(s);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = s->c;
    TmBandMode &m = s->band;
    c->enq_seq++;
    bool complete = false;
    rc = pass_complete(m, &complete);
    if (rc != TAMCMC_OK) return rc;
    if (!complete) {                                                    // not the fold pass's samples: the pass is discarded
        rc = band_pass_clear(s);
        return rc != TAMCMC_OK ? rc : TAMCMC_E_INVALID;
    }
    const size_t nx = (size_t)c->L.Nx, K = (size_t)m.K;
    std::vector<double> out;
    std::vector<int32_t> cutv;
    std::vector<uint32_t> N;
    try { out.resize(2 * K * nx); cutv.resize(K * nx); N.resize(K * nx); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    for (size_t j = 0; j < K; j++) {                                    // one threshold at a time: they share the work column
        TmBandArgs a = band_args(s);
        a.j = (int32_t)j;
        rc = timed_launch(s, s->timer, "summary bandess finish", [&] { return tm_launch_bandess_finish(a, c->stream); });
        if (rc != TAMCMC_OK) return rc;
        TM_HIP(hipMemcpyAsync(N.data() + j * nx, m.d_C + j * (size_t)(m.L + 1) * nx, nx * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));   // N = C_0
    }
    TM_HIP(hipMemcpyAsync(out.data(), m.tau, 2 * K * nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));     // tau[K] | ess[K]
    TM_HIP(hipMemcpyAsync(cutv.data(), m.cut, K * nx * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    TM_HIP(hipStreamSynchronize(c->stream));
    const double dn = (double)m.n_used, nan = std::nan("");
    const double *tauv = out.data(), *essv = out.data() + K * nx;
    tamcmc_summary_bandess_totals t{};
    t.n_used = m.n_used; t.n_rejected = m.n_rejected; t.lag = m.L; t.n_thresholds = m.K;
    for (size_t j = 0; j < TAMCMC_SUMMARY_MAX_QUANTILES; j++) { t.min_ess[j] = nan; t.bin_min_ess[j] = -1; }
    for (size_t j = 0; j < K; j++)
        for (size_t i = 0; i < nx; i++) {
            const size_t at = j * nx + i;
            const double e = essv[at];
            const double p = (double)N[at] / dn;
            const double q = 1.0 - p, pq = p * q;                       // (spelled out: no contraction whatever the flags)
            if (count_le) count_le[at] = (int32_t)N[at];
            if (p_hat) p_hat[at] = p;
            if (ess) ess[at] = e;
            if (tau) tau[at] = tauv[at];
            if (mcse_p) mcse_p[at] = std::sqrt(pq / e);
            if (cut) cut[at] = cutv[at];
            // the first bin wins a tie, a NaN is skipped
            if (t.bin_min_ess[j] < 0 ? !std::isnan(e) : e < t.min_ess[j]) { t.min_ess[j] = e; t.bin_min_ess[j] = (int64_t)i; }
            if (cutv[at] == m.L + 1) t.n_truncated[j]++;
            if (N[at] == 0 || (long long)N[at] == m.n_used) t.n_constant[j]++;
        }
    if (totals) *totals = t;
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_bandess_counts(tamcmc_summary *s, int32_t j, int32_t *C, int64_t *E)
{
    if (!s || !s->band.on || j < 0 || j >= s->band.K) return TAMCMC_E_INVALID;
    bool complete = false;
    int rc = summary_enter(s);
    if (rc == TAMCMC_OK) rc = pass_complete(s->band, &complete);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = s->c;
    if (!complete) return TAMCMC_E_INVALID;                             // (the pass stays: tamcmc_summary_bandess_result discards it)
    const TmBandMode &m = s->band;
    const size_t len = (size_t)(m.L + 1) * (size_t)c->L.Nx;
    if (C) TM_HIP(hipMemcpy(C, m.d_C + (size_t)j * len, len * sizeof(uint32_t), hipMemcpyDeviceToHost));     // (every count is <= n < 2^20)
    if (E) {
        TmBandArgs a = band_args(s);
        a.j = j; a.want_E = 1;
        c->enq_seq++;
        const int hr = tm_launch_bandess_finish(a, c->stream);
        if (hr != 0) return tm_launch_failed("summary bandess counts", hr);
        TM_HIP(hipMemcpyAsync(E, m.d_work, len * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        TM_HIP(hipStreamSynchronize(c->stream));
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_summary_bandess_end(tamcmc_summary *s)
{
    if (!s || !s->band.on) return TAMCMC_E_INVALID;
    const int rc = summary_enter(s);
    if (rc == TAMCMC_OK) band_free(s);
    return rc;
}
