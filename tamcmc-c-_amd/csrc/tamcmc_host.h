// tamcmc_host.h -- internal to csrc/: what the host-side objects of the C ABI (include/tamcmc_accel.h) share.  One source
// file per object: tamcmc_api.cpp the context (struct tamcmc_ctx below), tamcmc_group.cpp the fit groups,
// tamcmc_summary_api.cpp the posterior summaries.  Here: the HIP error text, the helpers every object uses (event polling,
// event-pair timer, pinned buffers, input staging), the context itself, and the functions of tamcmc_api.cpp that groups
// and summaries call.  Groups and summaries read the context's fields directly and write a few of them (after_ev /
// after_owner, enq_seq, groups, summaries): the struct is here anyway, so accessors would only add to this header.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tamcmc_accel.h"
#include "tamcmc_dev.h"

extern thread_local char tm_hip_err[256];   // the text of tamcmc_last_hip_error(): one buffer per thread (tamcmc_api.cpp)

#define TM_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            snprintf(tm_hip_err, sizeof(tm_hip_err), "%s -> %s", #call, hipGetErrorString(e_)); \
            return TAMCMC_E_HIP;                                                             \
        }                                                                                    \
    } while (0)

// hr: what a tm_launch_* function returned (a hipError_t other than hipSuccess)
inline int tm_launch_failed(const char *what, int hr)
{
    snprintf(tm_hip_err, sizeof(tm_hip_err), "%s launch -> %s", what, hipGetErrorString((hipError_t)hr));
    return TAMCMC_E_HIP;
}

// Wait for a recorded event by polling it.  hipStreamSynchronize may park the calling thread on an interrupt; on this
// platform that path showed rare stalls of 1-40 ms after a ~160 us batch (profiles/README.md), and a sampler waits
// thousands of times per second.
inline int tm_poll_event(hipEvent_t ev)
{
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return TAMCMC_OK;
        if (e != hipErrorNotReady) { snprintf(tm_hip_err, sizeof(tm_hip_err), "hipEventQuery -> %s", hipGetErrorString(e)); return TAMCMC_E_HIP; }
        __builtin_ia32_pause();
    }
}

// Timing of selected launches: begin / end record the next pair (start, stop) of a pool of events around a launch,
// total sums the pairs recorded since `used` was last put to zero (the stream must have been waited for).
struct TmTimer {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    int pool(size_t n)            // creating an event costs ~10 us: a caller that is timed itself fills the pool up front
    {
        for (hipEvent_t e; ev.size() < n; ev.push_back(e)) TM_HIP(hipEventCreate(&e));
        return TAMCMC_OK;
    }
    int begin(hipStream_t stream) { const int rc = pool(used + 2); if (rc == TAMCMC_OK) TM_HIP(hipEventRecord(ev[used], stream)); return rc; }
    int end(hipStream_t stream) { TM_HIP(hipEventRecord(ev[used + 1], stream)); used += 2; return TAMCMC_OK; }
    int total(double *total_ms, int64_t *launches) const
    {
        double t = 0.0;
        for (size_t i = 0; i + 1 < used; i += 2) {
            float ms = 0.f;
            TM_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            t += (double)ms;
        }
        *total_ms = t;
        *launches = (int64_t)(used / 2);
        return TAMCMC_OK;
    }
    void destroy() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); ev.clear(); used = 0; }
};

// A pinned host buffer and the device's side of it: the device view of the same memory (mapped, coherent: kernels read
// and write it over PCIe, no copy-engine round trip), a device twin of the same size (copied to and from), or nothing.
enum TmPinKind { TM_PIN_MAPPED, TM_PIN_TWIN, TM_PIN_HOST };
struct TmPinned {
    char *h = nullptr, *d = nullptr;
    size_t cap = 0;               // bytes
    TmPinKind kind = TM_PIN_HOST;
    template <class T> T *host() const { return reinterpret_cast<T *>(h); }
    template <class T> T *dev() const { return reinterpret_cast<T *>(d); }
    bool fits(size_t bytes) const { return bytes <= cap; }
    // Nothing while `bytes` fit; otherwise the memory is freed and `bytes` are allocated.  The freed memory must be idle:
    // an owner with launches or copies under way asks fits() and waits for its stream first.
    int reserve(size_t bytes, TmPinKind k)
    {
        if (fits(bytes)) return TAMCMC_OK;
        release();
        kind = k;
        TM_HIP(hipHostMalloc(reinterpret_cast<void **>(&h), bytes, k == TM_PIN_MAPPED ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault));
        if (k == TM_PIN_MAPPED) TM_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&d), h, 0));
        if (k == TM_PIN_TWIN) TM_HIP(hipMalloc(&d, bytes));
        cap = bytes;
        return TAMCMC_OK;
    }
    void release() { (void)hipHostFree(h); if (kind == TM_PIN_TWIN) (void)hipFree(d); h = d = nullptr; cap = 0; }
};

// The inputs of a host-pointer call into its staging: np doubles of parameter rows, then nc temperature coefficients.
inline void tm_stage_inputs(void *dst, const double *params, size_t np, const double *Tcoefs, size_t nc)
{
    std::memcpy(dst, params, np * sizeof(double));
    std::memcpy(static_cast<double *>(dst) + np, Tcoefs, nc * sizeof(double));
}

struct tamcmc_ctx {
    int device = 0;
    TmLayout L{};
    // Geometry (tamcmc_dev.h): units of 512 bins, cells of 8 units, tiles_l / tiles_g tiles per chain for the likelihood-only
    // and the gradient launch -- functions of the grid alone; a chain's tile BOUNDARIES are chosen by the setup kernel.
    int units = 0, cells = 0;
    int tiles_l = 1, tiles_g = 1;
    int tiles_max = 1;
    int equal_cost = 0;            // TAMCMC_EQUAL_COST=1: per-chain tile boundaries of equal cost instead of equal length
    int prio = 0;                  // TAMCMC_PRIO=1: issue priority by launch rank (s_setprio)
    TmCostModel cost_l{60, 5, 9, TM_TILE_MAXU_L}, cost_g{110, 13, 24, TM_TILE_MAXU};   // (.pad = units per tile at most)   // VALU instructions per bin: c0 + sum(a * ncomp + b) (TAMCMC_COST / TAMCMC_COST_GRAD)
    int last_tiles = 0;            // T of the most recent likelihood-only call (tamcmc_ctx_geometry)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // resident data
    double *d_x2 = nullptr, *d_y = nullptr, *d_lx = nullptr, *d_isig2 = nullptr;   // 2 x, y, log x, 1 / sigma^2
    int nspec = 1;                 // spectra resident in d_y / d_isig2 (blocks of Nx); tamcmc_ctx_set_spectra
    int32_t *d_spec = nullptr;     // [spec_n] chain -> spectrum map (tamcmc_ctx_set_chain_spectrum), or NULL: all chains use spectrum 0
    int spec_n = 0;
    // per-batch buffers (capacity in chains)
    int cap = 0;
    bool cap_grad = false;
    void *d_slab = nullptr;        // one allocation behind every per-batch buffer below (tm_ensure_capacity)
    double *d_params = nullptr, *d_T = nullptr, *d_logL = nullptr, *d_part = nullptr;
    double *d_gmult = nullptr, *d_gnoise = nullptr, *d_hser = nullptr;
    int32_t *d_order = nullptr; int order_mode = 2;
    int fuse = 1;                  // one tile per chain -> prologue and evaluation in one launch (TAMCMC_FUSED=0 disables)
    int32_t *d_status = nullptr, *d_rows = nullptr;
    TmMult *d_mult = nullptr;
    TmNoise *d_noise = nullptr;
    void *d_chain_rec = nullptr, *d_aux = nullptr;   // TmChain / TmMultFull records kept for the backward kernel
    double *d_wt = nullptr;        // [cap][2] {T, wscale} device copies written by the setup kernel
    int32_t *d_ticket = nullptr;   // [cap] arrival counters of the in-launch finalize (kept at zero between launches)
    TmCellRec *d_cell = nullptr;   // [cap][cells] background polynomials
    TmTileHdr *d_thdr = nullptr;   // [cap][tiles_max] tile headers (per-chain boundaries)
    TmActive *d_tidx = nullptr;    // [cap][tiles_max][n_mult] active multiplet lists
    double *d_model = nullptr;
    size_t model_cap = 0;
    // host-pointer entry point: pinned, device-mapped staging the kernels read / write directly over PCIe
    // (no copy-engine round trips): h_in = [params | Tcoefs], h_out = [logL | grad], h_status
    TmPinned h_in, h_out, h_status;
    int h_cap = 0, h_nvars = -1;
    hipEvent_t ev_done = nullptr;  // completion of a host-pointer call, polled (tm_poll_event)
    bool ev_recorded = false;      // wait_data: the event of the current call has been recorded (lazily)
    int in_flight = 0;             // chains of a tamcmc_eval_batch_begin not yet collected by _end
    int armed = 0;                 // chains of a tamcmc_eval_batch_arm whose launches wait behind the gate for _fire
    TmPinned gate;                 // pinned words the gate kernel watches
    uint32_t gate_seq = 0;         // value that opens the gate of the armed batch
    int gate_patience = 1 << 21;   // polls (~2 us each) before the gate gives up; TAMCMC_GATE_PATIENCE (tests)
    // variables
    int Nvars = 0;
    int32_t *d_relax = nullptr;
    // shader-clock probe (tamcmc_ctx_clock_probe_begin / _end): one wave on its own stream beside the evaluation
    hipStream_t probe_stream = nullptr;
    TmPinned probe;                // pinned: {core cycles, 100 MHz ticks}
    // profiling
    bool profile = false;
    int profile_stride = 1;       // events around every n-th eval launch (tamcmc_ctx_profile(ctx, n))
    long long profile_count = 0;
    TmTimer timer;
    int groups = 0;               // fit groups this context is a member of (tamcmc_group_create); destroy is refused meanwhile
    int summaries = 0;            // summary objects bound to this context (tamcmc_summary_create); destroy is refused meanwhile
    int modetables = 0;           // mode tables bound to this context (tamcmc_modetable_create), counted like the groups
    // ordering against fit groups (tamcmc_group_eval_begin): enq_seq counts what this library put on the stream, so that a
    // group can tell whether anything came since it last ordered itself against it; after_ev is a group's "launches done"
    // event this stream has still to wait for -- the wait is enqueued by the next use of the stream (tm_ctx_settle), not by
    // the group call
    uint64_t enq_seq = 0;
    hipEvent_t after_ev = nullptr;
    const void *after_owner = nullptr;
};

// A group call left an event for this stream to wait for: enqueue the wait now (before anything else goes on the stream).
static inline hipError_t tm_ctx_settle(tamcmc_ctx *c)
{
    if (!c->after_ev) return hipSuccess;
    const hipEvent_t e = c->after_ev;
    c->after_ev = nullptr; c->after_owner = nullptr;
    return hipStreamWaitEvent(c->stream, e, 0);
}
static inline hipError_t tm_ctx_stream_sync(tamcmc_ctx *c)
{
    const hipError_t e = tm_ctx_settle(c);
    return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}

// Number of tiles.  It depends on the grid only, never on the batch: a chain's result must not change with the number
// of chains evaluated beside it (a sharded run and a single-process run have to produce bit-identical chains).
static inline int tm_ctx_tiles(const tamcmc_ctx *c, bool grad) { return grad ? c->tiles_g : c->tiles_l; }
// one tile per chain (short grids): prologue and evaluation share a launch (TAMCMC_TILES=1 on a 9..16-unit grid: two launches)
static inline bool tm_takes_fused(const tamcmc_ctx *c, int tiles) { return tiles == 1 && c->fuse != 0 && c->units <= TM_TILE_MAXU; }
// The largest batch of one call (tamcmc_eval_batch in tamcmc_accel.h states it): no launch of the batch may exceed 2^32 - 1
// work-items, the rule tamcmc_group_eval applies to its 1-D launches.  Per chain the launches are one workgroup of the
// setup kernel (and, with a gradient, of the backward kernel: 512 threads each, TM_SETUP_THREADS / TM_BW_THREADS) and
// `tiles` workgroups of TM_THREADS of the eval kernel; the fused launch is one workgroup of TM_THREADS per chain.
#define TM_CHAIN_WG_MAX 512
static inline bool tm_batch_fits(const tamcmc_ctx *c, int Nchains, bool grad)
{
    const long long lim = 0xFFFFFFFFLL, n = Nchains;
    const int tiles = tm_ctx_tiles(c, grad);
    if (n * tiles > lim / TM_THREADS) return false;
    return (tm_takes_fused(c, tiles) && !grad) || n <= lim / TM_CHAIN_WG_MAX;
}
// The arrival counters of the first n chains back to zero (after a launch that failed, or did not finalize them).
static inline void tm_zero_tickets(const tamcmc_ctx *c, int n, hipStream_t stream) { (void)hipMemsetAsync(c->d_ticket, 0, (size_t)n * sizeof(int32_t), stream); }

// tamcmc_api.cpp
int tm_ensure_capacity(tamcmc_ctx *c, int Nchains, bool grad);
TmEvalArgs tm_eval_args(const tamcmc_ctx *c, int tiles, bool grad, double *d_logL, int32_t *d_status, const int32_t *d_rows,
                        double *d_model);
int tm_enqueue(tamcmc_ctx *c, int Nchains, const double *d_params, const double *d_T, double *d_logL, double *d_grad,
               int32_t *d_status, const int32_t *d_rows, double *d_model);

// Host path without model rows: instead of waiting for the launch to retire, watch the results arrive.  Every logL and
// gradient entry is one aligned 8-byte store and every status one 4-byte store into coherent pinned memory, written
// exactly once per launch, so a slot that no longer holds the marker put there before the launch holds its final
// value -- no ordering between slots is assumed.  The completion event is still recorded and consulted now and then:
// a failed launch ends the wait with an error instead of a hang, and should a result ever equal the marker (a kernel
// NaN does not have this payload) the wait ends when the launch retires.
static const uint64_t TM_PENDING_BITS = 0x7FF8DEADBEEF5A5AULL;
// The marker / wait code, shared by a context's host path and a fit group's (tamcmc_group_eval_begin): out = the watched
// doubles (the first n of them are the logL slots), st = the n status slots, ev / recorded = the completion event of the
// call, recorded lazily on `stream`.
struct TmWatch {
    uint64_t *out;
    int32_t *st;
    hipEvent_t *ev;
    bool *recorded;
    hipStream_t stream;
};
// nw = doubles to watch: n (logL) or n * (1 + Nvars) (logL, then the gradient rows)
static inline void tm_mark_slots(const TmWatch &w, int n, size_t nw)
{
    for (size_t m = 0; m < nw; m++) w.out[m] = TM_PENDING_BITS;
    for (int m = 0; m < n; m++) w.st[m] = -1;
}
// rearm(): puts the arrival counters behind the watched launch back to zero (called on every error path)
template <class Rearm>
static int tm_wait_slots(const TmWatch &w, int n, size_t nw, Rearm rearm)
{
    volatile const uint64_t *o = w.out;
    volatile const int32_t *st = w.st;
    unsigned spins = 0;
    for (size_t m = 0; m < nw;) {
        if (o[m] != TM_PENDING_BITS && (m >= (size_t)n || st[m] != -1)) { m++; continue; }
        __builtin_ia32_pause();
        if ((++spins & 2047u) == 0) {
            // The completion event is recorded only now, behind the kernels already in the stream (it completes once they
            // have): a call that gets its results within the first ~2000 polls -- every healthy call -- never pays for an
            // event on the launch path (~1.5 us of host time per call in a sampler loop).
            if (!*w.recorded) {
                if (!*w.ev && hipEventCreateWithFlags(w.ev, hipEventDisableTiming) != hipSuccess) return TAMCMC_E_HIP;
                if (hipEventRecord(*w.ev, w.stream) != hipSuccess) return TAMCMC_E_HIP;
                *w.recorded = true;
            }
            const hipError_t e = hipEventQuery(*w.ev);
            if (e == hipSuccess) {
                // The launch has retired: whatever the slots hold is final.  A logL / status slot that still holds its
                // marker was never written -- a chain whose finalize did not run (e.g. an arrival counter left non-zero
                // by an earlier failed launch).  Report it instead of handing the marker out as a result, and re-arm
                // the counters so that the context is usable again.
                for (size_t k = 0; k < (size_t)n; k++)
                    if (o[k] == TM_PENDING_BITS || st[k] == -1) {
                        snprintf(tm_hip_err, sizeof(tm_hip_err), "chain %zu was not finalized by a retired launch", k);
                        rearm();
                        return TAMCMC_E_HIP;
                    }
                return TAMCMC_OK;
            }
            if (e != hipErrorNotReady) {
                snprintf(tm_hip_err, sizeof(tm_hip_err), "hipEventQuery -> %s", hipGetErrorString(e));
                rearm();
                return TAMCMC_E_HIP;
            }
        }
    }
    return TAMCMC_OK;
}
// one slot: TAMCMC_PENDING, or its final value
static inline int tm_poll_slot(const uint64_t *out, const int32_t *status, size_t slot, double *logL, int32_t *st_out)
{
    const uint64_t v = reinterpret_cast<volatile const uint64_t *>(out)[slot];
    const int32_t st = reinterpret_cast<volatile const int32_t *>(status)[slot];
    if (v == TM_PENDING_BITS || st == -1) return TAMCMC_PENDING;
    std::memcpy(logL, &v, sizeof(double));
    *st_out = st;
    return TAMCMC_OK;
}
