// tamcmc_modetable_obj.h -- internal to csrc/: the posterior mode table's object, shared by the source files that work on
// it: tamcmc_modetable_api.cpp (the table, its statistics and quantiles), tamcmc_modediag_api.cpp (ESS, MCSE, split
// R-hat, covariances and correlations of its columns), tamcmc_moderank_api.cpp (their rank-normalised counterparts),
// tamcmc_seismic_api.cpp (the seismic indices appended to its columns) and tamcmc_modepdf_api.cpp (histograms, shortest
// intervals and pair densities of its columns).
//
// Each of the four features beside the table owns one member struct of the object (diag, rank, seis, pdf) and reaches no
// other's; the table's own file reaches them through their hooks alone:
//   invalidate()  the table's rows changed (push)
//   clear()       reset: the clock to zero and invalidate(); buffers and the seismic plan stay
//   release()     destroy: device memory and events
//   sized_by_columns()  (diag, rank) a device buffer exists that was sized while n_cols was what it is: indices_enable refuses
// Behind the object stand the helpers every call of the five files goes through: the handle checks, the entry, the timed
// launch, the column selection, the grow-only device buffer and the chunk width.
#pragma once
#include <new>

#include "tamcmc_host.h"
#include "tamcmc_modetable.h"
#include "tamcmc_seismic.h"

// kernel time and launches since create / reset
struct TmMtClock {
    double ms = 0.0;
    int64_t launches = 0;
    void clear() { ms = 0.0; launches = 0; }
    int read(double *total_ms, int64_t *n) const            // what a *_kernel_time call returns, once tm_mt_idle has passed the handle
    {
        if (!total_ms || !n) return TAMCMC_E_INVALID;
        *total_ms = ms; *n = launches;
        return TAMCMC_OK;
    }
};

// A device buffer that only grows.  reserve allocates nothing while the buffer fits and otherwise hands the new allocation
// back in *grown, the old one untouched: the caller installs it once nothing can fail before a launch, or frees it.  So a
// call that runs out of memory leaves the object as it was.
struct TmMtBuf {
    void *d = nullptr;
    size_t bytes = 0;
    int reserve(const size_t want, void **grown) const
    {
        *grown = nullptr;
        if (want <= bytes) return TAMCMC_OK;
        if (hipMalloc(grown, want) != hipSuccess) { (void)hipGetLastError(); *grown = nullptr; return TAMCMC_E_NOMEM; }
        return TAMCMC_OK;
    }
    void install(void *grown, const size_t want)
    {
        if (!grown) return;
        (void)hipFree(d);
        d = grown; bytes = want;
    }
    void release() { (void)hipFree(d); d = nullptr; bytes = 0; }
};

// tamcmc_modediag_* (tamcmc_modediag_api.cpp); nothing is allocated before the first call that needs it
struct TmMtDiag {
    TmMtBuf acc;                         // double [L + 1][n_cols] lag products, then [TM_MD_NFIN][n_cols] tau, ess, rhat; grown when L grows
    TmMtBuf cut;                         // int32 [n_cols]
    int L = 0;                           // L of the last _ess call, while acov_valid
    bool acov_valid = false;             // acc holds the lag products of the table as it is: no push or reset since
    TmMtBuf S;                           // double [n_sel][n_sel] sums of products of the last _cov / _corr call; grown when n_sel grows
    TmMtBuf sel;                         // int32 [n_sel] its columns
    TmMtClock clock;                     // lag, finish and covariance kernels
    void invalidate() { acov_valid = false; }
    void clear() { clock.clear(); invalidate(); }
    void release() { acc.release(); cut.release(); S.release(); sel.release(); }
    bool sized_by_columns() const { return acc.d || cut.d || S.d || sel.d; }
};

// tamcmc_moderank_* (tamcmc_moderank_api.cpp); nothing is allocated before the first call that needs it
struct TmMtRank {
    TmMtBuf scratch;                     // a chunk's key buffers, series, means, lag products, finish arrays (tmr_col_bytes each column)
    std::vector<double> acov;            // [TM_MR_NSERIES][L + 1][nsel] lag products of the last _diag call, on the host
    int L = 0, nsel = 0;
    bool valid = false;                  // acov is that of the table as it is: no push or reset since
    TmMtClock clock;                     // sort, transform, mean, lag and finish kernels of _diag / _series
    void invalidate() { valid = false; }
    void clear() { clock.clear(); invalidate(); }
    void release() { scratch.release(); }
    bool sized_by_columns() const { return scratch.d != nullptr; }
};

// tamcmc_modetable_indices_* (tamcmc_seismic_api.cpp); nothing is allocated until _indices_enable.  (How many columns the
// indices add is the table's own n_index_cols.)
struct TmMtSeis {
    TmSeisPlan plan;
    int32_t *d_i = nullptr;              // first [n_index + 1], n_num [n_index], src [n_terms], wsrc [n_terms]
    double *d_d = nullptr;               // coef [n_terms], offset [n_index]
    hipEvent_t ev[2] = {nullptr, nullptr};   // its own pair: the indices kernel is timed while the derive kernel's pair is in use
    TmMtClock clock;                     // indices kernel
    void invalidate() {}                 // nothing here is computed from the rows
    void clear() { clock.clear(); invalidate(); }
    void release()
    {
        (void)hipFree(d_i); (void)hipFree(d_d);
        for (hipEvent_t &e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        d_i = nullptr; d_d = nullptr;
    }
};

// tamcmc_modepdf_* (tamcmc_modepdf_api.cpp); nothing is allocated before the first call that needs it.  No
// sized_by_columns(): the scratch's size comes from the call's selection, bins and n, never from n_cols, so a table that was
// filled, histogrammed and reset may still enable its indices.
struct TmMtPdf {
    TmMtBuf scratch;                     // a call's arguments and counters, or an HPD chunk's keys and results
    TmMtClock clock;                     // histogram, pair and HPD kernels and the sort launches of _hpd
    void invalidate() {}                 // a call keeps no result
    void clear() { clock.clear(); invalidate(); }
    void release() { scratch.release(); }
};

struct tamcmc_modetable {
    tamcmc_ctx *c = nullptr;
    bool counted = false;                // the context's count includes this object
    int n_cols = 0, B = 0;
    int n_base_cols = 0, n_index_cols = 0;   // n_cols = n_base_cols + n_index_cols; n_index_cols = 0 until _indices_enable
    long long max_samples = 0;
    std::vector<TmMtCol> cols;
    double *d_params = nullptr;          // [B][Nparams]
    double *d_rows = nullptr;            // [B][n_cols]
    int32_t *d_status = nullptr, *d_accept = nullptr;   // [B]
    double *d_state = nullptr;           // [TM_MT_NSTATE][n_cols], then the copy a push can be undone from, then [TM_Q_MAXQ][n_cols] quantiles
    uint64_t *d_ranks = nullptr;         // [TM_Q_MAXQ]
    double *d_table = nullptr;           // [n_cols][max_samples]
    long long n_used = 0, n_rejected = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};   // the pair of every timed launch but the indices kernel's
    TmMtClock clock;                     // derive and fold kernels
    size_t state_doubles() const { return (size_t)TM_MT_NSTATE * (size_t)n_cols; }
    TmMtDiag diag;
    TmMtRank rank;
    TmMtSeis seis;
    TmMtPdf pdf;
};

// ---- the helpers of every call ----
// The handle is there and nothing of its context is in flight or armed.  (Like tm_mt_ready it touches no device: a NULL
// handle is refused on a machine without one.)
inline bool tm_mt_idle(const tamcmc_modetable *mt) { return mt && !mt->c->in_flight && !mt->c->armed; }
// ... and the table keeps rows on the device, n_min of them or more
inline bool tm_mt_ready(const tamcmc_modetable *mt, const long long n_min) { return tm_mt_idle(mt) && mt->max_samples != 0 && mt->n_used >= n_min; }

// the context's device, its stream waited for, and the call counted as work this library put on the stream
inline int tm_mt_enter(tamcmc_modetable *mt)
{
    TM_HIP(hipSetDevice(mt->c->device));
    TM_HIP(tm_ctx_stream_sync(mt->c));
    mt->c->enq_seq++;
    return TAMCMC_OK;
}

// One launch between the events ev[0] and ev[1] on the context's stream, not waited for: the table's blocks and the indices
// kernel behind them overlap with a copy.  tm_mt_timed_add adds the time once the caller has waited for the stream.
template <class F>
inline int tm_mt_timed_record(tamcmc_modetable *mt, const hipEvent_t *ev, const char *what, F &&launch)
{
    const hipStream_t stream = mt->c->stream;
    TM_HIP(hipEventRecord(ev[0], stream));
    const int hr = launch();
    if (hr != 0) return tm_launch_failed(what, hr);
    TM_HIP(hipEventRecord(ev[1], stream));
    return TAMCMC_OK;
}
inline int tm_mt_timed_add(const hipEvent_t *ev, TmMtClock &clock)
{
    float ms = 0.f;
    TM_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    clock.ms += (double)ms;
    clock.launches++;
    return TAMCMC_OK;
}
// One launch between the object's two events, waited for, its time added to `clock`.  The stream is waited for when the
// launch fails too, so no caller has to.
template <class F>
inline int tm_mt_timed(tamcmc_modetable *mt, TmMtClock &clock, const char *what, F &&launch)
{
    const int rc = tm_mt_timed_record(mt, mt->ev, what, launch);
    if (rc != TAMCMC_OK) { (void)hipStreamSynchronize(mt->c->stream); return rc; }
    TM_HIP(hipStreamSynchronize(mt->c->stream));
    return tm_mt_timed_add(mt->ev, clock);
}

// The selection of a call: cols NULL means the first n_sel columns; more than max_sel or n_cols of them, an index out of
// range or a repeated one is refused, all of it before anything is allocated but sel itself.
inline int tm_mt_select(const tamcmc_modetable *mt, const int32_t n_sel, const int32_t *cols, std::vector<int32_t> &sel, const int32_t max_sel = INT32_MAX)
{
    if (n_sel < 1 || n_sel > mt->n_cols || n_sel > max_sel) return TAMCMC_E_INVALID;
    std::vector<char> seen;
    try { sel.resize((size_t)n_sel); seen.assign((size_t)mt->n_cols, 0); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    for (int32_t k = 0; k < n_sel; k++) {
        const int32_t col = cols ? cols[k] : k;
        if (col < 0 || col >= mt->n_cols || seen[(size_t)col]) return TAMCMC_E_INVALID;
        seen[(size_t)col] = 1;
        sel[(size_t)k] = col;
    }
    return TAMCMC_OK;
}

// Columns of a chunk: as many as `budget` bytes hold at `per` bytes each beside `fixed` bytes, at least one, at most the
// selection and what the kernels' grids take.
inline int tm_mt_chunk_width(const size_t budget, const size_t fixed, const size_t per, const size_t n_sel, const size_t grid_limit)
{
    size_t w = budget > fixed ? (budget - fixed) / per : 0;
    if (w < 1) w = 1;
    if (w > n_sel) w = n_sel;
    if (w > grid_limit) w = grid_limit;
    return (int)w;
}

// tamcmc_seismic_api.cpp, called by a block of tamcmc_modetable_derive / _push behind the derive kernel when n_index_cols > 0:
// the indices kernel on the block's n rows (between the feature's own events when `timed`), and the addition of that time
// once the stream has been waited for.
int tm_seis_block(tamcmc_modetable *mt, int n, bool timed);
int tm_seis_timed_done(tamcmc_modetable *mt);
