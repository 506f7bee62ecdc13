// tamcmc_modetable_api.cpp -- host side of the posterior mode table (tamcmc_modetable_* in include/tamcmc_accel.h): the
// object, its blocks and the results.  The kernels are in tamcmc_modetable.hip, the column layout and the shared
// arithmetic in tamcmc_modetable.h, the object's struct in tamcmc_modetable_obj.h (tamcmc_modediag_api.cpp,
// tamcmc_moderank_api.cpp, tamcmc_modepdf_api.cpp and tamcmc_seismic_api.cpp work on it too; the last one appends the seismic
// indices as further columns, and a block then runs its indices kernel between the derive and the fold kernel).
//
// A push takes its samples in blocks of B on the context's stream: the params rows go to the device, the derive kernel
// writes B x n_cols rows and B status codes, the status codes come back, the host decides which samples are accepted
// (status OK and not skipped) and hands that to the fold kernel with the number of samples accepted so far.  The counts
// live on the host; the statistics and the table on the device.  A push that would overfill the table is undone from a
// copy of the statistics taken when it began: the rows it appended lie past the count and are never read.
#include <cmath>
#include <new>

#include "tamcmc_modetable_obj.h"          // struct tamcmc_modetable

static int mt_check(const tamcmc_modetable *mt, int32_t Nsamples, int32_t Nparams, const double *params)
{
    if (!mt || !params || Nsamples < 1) return TAMCMC_E_INVALID;
    const tamcmc_ctx *c = mt->c;
    if (Nparams != c->L.Nparams || c->in_flight || c->armed) return TAMCMC_E_INVALID;
    return TAMCMC_OK;
}

// params rows of a block to the device, the derive kernel behind them (timed when `timed`), and behind that the indices
// kernel of a table whose seismic indices are enabled
static int mt_derive_block(tamcmc_modetable *mt, int n, const double *params, bool timed)
{
    tamcmc_ctx *c = mt->c;
    const size_t np = (size_t)c->L.Nparams;
    TM_HIP(tm_ctx_settle(c));
    c->enq_seq++;
    TM_HIP(hipMemcpyAsync(mt->d_params, params, (size_t)n * np * sizeof(double), hipMemcpyHostToDevice, c->stream));
    TmMtDeriveArgs a{};
    a.L = c->L; a.params = mt->d_params; a.rows = mt->d_rows; a.status = mt->d_status; a.B = n; a.n_cols = mt->n_cols;
    const size_t lds = ((np + 1) & ~(size_t)1) * sizeof(double);
    int rc;
    if (timed) rc = tm_mt_timed_record(mt, mt->ev, "modetable derive", [&] { return tm_launch_modetable_derive(a, lds, c->stream); });
    else {
        const int hr = tm_launch_modetable_derive(a, lds, c->stream);
        rc = hr != 0 ? tm_launch_failed("modetable derive", hr) : TAMCMC_OK;
    }
    if (rc != TAMCMC_OK || mt->n_index_cols == 0) return rc;
    return tm_seis_block(mt, n, timed);             // the seismic indices behind the derive kernel (tamcmc_seismic_api.cpp)
}

static int mt_clear(tamcmc_modetable *mt)
{
    mt->n_used = 0; mt->n_rejected = 0; mt->clock.clear();
    mt->diag.clear(); mt->rank.clear(); mt->seis.clear(); mt->pdf.clear();
    TM_HIP(hipMemsetAsync(mt->d_state, 0, mt->state_doubles() * sizeof(double), mt->c->stream));
    return TAMCMC_OK;
}

extern "C" int tamcmc_modetable_create(tamcmc_modetable **out, tamcmc_ctx *c, int64_t max_samples)
{
    if (!out) return TAMCMC_E_INVALID;
    *out = nullptr;
    if (!c || max_samples < 0 || max_samples >= ((int64_t)1 << 31) || c->in_flight || c->armed) return TAMCMC_E_INVALID;
    if (c->L.family == TM_FAM_GAUSS || c->L.n_mult < 1 || c->L.n_mult > TM_MAXMULT) return TAMCMC_E_INVALID;   // ids 0 and 1: no multiplets
    tamcmc_modetable *mt = new (std::nothrow) tamcmc_modetable();
    if (!mt) return TAMCMC_E_NOMEM;
    mt->c = c;
    mt->max_samples = (long long)max_samples;
    auto fail = [&](int code) { (void)hipGetLastError(); tamcmc_modetable_destroy(mt); return code; };
    try {
        mt->n_cols = tm_mt_layout(c->L, nullptr);
        mt->cols.resize((size_t)mt->n_cols);
    } catch (const std::bad_alloc &) { return fail(TAMCMC_E_NOMEM); }
    tm_mt_layout(c->L, mt->cols.data());
    mt->n_base_cols = mt->n_cols;
    mt->B = tm_mt_block(mt->n_cols);
    const size_t nc = (size_t)mt->n_cols, b = (size_t)mt->B, np = (size_t)c->L.Nparams;
    if (((np + 1) & ~(size_t)1) * sizeof(double) > 60 * 1024) return fail(TAMCMC_E_INVALID);       // the row does not fit the derive kernel's LDS
    if (max_samples > 0 && (size_t)max_samples > (SIZE_MAX / sizeof(double)) / nc) return fail(TAMCMC_E_NOMEM);
    if (hipSetDevice(c->device) != hipSuccess) return fail(TAMCMC_E_NODEVICE);
    if (hipMalloc(&mt->d_params, b * np * sizeof(double)) != hipSuccess || hipMalloc(&mt->d_rows, b * nc * sizeof(double)) != hipSuccess ||
        hipMalloc(&mt->d_status, b * sizeof(int32_t)) != hipSuccess || hipMalloc(&mt->d_accept, b * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&mt->d_state, (2 * TM_MT_NSTATE + TM_Q_MAXQ) * nc * sizeof(double)) != hipSuccess ||
        hipMalloc(&mt->d_ranks, TM_Q_MAXQ * sizeof(uint64_t)) != hipSuccess ||
        (max_samples > 0 && hipMalloc(&mt->d_table, tm_mt_table_bytes(mt->max_samples, mt->n_cols)) != hipSuccess))
        return fail(TAMCMC_E_NOMEM);
    if (hipEventCreate(&mt->ev[0]) != hipSuccess || hipEventCreate(&mt->ev[1]) != hipSuccess) return fail(TAMCMC_E_HIP);
    if (tm_ctx_settle(c) != hipSuccess || mt_clear(mt) != TAMCMC_OK) return fail(TAMCMC_E_HIP);
    c->enq_seq++;
    c->modetables++;
    mt->counted = true;
    *out = mt;
    return TAMCMC_OK;
}

extern "C" int tamcmc_modetable_destroy(tamcmc_modetable *mt)
{
    if (!mt) return TAMCMC_OK;
    tamcmc_ctx *c = mt->c;
    if (c->armed) return TAMCMC_E_INVALID;          // the stream cannot be waited for behind a closed gate
    (void)hipSetDevice(c->device);
    if (c->stream) (void)tm_ctx_stream_sync(c);
    if (mt->counted) c->modetables--;
    (void)hipFree(mt->d_params); (void)hipFree(mt->d_rows); (void)hipFree(mt->d_status); (void)hipFree(mt->d_accept);
    (void)hipFree(mt->d_state); (void)hipFree(mt->d_ranks); (void)hipFree(mt->d_table);
    mt->diag.release(); mt->rank.release(); mt->seis.release(); mt->pdf.release();
    for (hipEvent_t e : mt->ev) if (e) (void)hipEventDestroy(e);
    delete mt;
    return TAMCMC_OK;
}

extern "C" int tamcmc_modetable_columns(tamcmc_modetable *mt, int32_t *n_cols, int32_t *n_mult)
{
    if (!tm_mt_idle(mt) || !n_cols || !n_mult) return TAMCMC_E_INVALID;
    *n_cols = mt->n_cols;
    *n_mult = mt->c->L.n_mult;
    return TAMCMC_OK;
}

extern "C" int tamcmc_modetable_column(tamcmc_modetable *mt, int32_t col, tamcmc_modetable_col *out)
{
    if (!tm_mt_idle(mt) || !out || col < 0 || col >= mt->n_cols) return TAMCMC_E_INVALID;
    const TmMtCol &k = mt->cols[(size_t)col];
    out->kind = k.kind; out->mult = k.mult; out->order = k.order; out->l = k.l; out->m = k.m; out->param_index = k.param_index;
    return TAMCMC_OK;
}

extern "C" int tamcmc_modetable_derive(tamcmc_modetable *mt, int32_t Nsamples, int32_t Nparams, const double *params, double *rows,
                                       int32_t *status)
{
    int rc = mt_check(mt, Nsamples, Nparams, params);
    if (rc != TAMCMC_OK) return rc;
    if (!rows) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = mt->c;
    TM_HIP(hipSetDevice(c->device));
    const size_t nc = (size_t)mt->n_cols, np = (size_t)Nparams;
    auto fail = [&](int code) { (void)hipStreamSynchronize(c->stream); return code; };
    for (int32_t k = 0; k < Nsamples; k += mt->B) {
        const int n = Nsamples - k < mt->B ? Nsamples - k : mt->B;
        rc = mt_derive_block(mt, n, params + (size_t)k * np, false);
        if (rc != TAMCMC_OK) return fail(rc);
        if (hipMemcpyAsync(rows + (size_t)k * nc, mt->d_rows, (size_t)n * nc * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            (status && hipMemcpyAsync(status + k, mt->d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            return fail(TAMCMC_E_HIP);
    }
    TM_HIP(hipGetLastError());
    return TAMCMC_OK;
}

extern "C" int tamcmc_modetable_push(tamcmc_modetable *mt, int32_t Nsamples, int32_t Nparams, const double *params, const int32_t *skip,
                                     int32_t *status)
{
    int rc = mt_check(mt, Nsamples, Nparams, params);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = mt->c;
    TM_HIP(hipSetDevice(c->device));
    mt->diag.invalidate(); mt->rank.invalidate(); mt->seis.invalidate(); mt->pdf.invalidate();      // what they keep is that of the table before this push
    const size_t np = (size_t)Nparams, ns = mt->state_doubles();
    std::vector<int32_t> st, acc;
    try { st.resize((size_t)Nsamples); acc.resize((size_t)mt->B); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    const long long used0 = mt->n_used, rej0 = mt->n_rejected;
    auto fail = [&](int code) { (void)hipStreamSynchronize(c->stream); return code; };
    // undo: the statistics as they were, the counts as they were (rows appended since lie past the count)
    auto undo = [&](int code) {
        (void)hipMemcpyAsync(mt->d_state, mt->d_state + ns, ns * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
        mt->n_used = used0; mt->n_rejected = rej0;
        return fail(code);
    };
    TM_HIP(tm_ctx_settle(c));
    TM_HIP(hipMemcpyAsync(mt->d_state + ns, mt->d_state, ns * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    for (int32_t k = 0; k < Nsamples; k += mt->B) {
        const int n = Nsamples - k < mt->B ? Nsamples - k : mt->B;
        rc = mt_derive_block(mt, n, params + (size_t)k * np, true);
        if (rc != TAMCMC_OK) return undo(rc);
        if (hipMemcpyAsync(st.data() + k, mt->d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess || tm_mt_timed_add(mt->ev, mt->clock) != TAMCMC_OK ||
            (mt->n_index_cols > 0 && tm_seis_timed_done(mt) != TAMCMC_OK))
            return undo(TAMCMC_E_HIP);
        long long take = 0;
        for (int i = 0; i < n; i++) {
            acc[(size_t)i] = (st[(size_t)(k + i)] == TAMCMC_CHAIN_OK && !(skip && skip[k + i] != 0)) ? 1 : 0;
            take += acc[(size_t)i];
        }
        if (mt->max_samples > 0 && mt->n_used + take > mt->max_samples) return undo(TAMCMC_E_INVALID);
        if (take > 0) {
            if (hipMemcpyAsync(mt->d_accept, acc.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream) != hipSuccess)
                return undo(TAMCMC_E_HIP);
            TmMtFoldArgs a{};
            a.rows = mt->d_rows; a.accept = mt->d_accept; a.state = mt->d_state; a.table = mt->d_table;
            a.n_before = mt->n_used; a.max_samples = mt->max_samples; a.B = n; a.n_cols = mt->n_cols;
            rc = tm_mt_timed_record(mt, mt->ev, "modetable fold", [&] { return tm_launch_modetable_fold(a, c->stream); });
            if (rc != TAMCMC_OK) return undo(rc);
            if (hipStreamSynchronize(c->stream) != hipSuccess || tm_mt_timed_add(mt->ev, mt->clock) != TAMCMC_OK) return undo(TAMCMC_E_HIP);
        }
        mt->n_used += take;
        mt->n_rejected += n - take;
    }
    TM_HIP(hipGetLastError());
    if (status) std::memcpy(status, st.data(), (size_t)Nsamples * sizeof(int32_t));
    return TAMCMC_OK;
}

extern "C" int tamcmc_modetable_result(tamcmc_modetable *mt, tamcmc_modetable_totals *t, double *mean, double *sd, double *mn, double *mx)
{
    if (!tm_mt_idle(mt)) return TAMCMC_E_INVALID;
    const int rc = tm_mt_enter(mt);                 // (it enqueues nothing; the count it adds to only makes a fit group order itself once more)
    if (rc != TAMCMC_OK) return rc;
    const size_t nc = (size_t)mt->n_cols;
    std::vector<double> st;
    try { st.resize(mt->state_doubles()); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    TM_HIP(hipMemcpy(st.data(), mt->d_state, st.size() * sizeof(double), hipMemcpyDeviceToHost));
    const long long n = mt->n_used;
    const double nan = std::nan(""), dn = (double)n;
    for (size_t i = 0; i < nc; i++) {
        if (mean) mean[i] = n >= 1 ? st[TM_MT_MEAN * nc + i] : nan;
        if (sd) sd[i] = n >= 2 ? std::sqrt(st[TM_MT_M2 * nc + i] / (dn - 1.0)) : nan;
        if (mn) mn[i] = n >= 1 ? st[TM_MT_MIN * nc + i] : nan;
        if (mx) mx[i] = n >= 1 ? st[TM_MT_MAX * nc + i] : nan;
    }
    if (t) { t->n_used = n; t->n_rejected = mt->n_rejected; t->n_cols = mt->n_cols; t->n_mult = mt->c->L.n_mult; }
    return TAMCMC_OK;
}

extern "C" int tamcmc_modetable_quantiles(tamcmc_modetable *mt, int32_t Nq, const double *q, int64_t *ranks, double *out)
{
    if (!tm_mt_idle(mt) || !q || !out || Nq < 1 || Nq > TAMCMC_SUMMARY_MAX_QUANTILES) return TAMCMC_E_INVALID;
    for (int j = 0; j < Nq; j++)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return TAMCMC_E_INVALID;        // (a NaN fails both comparisons)
    if (mt->max_samples < 1 || mt->n_used < 1) return TAMCMC_E_INVALID;
    const int rc = tm_mt_enter(mt);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = mt->c;
    uint64_t rk[TM_Q_MAXQ] = {};
    for (int j = 0; j < Nq; j++) rk[j] = (uint64_t)tmq_rank(q[j], (int64_t)mt->n_used);
    const size_t nc = (size_t)mt->n_cols;
    auto fail = [&](int code) { (void)hipStreamSynchronize(c->stream); return code; };
    if (hipMemcpyAsync(mt->d_ranks, rk, sizeof(rk), hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(TAMCMC_E_HIP);
    TmMtQuantArgs a{};
    a.table = mt->d_table; a.state = mt->d_state; a.ranks = mt->d_ranks; a.out = mt->d_state + 2 * mt->state_doubles();
    a.n = mt->n_used; a.max_samples = mt->max_samples; a.n_cols = mt->n_cols; a.Nq = Nq;
    const int hr = tm_launch_modetable_quantiles(a, c->stream);
    if (hr != 0) { (void)tm_launch_failed("modetable quantiles", hr); return fail(TAMCMC_E_HIP); }
    if (hipMemcpyAsync(out, a.out, (size_t)Nq * nc * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(TAMCMC_E_HIP);
    if (ranks) for (int j = 0; j < Nq; j++) ranks[j] = (int64_t)rk[j];
    return TAMCMC_OK;
}

extern "C" int tamcmc_modetable_reset(tamcmc_modetable *mt)
{
    if (!tm_mt_idle(mt)) return TAMCMC_E_INVALID;
    const int rc = tm_mt_enter(mt);
    return rc != TAMCMC_OK ? rc : mt_clear(mt);
}

extern "C" int tamcmc_modetable_kernel_time(tamcmc_modetable *mt, double *total_ms, int64_t *launches)
{
    return tm_mt_idle(mt) ? mt->clock.read(total_ms, launches) : TAMCMC_E_INVALID;
}
