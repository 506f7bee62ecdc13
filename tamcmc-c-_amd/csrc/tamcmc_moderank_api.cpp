// tamcmc_moderank_api.cpp -- host side of the mode table's rank-normalised diagnostics (tamcmc_moderank_* in
// include/tamcmc_accel.h): bulk and tail ESS, rank-normalised and folded split R-hat of the table's columns.  The sort,
// transform and mean kernels are in tamcmc_moderank.hip, the shared arithmetic in tamcmc_moderank.h; the lag products and the
// finish of the four series are tamcmc_modediag.hip's kernels, launched on the series table.
//
// A call writes nothing of the table's state and nothing of tamcmc_modediag_*'s buffers.  The selected columns are taken in
// chunks of w columns, w sized so that a chunk (tmr_col_bytes per column) fits the scratch; columns are independent, so no
// result bit depends on w.  The scratch hangs off the object, grown only when a call needs more, the new one allocated
// before the old one is freed; the lag products of the last call are kept on the host.
#include <cmath>
#include <new>

#include "tamcmc_modetable_obj.h"
#include "tamcmc_moderank.h"

// a chunk's buffers inside one allocation of w * tmr_col_bytes(n, L) bytes: the 8-byte arrays first
struct MrChunk {
    TmMrArgs r{};
    TmMdArgs d{};
};
static MrChunk mr_carve(const tamcmc_modetable *mt, void *base, const int w, const long long n, const int L, long long *rank2)
{
    MrChunk k;
    const size_t P = (size_t)tmr_padded(n), ns = (size_t)TM_MR_NSERIES * (size_t)w;
    uint64_t *keys = (uint64_t *)base;
    double *series = (double *)(keys + 2 * (size_t)w * P);
    double *mean = series + ns * (size_t)n;
    double *acc = mean + ns;
    double *fin = acc + (size_t)(L + 1) * ns;
    double *medq = fin + (size_t)TM_MD_NFIN * ns;
    int32_t *cut = (int32_t *)(medq + 3 * (size_t)w);
    int32_t *sel = cut + ns;
    k.r = tmr_sort_args(mt->d_table, sel, keys, n, mt->max_samples, (long long)P, w);
    k.r.series = series; k.r.mean = mean; k.r.medq = medq; k.r.rank2 = rank2;
    k.d.table = series; k.d.mean = mean; k.d.acc = acc; k.d.fin = fin; k.d.cut = cut;
    k.d.n = n; k.d.max_samples = n; k.d.n_cols = (int32_t)ns; k.d.L = L;
    k.d.tau_floor = 1.0 / std::log10((double)n);
    return k;
}

// the chunk's columns to the device, then the kernels that form its series and, with `lags`, those of their lag products
static int mr_run(tamcmc_modetable *mt, const MrChunk &k, const int32_t *sel, const bool lags)
{
    tamcmc_ctx *c = mt->c;
    TmMtClock &clock = mt->rank.clock;
    TM_HIP(hipMemcpy((void *)k.r.sel, sel, (size_t)k.r.w * sizeof(int32_t), hipMemcpyHostToDevice));
    int rc = tm_mt_timed(mt, clock, "moderank sort", [&] { return tm_launch_moderank_sort(k.r, 0, c->stream); });
    if (rc == TAMCMC_OK) rc = tm_mt_timed(mt, clock, "moderank sort (folded)", [&] { return tm_launch_moderank_sort(k.r, 1, c->stream); });
    if (rc == TAMCMC_OK) rc = tm_mt_timed(mt, clock, "moderank transform", [&] { return tm_launch_moderank_transform(k.r, c->stream); });
    if (rc == TAMCMC_OK) rc = tm_mt_timed(mt, clock, "moderank mean", [&] { return tm_launch_moderank_mean(k.r, c->stream); });
    if (rc == TAMCMC_OK && lags) rc = tm_mt_timed(mt, clock, "moderank lag", [&] { return tm_launch_modediag_lag(k.d, c->stream); });
    if (rc == TAMCMC_OK && lags) rc = tm_mt_timed(mt, clock, "moderank finish", [&] { return tm_launch_modediag_finish(k.d, c->stream); });
    return rc;
}

extern "C" int tamcmc_moderank_diag(tamcmc_modetable *mt, int32_t max_lag, int32_t n_sel, const int32_t *cols, int64_t scratch_bytes,
                                    tamcmc_moderank_totals *totals, double *out, int32_t *cut)
{
    if (!tm_mt_ready(mt, 4)) return TAMCMC_E_INVALID;
    if (max_lag < 0 || max_lag > TAMCMC_MODEDIAG_MAX_LAG || scratch_bytes < 0) return TAMCMC_E_INVALID;
    const long long n = mt->n_used;
    const int L = tme_lag_limit(max_lag, n);
    const size_t ns = (size_t)n_sel, S = TM_MR_NSERIES, nl = (size_t)(L + 1);
    std::vector<int32_t> sel, cutv, cc;
    std::vector<double> fin, acov, chunk_acc;
    int rc = tm_mt_select(mt, n_sel, cols, sel);
    if (rc != TAMCMC_OK) return rc;
    const size_t per = tmr_col_bytes(n, L);
    const size_t budget = scratch_bytes ? (size_t)scratch_bytes : (size_t)TM_MR_DEFAULT_SCRATCH;
    int w = tm_mt_chunk_width(budget, 0, per, ns, 16383);   // (4 w series are the lag kernel's grid.x, w the transform kernel's grid.y)
    try {
        cutv.resize(S * ns); fin.resize((size_t)TM_MD_NFIN * S * ns); acov.resize(S * nl * ns);
        chunk_acc.resize(S * (size_t)w * (nl + TM_MD_NFIN)); cc.resize(S * (size_t)w);
    } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    // the scratch first: a call that cannot have it returns with the object, its context's counters included, as it was
    TM_HIP(hipSetDevice(mt->c->device));
    TmMtRank &R = mt->rank;
    void *grown = nullptr;
    if (R.scratch.reserve((size_t)w * per, &grown) != TAMCMC_OK) {
        if (R.scratch.reserve(per, &grown) != TAMCMC_OK) return TAMCMC_E_NOMEM;
        w = grown ? 1 : (int)(R.scratch.bytes / per);   // one column at a time, or what the scratch at hand holds
    }
    rc = tm_mt_enter(mt);
    if (rc != TAMCMC_OK) { (void)hipFree(grown); return rc; }
    R.scratch.install(grown, (size_t)w * per);
    R.valid = false;
    for (size_t k0 = 0; k0 < ns; k0 += (size_t)w) {
        const int wc = ns - k0 < (size_t)w ? (int)(ns - k0) : w;
        const MrChunk k = mr_carve(mt, R.scratch.d, wc, n, L, nullptr);
        rc = mr_run(mt, k, sel.data() + k0, true);
        if (rc != TAMCMC_OK) return rc;
        const size_t cs = S * (size_t)wc;                                   // the chunk's series: TM_MR_NSERIES c + s
        TM_HIP(hipMemcpy(chunk_acc.data(), k.d.acc, (nl + TM_MD_NFIN) * cs * sizeof(double), hipMemcpyDeviceToHost));   // acc, then fin behind it
        for (size_t c = 0; c < (size_t)wc; c++)
            for (size_t s = 0; s < S; s++) {
                for (size_t l = 0; l < nl; l++) acov[(s * nl + l) * ns + k0 + c] = chunk_acc[l * cs + S * c + s];
                for (size_t f = 0; f < TM_MD_NFIN; f++) fin[(f * S + s) * ns + k0 + c] = chunk_acc[(nl + f) * cs + S * c + s];
            }
        TM_HIP(hipMemcpy(cc.data(), k.d.cut, cs * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t c = 0; c < (size_t)wc; c++)
            for (size_t s = 0; s < S; s++) cutv[s * ns + k0 + c] = cc[S * c + s];
    }
    R.acov.swap(acov);
    R.L = L; R.nsel = n_sel; R.valid = true;
    auto F = [&](int f, int s, size_t k) { return fin[((size_t)f * S + (size_t)s) * ns + k]; };
    std::vector<double> eb, et, rh, a0;
    try { eb.resize(ns); et.resize(ns); rh.resize(ns); a0.resize(ns); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    for (size_t k = 0; k < ns; k++) {
        eb[k] = F(TM_MD_ESS, TM_MR_Z, k);
        et[k] = tmr_min_skip(F(TM_MD_ESS, TM_MR_I05, k), F(TM_MD_ESS, TM_MR_I95, k));
        rh[k] = tmr_max_skip(F(TM_MD_RHAT, TM_MR_Z, k), F(TM_MD_RHAT, TM_MR_ZFOLD, k));
        a0[k] = R.acov[((size_t)TM_MR_Z * nl) * ns + k];
        if (out) {
            out[TM_MR_ESS_BULK * ns + k] = eb[k];
            out[TM_MR_ESS_TAIL * ns + k] = et[k];
            out[TM_MR_RHAT * ns + k] = rh[k];
            out[TM_MR_TAU_BULK * ns + k] = F(TM_MD_TAU, TM_MR_Z, k);
            out[TM_MR_RHAT_BULK * ns + k] = F(TM_MD_RHAT, TM_MR_Z, k);
            out[TM_MR_RHAT_FOLD * ns + k] = F(TM_MD_RHAT, TM_MR_ZFOLD, k);
            out[TM_MR_ESS_Q05 * ns + k] = F(TM_MD_ESS, TM_MR_I05, k);
            out[TM_MR_ESS_Q95 * ns + k] = F(TM_MD_ESS, TM_MR_I95, k);
        }
    }
    if (cut) std::memcpy(cut, cutv.data(), cutv.size() * sizeof(int32_t));
    if (totals) {
        const TmrTotals t = tmr_totals(n_sel, sel.data(), n, L, eb.data(), et.data(), rh.data(), cutv.data() + (size_t)TM_MR_Z * ns, a0.data());
        totals->n_used = t.n_used; totals->lag = t.lag;
        totals->min_ess_bulk = t.min_ess_bulk; totals->min_ess_tail = t.min_ess_tail; totals->max_rhat = t.max_rhat;
        totals->col_min_ess_bulk = t.col_min_ess_bulk; totals->col_min_ess_tail = t.col_min_ess_tail; totals->col_max_rhat = t.col_max_rhat;
        totals->n_truncated = t.n_truncated; totals->n_constant = t.n_constant; totals->n_rhat_high = t.n_rhat_high;
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_moderank_acov(tamcmc_modetable *mt, int32_t series, double *acov)
{
    if (!tm_mt_ready(mt, 4) || !acov || series < 0 || series >= TM_MR_NSERIES || !mt->rank.valid) return TAMCMC_E_INVALID;
    const size_t m = (size_t)(mt->rank.L + 1) * (size_t)mt->rank.nsel;
    std::memcpy(acov, mt->rank.acov.data() + (size_t)series * m, m * sizeof(double));
    return TAMCMC_OK;
}

extern "C" int tamcmc_moderank_series(tamcmc_modetable *mt, int32_t col, int64_t *rank2, int64_t *rank2_fold, double *series, double *mean,
                                      double *med_q)
{
    if (!tm_mt_ready(mt, 4) || col < 0 || col >= mt->n_cols) return TAMCMC_E_INVALID;
    const long long n = mt->n_used;
    const int L = 1;                                                        // (the lag kernels are not run)
    int rc = tm_mt_enter(mt);
    if (rc != TAMCMC_OK) return rc;
    void *base = nullptr;
    long long *d_rank2 = nullptr;
    if (hipMalloc(&base, tmr_col_bytes(n, L)) != hipSuccess || hipMalloc(&d_rank2, 2 * (size_t)n * sizeof(long long)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(base);
        return TAMCMC_E_NOMEM;
    }
    const MrChunk k = mr_carve(mt, base, 1, n, L, d_rank2);
    tamcmc_ctx *c = mt->c;
    auto done = [&](int code) { (void)hipStreamSynchronize(c->stream); (void)hipFree(base); (void)hipFree(d_rank2); return code; };
    rc = mr_run(mt, k, &col, false);
    if (rc != TAMCMC_OK) return done(rc);
    const size_t sn = (size_t)n;
    if ((rank2 && hipMemcpy(rank2, d_rank2, sn * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) ||
        (rank2_fold && hipMemcpy(rank2_fold, d_rank2 + sn, sn * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) ||
        (series && hipMemcpy(series, k.r.series, TM_MR_NSERIES * sn * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
        (mean && hipMemcpy(mean, k.r.mean, TM_MR_NSERIES * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
        (med_q && hipMemcpy(med_q, k.r.medq, 3 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
        return done(TAMCMC_E_HIP);
    return done(TAMCMC_OK);
}

extern "C" int tamcmc_moderank_kernel_time(tamcmc_modetable *mt, double *total_ms, int64_t *launches)
{
    return tm_mt_idle(mt) ? mt->rank.clock.read(total_ms, launches) : TAMCMC_E_INVALID;
}
