// tamcmc_modediag_api.cpp -- host side of the mode table's diagnostics (tamcmc_modediag_* in include/tamcmc_accel.h): ESS,
// MCSE and split R-hat of every column, covariances and correlations between columns.  The kernels are in
// tamcmc_modediag.hip, the shared arithmetic in tamcmc_modediag.h, the object in tamcmc_modetable_obj.h.
//
// Every call works on the rows the table holds on the device and writes nothing of the table's state: it reads the
// column-major table and the Welford means.  Its own buffers hang off the object and are allocated at the first call that
// needs them: the lag products and the finish arrays (grown only when L grows), the matrix of sums and the column list of
// a covariance call (grown only when n_sel grows).  A new buffer is allocated before the old one is freed, so a call that
// runs out of memory leaves the object as it was.
#include <cmath>
#include <new>

#include "tamcmc_modetable_obj.h"
#include "tamcmc_modediag.h"

extern "C" int tamcmc_modediag_ess(tamcmc_modetable *mt, int32_t max_lag, tamcmc_modediag_totals *totals, double *ess, double *tau, double *mcse,
                                   double *rhat, int32_t *cut)
{
    if (!tm_mt_ready(mt, 4)) return TAMCMC_E_INVALID;
    if (max_lag < 0 || max_lag > TAMCMC_MODEDIAG_MAX_LAG) return TAMCMC_E_INVALID;
    const long long n = mt->n_used;
    const int L = tme_lag_limit(max_lag, n);
    const size_t nc = (size_t)mt->n_cols;
    std::vector<double> fin, m2, a0;
    std::vector<int32_t> cutv;
    try { fin.resize(TM_MD_NFIN * nc); m2.resize(nc); a0.resize(nc); cutv.resize(nc); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    int rc = tm_mt_enter(mt);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = mt->c;
    TmMtDiag &D = mt->diag;
    const size_t acc_bytes = ((size_t)(L + 1) + TM_MD_NFIN) * nc * sizeof(double), cut_bytes = nc * sizeof(int32_t);
    void *acc = nullptr, *dcut = nullptr;
    if (D.acc.reserve(acc_bytes, &acc) != TAMCMC_OK || D.cut.reserve(cut_bytes, &dcut) != TAMCMC_OK) { (void)hipFree(acc); return TAMCMC_E_NOMEM; }
    D.acc.install(acc, acc_bytes);
    D.cut.install(dcut, cut_bytes);
    D.acov_valid = false;
    TmMdArgs a{};
    a.table = mt->d_table; a.mean = mt->d_state + (size_t)TM_MT_MEAN * nc;
    a.acc = (double *)D.acc.d; a.fin = a.acc + (size_t)(L + 1) * nc; a.cut = (int32_t *)D.cut.d;
    a.n = n; a.max_samples = mt->max_samples; a.n_cols = mt->n_cols; a.L = L;
    a.tau_floor = 1.0 / std::log10((double)n);
    rc = tm_mt_timed(mt, D.clock, "modediag lag", [&] { return tm_launch_modediag_lag(a, c->stream); });
    if (rc == TAMCMC_OK) rc = tm_mt_timed(mt, D.clock, "modediag finish", [&] { return tm_launch_modediag_finish(a, c->stream); });
    if (rc != TAMCMC_OK) return rc;
    TM_HIP(hipMemcpy(fin.data(), a.fin, fin.size() * sizeof(double), hipMemcpyDeviceToHost));
    TM_HIP(hipMemcpy(cutv.data(), a.cut, nc * sizeof(int32_t), hipMemcpyDeviceToHost));
    TM_HIP(hipMemcpy(a0.data(), a.acc, nc * sizeof(double), hipMemcpyDeviceToHost));
    TM_HIP(hipMemcpy(m2.data(), mt->d_state + (size_t)TM_MT_M2 * nc, nc * sizeof(double), hipMemcpyDeviceToHost));
    D.L = L;
    D.acov_valid = true;
    const double dn = (double)n;
    for (size_t i = 0; i < nc; i++) {
        const double sd = std::sqrt(m2[i] / (dn - 1.0));                    // the sd of tamcmc_modetable_result
        if (ess) ess[i] = fin[TM_MD_ESS * nc + i];
        if (tau) tau[i] = fin[TM_MD_TAU * nc + i];
        if (mcse) mcse[i] = sd / std::sqrt(fin[TM_MD_ESS * nc + i]);
        if (rhat) rhat[i] = fin[TM_MD_RHAT * nc + i];
        if (cut) cut[i] = cutv[i];
    }
    if (totals) {
        const TmdTotals t = tmd_totals(mt->n_cols, n, L, fin.data() + TM_MD_ESS * nc, fin.data() + TM_MD_RHAT * nc, cutv.data(), a0.data());
        totals->n_used = t.n_used; totals->lag = t.lag; totals->min_ess = t.min_ess; totals->max_rhat = t.max_rhat;
        totals->col_min_ess = t.col_min_ess; totals->col_max_rhat = t.col_max_rhat;
        totals->n_truncated = t.n_truncated; totals->n_constant = t.n_constant; totals->n_rhat_high = t.n_rhat_high;
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_modediag_acov(tamcmc_modetable *mt, double *acov)
{
    if (!tm_mt_ready(mt, 4) || !acov || !mt->diag.acov_valid) return TAMCMC_E_INVALID;
    const int rc = tm_mt_enter(mt);
    if (rc != TAMCMC_OK) return rc;
    TM_HIP(hipMemcpy(acov, mt->diag.acc.d, (size_t)(mt->diag.L + 1) * (size_t)mt->n_cols * sizeof(double), hipMemcpyDeviceToHost));
    return TAMCMC_OK;
}

// S (n_sel x n_sel sums of products) of the selected columns into out, divided by n - 1
static int md_cov(tamcmc_modetable *mt, int32_t n_sel, const int32_t *cols, double *out)
{
    if (!tm_mt_ready(mt, 2) || !out) return TAMCMC_E_INVALID;
    std::vector<int32_t> sel;
    int rc = tm_mt_select(mt, n_sel, cols, sel, TAMCMC_MODEDIAG_MAX_COLS);
    if (rc != TAMCMC_OK) return rc;
    rc = tm_mt_enter(mt);
    if (rc != TAMCMC_OK) return rc;
    tamcmc_ctx *c = mt->c;
    TmMtDiag &D = mt->diag;
    const size_t ns = (size_t)n_sel, nc = (size_t)mt->n_cols, S_bytes = ns * ns * sizeof(double), sel_bytes = ns * sizeof(int32_t);
    void *S = nullptr, *dsel = nullptr;
    if (D.S.reserve(S_bytes, &S) != TAMCMC_OK || D.sel.reserve(sel_bytes, &dsel) != TAMCMC_OK) { (void)hipFree(S); return TAMCMC_E_NOMEM; }
    D.S.install(S, S_bytes);
    D.sel.install(dsel, sel_bytes);
    TM_HIP(hipMemcpy(D.sel.d, sel.data(), sel_bytes, hipMemcpyHostToDevice));
    TmMdCovArgs a{};
    a.table = mt->d_table; a.mean = mt->d_state + (size_t)TM_MT_MEAN * nc; a.sel = (const int32_t *)D.sel.d; a.S = (double *)D.S.d;
    a.n = mt->n_used; a.max_samples = mt->max_samples; a.n_cols = mt->n_cols; a.n_sel = n_sel;
    rc = tm_mt_timed(mt, D.clock, "modediag cov", [&] { return tm_launch_modediag_cov(a, c->stream); });
    if (rc != TAMCMC_OK) return rc;
    TM_HIP(hipMemcpy(out, D.S.d, S_bytes, hipMemcpyDeviceToHost));
    const double dn1 = (double)(mt->n_used - 1);
    for (size_t k = 0; k < ns * ns; k++) out[k] = out[k] / dn1;
    return TAMCMC_OK;
}

extern "C" int tamcmc_modediag_cov(tamcmc_modetable *mt, int32_t n_sel, const int32_t *cols, double *cov) { return md_cov(mt, n_sel, cols, cov); }

extern "C" int tamcmc_modediag_corr(tamcmc_modetable *mt, int32_t n_sel, const int32_t *cols, double *corr)
{
    const size_t ns = n_sel >= 1 && n_sel <= TAMCMC_MODEDIAG_MAX_COLS ? (size_t)n_sel : 0;   // (anything else: md_cov refuses it)
    std::vector<double> var;
    try { var.resize(ns); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    const int rc = md_cov(mt, n_sel, cols, corr);
    if (rc != TAMCMC_OK) return rc;
    for (size_t i = 0; i < ns; i++) var[i] = corr[i * ns + i];
    for (size_t i = 0; i < ns; i++)
        for (size_t j = 0; j < ns; j++) corr[i * ns + j] = tmd_corr(corr[i * ns + j], var[i], var[j], i == j);
    return TAMCMC_OK;
}

extern "C" int tamcmc_modediag_kernel_time(tamcmc_modetable *mt, double *total_ms, int64_t *launches)
{
    return tm_mt_idle(mt) ? mt->diag.clock.read(total_ms, launches) : TAMCMC_E_INVALID;
}
