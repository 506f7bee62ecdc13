// tamcmc_seismic_api.cpp -- host side of the mode table's seismic indices (tamcmc_modetable_indices_*,
// tamcmc_modetable_index_terms, tamcmc_seismic_kernel_time in include/tamcmc_accel_seismic.h).  The plan and the shared
// arithmetic are in tamcmc_seismic.h, the kernel in tamcmc_seismic.hip, the object in tamcmc_modetable_obj.h.
//
// enable derives the reference row through the table's own derive kernel, builds the plan from it on the host, allocates
// the block's rows, the state and the table once more for the larger number of columns and only then lets go of the old
// ones: a failure leaves the object as it was.  From then on a block of tamcmc_modetable_derive / _push runs the derive
// kernel with the total number of columns as its row stride and the indices kernel behind it (tm_seis_block); the fold and
// everything downstream see n_base_cols + n_index_cols columns and need no change.
#include <new>

#include "tamcmc_modetable_obj.h"

static void seis_info(const tamcmc_modetable *mt, tamcmc_seismic_info *info)
{
    const TmSeisPlan &P = mt->seis.plan;
    info->n_base_cols = mt->n_base_cols; info->n_index_cols = mt->n_index_cols; info->n_radial = P.n_radial;
    info->n_unassigned = P.n_unassigned; info->n_base = P.n_base; info->dnu_ref = P.dnu_ref; info->eps_ref = P.eps_ref;
}

int tm_seis_block(tamcmc_modetable *mt, int n, bool timed)
{
    const TmSeisPlan &P = mt->seis.plan;
    const size_t ni = (size_t)P.n_index(), nt = (size_t)P.n_terms();
    TmSeisArgs a{};
    a.rows = mt->d_rows; a.status = mt->d_status;
    a.first = mt->seis.d_i; a.n_num = a.first + ni + 1; a.src = a.n_num + ni; a.wsrc = a.src + nt;
    a.coef = mt->seis.d_d; a.offset = a.coef + nt;
    a.B = n; a.n_cols = mt->n_cols; a.n_base_cols = mt->n_base_cols; a.n_index = mt->n_index_cols;
    const hipStream_t stream = mt->c->stream;
    if (timed) return tm_mt_timed_record(mt, mt->seis.ev, "seismic indices", [&] { return tm_launch_seismic(a, stream); });
    const int hr = tm_launch_seismic(a, stream);
    return hr != 0 ? tm_launch_failed("seismic indices", hr) : TAMCMC_OK;
}

int tm_seis_timed_done(tamcmc_modetable *mt) { return tm_mt_timed_add(mt->seis.ev, mt->seis.clock); }

extern "C" int tamcmc_modetable_indices_enable(tamcmc_modetable *mt, int32_t Nparams, const double *ref_params, tamcmc_seismic_info *info)
{
    if (!tm_mt_idle(mt) || !ref_params || !info) return TAMCMC_E_INVALID;
    tamcmc_ctx *c = mt->c;
    if (Nparams != c->L.Nparams) return TAMCMC_E_INVALID;
    if (mt->n_index_cols > 0 || mt->n_used != 0 || mt->n_rejected != 0) return TAMCMC_E_INVALID;         // once, on an empty table
    if (mt->diag.sized_by_columns() || mt->rank.sized_by_columns()) return TAMCMC_E_INVALID;               // a diagnostics buffer exists
    const int nb = mt->n_base_cols;
    if (((size_t)nb + 1) * sizeof(double) > TM_SEIS_LDS_MAX) return TAMCMC_E_INVALID;                      // the row does not fit the kernel's LDS
    TM_HIP(hipSetDevice(c->device));
    TM_HIP(tm_ctx_stream_sync(c));

    // the reference row, by the derive kernel (one sample, the base columns)
    std::vector<double> ref;
    int32_t st = -1;
    try { ref.resize((size_t)nb); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    {
        const size_t np = (size_t)Nparams;
        TM_HIP(tm_ctx_settle(c));
        c->enq_seq++;
        TmMtDeriveArgs a{};
        a.L = c->L; a.params = mt->d_params; a.rows = mt->d_rows; a.status = mt->d_status; a.B = 1; a.n_cols = nb;
        auto fail = [&](int code) { (void)hipStreamSynchronize(c->stream); return code; };
        if (hipMemcpyAsync(mt->d_params, ref_params, np * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(TAMCMC_E_HIP);
        const int hr = tm_launch_modetable_derive(a, ((np + 1) & ~(size_t)1) * sizeof(double), c->stream);
        if (hr != 0) { (void)tm_launch_failed("modetable derive", hr); return fail(TAMCMC_E_HIP); }
        if (hipMemcpyAsync(ref.data(), mt->d_rows, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipMemcpyAsync(&st, mt->d_status, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            return fail(TAMCMC_E_HIP);
        TM_HIP(hipStreamSynchronize(c->stream));
    }
    if (st != TAMCMC_CHAIN_OK) return TAMCMC_E_INVALID;

    TmSeisPlan P;
    std::vector<TmMtCol> cols;
    std::vector<int32_t> hi;
    std::vector<double> hd;
    try {
        if (tm_seis_plan(mt->cols.data(), nb, ref.data(), P) != 0) return TAMCMC_E_INVALID;
        cols = mt->cols;
        cols.insert(cols.end(), P.cols.begin(), P.cols.end());
        hi.insert(hi.end(), P.first.begin(), P.first.end());
        hi.insert(hi.end(), P.n_num.begin(), P.n_num.end());
        hi.insert(hi.end(), P.src.begin(), P.src.end());
        hi.insert(hi.end(), P.wsrc.begin(), P.wsrc.end());
        hd.insert(hd.end(), P.coef.begin(), P.coef.end());
        hd.insert(hd.end(), P.offset.begin(), P.offset.end());
    } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    const int ni = P.n_index();
    if (ni < 1) return TAMCMC_E_INVALID;
    const int n_cols = nb + ni, B = tm_mt_block(n_cols);           // B <= the block of the base columns: d_params, d_status, d_accept stay
    const size_t nc = (size_t)n_cols;
    if (mt->max_samples > 0 && (size_t)mt->max_samples > (SIZE_MAX / sizeof(double)) / nc) return TAMCMC_E_NOMEM;

    double *rows = nullptr, *state = nullptr, *table = nullptr, *sd = nullptr;
    int32_t *si = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto fail = [&](int code) {
        (void)hipGetLastError();
        (void)hipFree(rows); (void)hipFree(state); (void)hipFree(table); (void)hipFree(si); (void)hipFree(sd);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        return code;
    };
    if (hipMalloc(&rows, (size_t)B * nc * sizeof(double)) != hipSuccess ||
        hipMalloc(&state, (2 * TM_MT_NSTATE + TM_Q_MAXQ) * nc * sizeof(double)) != hipSuccess ||
        (mt->max_samples > 0 && hipMalloc(&table, tm_mt_table_bytes(mt->max_samples, n_cols)) != hipSuccess) ||
        hipMalloc(&si, hi.size() * sizeof(int32_t)) != hipSuccess || hipMalloc(&sd, hd.size() * sizeof(double)) != hipSuccess)
        return fail(TAMCMC_E_NOMEM);
    if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess) return fail(TAMCMC_E_HIP);
    if (hipMemcpy(si, hi.data(), hi.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(sd, hd.data(), hd.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemsetAsync(state, 0, (size_t)TM_MT_NSTATE * nc * sizeof(double), c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(TAMCMC_E_HIP);

    // nothing below fails
    (void)hipFree(mt->d_rows); (void)hipFree(mt->d_state); (void)hipFree(mt->d_table);
    mt->d_rows = rows; mt->d_state = state; mt->d_table = table;
    mt->seis.d_i = si; mt->seis.d_d = sd;
    mt->seis.ev[0] = ev[0]; mt->seis.ev[1] = ev[1];
    mt->cols.swap(cols);
    mt->seis.plan = std::move(P);
    mt->n_index_cols = ni; mt->n_cols = n_cols; mt->B = B;
    mt->seis.clock.clear();
    seis_info(mt, info);
    return TAMCMC_OK;
}

extern "C" int tamcmc_modetable_indices_info(tamcmc_modetable *mt, tamcmc_seismic_info *info)
{
    if (!tm_mt_idle(mt) || !info || mt->n_index_cols < 1) return TAMCMC_E_INVALID;
    seis_info(mt, info);
    return TAMCMC_OK;
}

extern "C" int tamcmc_modetable_index_terms(tamcmc_modetable *mt, int32_t col, int32_t cap, int32_t *n_num, int32_t *n_den,
                                            int32_t *src, int32_t *wsrc, double *coef, double *offset)
{
    if (!tm_mt_idle(mt) || !n_num || !n_den) return TAMCMC_E_INVALID;
    if (col < mt->n_base_cols || col >= mt->n_cols) return TAMCMC_E_INVALID;
    const TmSeisPlan &P = mt->seis.plan;
    const size_t j = (size_t)(col - mt->n_base_cols);
    const int t0 = P.first[j], t2 = P.first[j + 1];
    *n_num = P.n_num[j];
    *n_den = t2 - t0 - P.n_num[j];
    if (cap < t2 - t0 || !src || !wsrc || !coef || !offset) return TAMCMC_E_INVALID;
    for (int t = t0; t < t2; t++) { src[t - t0] = P.src[(size_t)t]; wsrc[t - t0] = P.wsrc[(size_t)t]; coef[t - t0] = P.coef[(size_t)t]; }
    *offset = P.offset[j];
    return TAMCMC_OK;
}

extern "C" int tamcmc_seismic_kernel_time(tamcmc_modetable *mt, double *total_ms, int64_t *launches)
{
    return tm_mt_idle(mt) ? mt->seis.clock.read(total_ms, launches) : TAMCMC_E_INVALID;
}
