// tamcmc_modepdf_api.cpp -- host side of the mode table's marginal histograms, shortest intervals and pair densities
// (tamcmc_modepdf_* in include/tamcmc_accel_pdf.h).  The kernels are in tamcmc_modepdf.hip, the shared arithmetic in
// tamcmc_modepdf.h; the sorted keys of _hpd come from tamcmc_moderank.hip's sort kernel, launched on this file's own scratch.
//
// A call writes nothing of the table's state and nothing of tamcmc_modediag_*'s or tamcmc_moderank_*'s buffers.  Its one
// device buffer hangs off the object, grown only when a call needs more, the new one allocated before the old one is freed:
// a call that cannot have it returns TAMCMC_E_NOMEM with the object as it was.  The ranges, the scales and the window
// lengths are formed here, once per column; the uint32 counters of the kernels are widened here.
#include <cmath>
#include <new>

#include "tamcmc_modetable_obj.h"
#include "tamcmc_moderank.h"
#include "tamcmc_modepdf.h"
#include "tamcmc_accel_pdf.h"

// The scratch at `bytes` or more, then the entry.  The scratch comes first: a call that cannot have it returns
// TAMCMC_E_NOMEM with the object, its context's counters included, as it was.
static int pdf_enter(tamcmc_modetable *mt, const size_t bytes)
{
    TM_HIP(hipSetDevice(mt->c->device));
    void *grown = nullptr;
    int rc = mt->pdf.scratch.reserve(bytes, &grown);
    if (rc != TAMCMC_OK) return rc;
    rc = tm_mt_enter(mt);
    if (rc != TAMCMC_OK) { (void)hipFree(grown); return rc; }
    mt->pdf.scratch.install(grown, bytes);
    return TAMCMC_OK;
}

// the ranges of `m` columns: explicit ones checked (refused: false), default ones the table's min and max as
// tamcmc_modetable_result returns them (read once into `state`), with status TM_PDF_RANGE where they cannot be used
static bool pdf_ranges(const tamcmc_modetable *mt, const size_t m, const int32_t *col, const double *lo, const double *hi, const int n_bins,
                       const std::vector<double> &state, double *rlo, double *rhi, double *rs, int32_t *status)
{
    const size_t nc = (size_t)mt->n_cols;
    for (size_t j = 0; j < m; j++) {
        if (lo) {
            if (!tmp_range_ok(lo[j], hi[j])) return false;
            rlo[j] = lo[j]; rhi[j] = hi[j]; status[j] = 0;
        } else {
            rlo[j] = state[TM_MT_MIN * nc + (size_t)col[j]];
            rhi[j] = state[TM_MT_MAX * nc + (size_t)col[j]];
            status[j] = tmp_range_ok(rlo[j], rhi[j]) ? 0 : TM_PDF_RANGE;
        }
        rs[j] = status[j] == 0 ? tmp_scale(rlo[j], rhi[j], n_bins) : 0.0;
    }
    return true;
}

extern "C" int tamcmc_modepdf_hist(tamcmc_modetable *mt, int32_t n_bins, int32_t n_sel, const int32_t *cols, const double *lo, const double *hi,
                                   int64_t *counts, int64_t *below, int64_t *above, double *range, int32_t *status)
{
    if (!tm_mt_ready(mt, 1)) return TAMCMC_E_INVALID;
    if (n_bins < 1 || n_bins > TAMCMC_MODEPDF_MAX_BINS || !counts || !below || !above || (lo == nullptr) != (hi == nullptr)) return TAMCMC_E_INVALID;
    std::vector<int32_t> sel, st;
    int rc = tm_mt_select(mt, n_sel, cols, sel);
    if (rc != TAMCMC_OK) return rc;
    const size_t ns = (size_t)n_sel, nb2 = (size_t)n_bins + 2;
    std::vector<double> state, arg;
    std::vector<uint32_t> cnt;
    try { st.resize(ns); arg.resize(3 * ns); cnt.resize(ns * nb2); if (!lo) state.resize(mt->state_doubles()); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    if (lo && !pdf_ranges(mt, ns, sel.data(), lo, hi, n_bins, state, arg.data(), arg.data() + ns, arg.data() + 2 * ns, st.data())) return TAMCMC_E_INVALID;
    // device buffer: lo, hi, s [n_sel] doubles each; counters [n_sel][n_bins + 2]; sel, status [n_sel]
    const size_t bytes = 3 * ns * sizeof(double) + ns * nb2 * sizeof(uint32_t) + 2 * ns * sizeof(int32_t);
    rc = pdf_enter(mt, bytes);
    if (rc != TAMCMC_OK) return rc;
    if (!lo) {
        TM_HIP(hipMemcpy(state.data(), mt->d_state, state.size() * sizeof(double), hipMemcpyDeviceToHost));
        (void)pdf_ranges(mt, ns, sel.data(), nullptr, nullptr, n_bins, state, arg.data(), arg.data() + ns, arg.data() + 2 * ns, st.data());
    }
    double *d_arg = (double *)mt->pdf.scratch.d;
    uint32_t *d_cnt = (uint32_t *)(d_arg + 3 * ns);
    int32_t *d_sel = (int32_t *)(d_cnt + ns * nb2);
    TM_HIP(hipMemcpy(d_arg, arg.data(), 3 * ns * sizeof(double), hipMemcpyHostToDevice));
    TM_HIP(hipMemcpy(d_sel, sel.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice));
    TM_HIP(hipMemcpy(d_sel + ns, st.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice));
    TmPdfHistArgs a{};
    a.table = mt->d_table; a.sel = d_sel; a.status = d_sel + ns; a.lo = d_arg; a.hi = d_arg + ns; a.s = d_arg + 2 * ns; a.out = d_cnt;
    a.n = mt->n_used; a.max_samples = mt->max_samples; a.n_sel = n_sel; a.n_bins = n_bins;
    rc = tm_mt_timed(mt, mt->pdf.clock, "modepdf hist", [&] { return tm_launch_modepdf_hist(a, mt->c->stream); });
    if (rc != TAMCMC_OK) return rc;
    TM_HIP(hipMemcpy(cnt.data(), d_cnt, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t j = 0; j < ns; j++) {
        const uint32_t *c = cnt.data() + j * nb2;
        for (size_t b = 0; b < (size_t)n_bins; b++) counts[j * (size_t)n_bins + b] = (int64_t)c[b];
        below[j] = (int64_t)c[n_bins]; above[j] = (int64_t)c[n_bins + 1];
        if (range) { range[2 * j] = arg[j]; range[2 * j + 1] = arg[ns + j]; }
        if (status) status[j] = st[j];
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_modepdf_hist2d(tamcmc_modetable *mt, int32_t n_bins, int32_t n_pairs, const int32_t *pairs, const double *lo,
                                     const double *hi, int32_t n_mass, const double *mass, int64_t *counts, int64_t *outside, int64_t *level,
                                     int32_t *status)
{
    if (!tm_mt_ready(mt, 1)) return TAMCMC_E_INVALID;
    if (n_bins < 1 || n_bins > TAMCMC_MODEPDF_MAX_BINS2D || n_pairs < 1 || n_pairs > TAMCMC_MODEPDF_MAX_PAIRS || !pairs || !counts || !outside ||
        (lo == nullptr) != (hi == nullptr) || n_mass < 0 || n_mass > TAMCMC_MODEPDF_MAX_MASS || (n_mass > 0 && (!mass || !level)))
        return TAMCMC_E_INVALID;
    for (int32_t k = 0; k < 2 * n_pairs; k++)
        if (pairs[k] < 0 || pairs[k] >= mt->n_cols) return TAMCMC_E_INVALID;
    for (int32_t m = 0; m < n_mass; m++)
        if (!tmp_mass_ok(mass[m])) return TAMCMC_E_INVALID;
    const size_t np = (size_t)n_pairs, cells = (size_t)n_bins * (size_t)n_bins;
    std::vector<int32_t> st, pst;
    std::vector<double> state, arg;
    std::vector<uint32_t> cnt;
    try {
        st.resize(2 * np); pst.resize(np); arg.resize(6 * np); cnt.resize(np * (cells + 1));
        if (!lo) state.resize(mt->state_doubles());
    } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    if (lo && !pdf_ranges(mt, 2 * np, pairs, lo, hi, n_bins, state, arg.data(), arg.data() + 2 * np, arg.data() + 4 * np, st.data())) return TAMCMC_E_INVALID;
    // device buffer: lo, hi, s [n_pairs][2] doubles each; counters [n_pairs][cells + 1]; pairs [n_pairs][2], status [n_pairs]
    const size_t bytes = 6 * np * sizeof(double) + np * (cells + 1) * sizeof(uint32_t) + 3 * np * sizeof(int32_t);
    int rc = pdf_enter(mt, bytes);
    if (rc != TAMCMC_OK) return rc;
    if (!lo) {
        TM_HIP(hipMemcpy(state.data(), mt->d_state, state.size() * sizeof(double), hipMemcpyDeviceToHost));
        (void)pdf_ranges(mt, 2 * np, pairs, nullptr, nullptr, n_bins, state, arg.data(), arg.data() + 2 * np, arg.data() + 4 * np, st.data());
    }
    for (size_t p = 0; p < np; p++) pst[p] = (st[2 * p] || st[2 * p + 1]) ? TM_PDF_RANGE : 0;
    double *d_arg = (double *)mt->pdf.scratch.d;
    uint32_t *d_cnt = (uint32_t *)(d_arg + 6 * np);
    int32_t *d_pairs = (int32_t *)(d_cnt + np * (cells + 1));
    TM_HIP(hipMemcpy(d_arg, arg.data(), 6 * np * sizeof(double), hipMemcpyHostToDevice));
    TM_HIP(hipMemcpy(d_pairs, pairs, 2 * np * sizeof(int32_t), hipMemcpyHostToDevice));
    TM_HIP(hipMemcpy(d_pairs + 2 * np, pst.data(), np * sizeof(int32_t), hipMemcpyHostToDevice));
    TmPdfPairArgs a{};
    a.table = mt->d_table; a.pairs = d_pairs; a.status = d_pairs + 2 * np; a.lo = d_arg; a.hi = d_arg + 2 * np; a.s = d_arg + 4 * np; a.out = d_cnt;
    a.n = mt->n_used; a.max_samples = mt->max_samples; a.n_pairs = n_pairs; a.n_bins = n_bins;
    rc = tm_mt_timed(mt, mt->pdf.clock, "modepdf pair", [&] { return tm_launch_modepdf_pair(a, mt->c->stream); });
    if (rc != TAMCMC_OK) return rc;
    TM_HIP(hipMemcpy(cnt.data(), d_cnt, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t p = 0; p < np; p++) {
        const uint32_t *c = cnt.data() + p * (cells + 1);
        int64_t *out = counts + p * cells, n_in = 0;
        for (size_t b = 0; b < cells; b++) { out[b] = (int64_t)c[b]; n_in += out[b]; }
        outside[p] = (int64_t)c[cells];
        if (status) status[p] = pst[p];
        if (n_mass > 0) {
            std::vector<int64_t> desc;
            try { desc = tmp_sorted_counts(out, cells); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
            for (int32_t m = 0; m < n_mass; m++) level[(size_t)m * np + p] = tmp_level(desc, n_in, mass[m]);
        }
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_modepdf_hpd(tamcmc_modetable *mt, int32_t n_mass, const double *mass, int32_t n_sel, const int32_t *cols,
                                  int64_t scratch_bytes, int64_t *k, int64_t *start, double *lo, double *hi)
{
    if (!tm_mt_ready(mt, 4)) return TAMCMC_E_INVALID;
    if (n_mass < 1 || n_mass > TAMCMC_MODEPDF_MAX_MASS || !mass || scratch_bytes < 0 || !start || !lo || !hi) return TAMCMC_E_INVALID;
    for (int32_t m = 0; m < n_mass; m++)
        if (!tmp_mass_ok(mass[m])) return TAMCMC_E_INVALID;
    std::vector<int32_t> sel;
    int rc = tm_mt_select(mt, n_sel, cols, sel);
    if (rc != TAMCMC_OK) return rc;
    const long long n = mt->n_used, P = tmr_padded(n);
    long long kk[TM_PDF_MAX_MASS] = {};
    for (int32_t m = 0; m < n_mass; m++) kk[m] = tmp_window(mass[m], n);
    // chunks of w columns: w * tmp_hpd_col_bytes and the window lengths fit the scratch; at least one column
    const size_t ns = (size_t)n_sel, nm = (size_t)n_mass, per = tmp_hpd_col_bytes(P, n_mass), fixed = TM_PDF_MAX_MASS * sizeof(long long);
    const size_t budget = scratch_bytes ? (size_t)scratch_bytes : (size_t)TM_PDF_DEFAULT_SCRATCH;
    const int w = tm_mt_chunk_width(budget, fixed, per, ns, 65535);
    std::vector<double> res;
    try { res.resize(3 * nm * (size_t)w); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    const size_t bytes = fixed + (size_t)w * per;
    rc = pdf_enter(mt, bytes);
    if (rc != TAMCMC_OK) return rc;
    // the 8-byte arrays first: k [TM_PDF_MAX_MASS], keys [w][P], start, lo, hi [n_mass][w] each, then sel [w]
    long long *d_k = (long long *)mt->pdf.scratch.d;
    uint64_t *d_keys = (uint64_t *)(d_k + TM_PDF_MAX_MASS);
    long long *d_start = (long long *)(d_keys + (size_t)w * (size_t)P);
    double *d_lo = (double *)(d_start + nm * (size_t)w), *d_hi = d_lo + nm * (size_t)w;
    int32_t *d_sel = (int32_t *)(d_hi + nm * (size_t)w);
    TM_HIP(hipMemcpy(d_k, kk, sizeof(kk), hipMemcpyHostToDevice));
    for (size_t k0 = 0; k0 < ns; k0 += (size_t)w) {
        const int wc = ns - k0 < (size_t)w ? (int)(ns - k0) : w;
        TM_HIP(hipMemcpy(d_sel, sel.data() + k0, (size_t)wc * sizeof(int32_t), hipMemcpyHostToDevice));
        const TmMrArgs r = tmr_sort_args(mt->d_table, d_sel, d_keys, n, mt->max_samples, P, wc);
        rc = tm_mt_timed(mt, mt->pdf.clock, "modepdf sort", [&] { return tm_launch_moderank_sort(r, 0, mt->c->stream); });
        if (rc != TAMCMC_OK) return rc;
        TmPdfHpdArgs a{};
        a.keys = d_keys; a.k = d_k; a.start = d_start; a.lo = d_lo; a.hi = d_hi; a.n = n; a.P = P; a.w = wc; a.n_mass = n_mass;
        rc = tm_mt_timed(mt, mt->pdf.clock, "modepdf hpd", [&] { return tm_launch_modepdf_hpd(a, mt->c->stream); });
        if (rc != TAMCMC_OK) return rc;
        // start, lo, hi lie one behind the other, [n_mass][wc] each with the chunk's own width
        const size_t m1 = nm * (size_t)wc;
        TM_HIP(hipMemcpy(res.data(), d_start, m1 * sizeof(long long), hipMemcpyDeviceToHost));
        TM_HIP(hipMemcpy(res.data() + m1, d_lo, m1 * sizeof(double), hipMemcpyDeviceToHost));
        TM_HIP(hipMemcpy(res.data() + 2 * m1, d_hi, m1 * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t m = 0; m < nm; m++)
            for (size_t c = 0; c < (size_t)wc; c++) {
                long long s;
                std::memcpy(&s, &res[m * (size_t)wc + c], sizeof(s));
                start[m * ns + k0 + c] = (int64_t)s;
                lo[m * ns + k0 + c] = res[m1 + m * (size_t)wc + c];
                hi[m * ns + k0 + c] = res[2 * m1 + m * (size_t)wc + c];
            }
    }
    if (k) for (int32_t m = 0; m < n_mass; m++) k[m] = (int64_t)kk[m];
    return TAMCMC_OK;
}

extern "C" int tamcmc_modepdf_kernel_time(tamcmc_modetable *mt, double *total_ms, int64_t *launches)
{
    return tm_mt_idle(mt) ? mt->pdf.clock.read(total_ms, launches) : TAMCMC_E_INVALID;
}
