// tamcmc_scan_null_api.cpp -- the host side of the scan's Monte-Carlo null (tamcmc_scan_null_* in include/tamcmc_accel.h,
// tamcmc_scan_null.h): an object of its own, bound to a device and to no context or chain.  run() works the replicates in
// chunks (tmn_chunk): the extremes and the combine kernel of tamcmc_scan_null.hip on the object's stream, the chunk's 2 K
// extremes per replicate copied back, and min_log formed here with the scan's own tail functions, without FMA contraction.
// Lines and p-values are counting over what has been run so far (TmNullCalib), rebuilt when replicates have been added.
#include <hip/hip_runtime.h>
#include <cmath>
#include <new>

#pragma clang fp contract(off)

#include "tamcmc_host.h"
#include "tamcmc_scan_null.h"

struct tamcmc_scan_null {
    int device = 0;
    TmNullArgs a{};                      // the object's constants; rep0 and n are set per chunk
    TmWinShape shape[TM_SCAN_MAX_WIDTHS];
    long long first = 0;                 // global replicate of replicate 0
    long long R = 0;                     // replicates done
    long long C = 0;                     // replicates per chunk
    hipStream_t stream = nullptr;
    double *d_q = nullptr;               // [Nx], allocated by the first _variates
    // per side (0: maximum / excess, 1: minimum / deficit) and width, R each
    std::vector<double> ext[2][TM_SCAN_MAX_WIDTHS], mlog[2][TM_SCAN_MAX_WIDTHS];
    std::vector<int64_t> pos[2][TM_SCAN_MAX_WIDTHS];
    std::vector<double> h_val;           // [C][K][2] staging of a chunk
    std::vector<long long> h_pos;
    TmNullCalib calib[2];                // of the first calib[side].R replicates
    bool profile = false;
    TmTimer timer;                       // one event pair per chunk: both kernels
};

static void null_free(tamcmc_scan_null *h)
{
    (void)hipFree(h->a.part_val); (void)hipFree(h->a.part_pos); (void)hipFree(h->a.ext_val); (void)hipFree(h->a.ext_pos);
    (void)hipFree(h->d_q);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    h->timer.destroy();
    delete h;
}

extern "C" int tamcmc_scan_null_create(tamcmc_scan_null **out, int device_id, int likelihood_case, double likelihood_p, int64_t Nx,
                                       int32_t n_widths, const int32_t *W, uint64_t seed, int64_t first_replicate)
{
    if (!out) return TAMCMC_E_INVALID;
    *out = nullptr;
    if (likelihood_case != 0 && likelihood_case != 1) return TAMCMC_E_UNKNOWN_MODEL;
    if (!W || n_widths < 1 || n_widths > TAMCMC_SUMMARY_SCAN_MAX_WIDTHS || Nx < 1 || Nx > 0x7FFFFFFFLL || first_replicate < 0)
        return TAMCMC_E_INVALID;
    for (int k = 0; k < n_widths; k++)
        if (W[k] < 1 || W[k] > TAMCMC_SUMMARY_WINDOW_MAX_BINS || W[k] > Nx || (k > 0 && W[k] <= W[k - 1])) return TAMCMC_E_INVALID;
    const bool chi = likelihood_case == 0;
    if (chi && !(likelihood_p >= 1.0 && likelihood_p <= (double)TAMCMC_SUMMARY_WINDOW_MAX_SHAPE &&
                 (int)likelihood_p * W[n_widths - 1] <= TAMCMC_SUMMARY_WINDOW_MAX_SHAPE))
        return TAMCMC_E_INVALID;
    const int ndev = tamcmc_device_count();
    if (ndev <= 0 || device_id < 0 || device_id >= ndev) return TAMCMC_E_NODEVICE;

    tamcmc_scan_null *h = new (std::nothrow) tamcmc_scan_null();
    if (!h) return TAMCMC_E_NOMEM;
    h->device = device_id;
    h->first = first_replicate;
    TmNullArgs &a = h->a;
    a.seed = seed; a.Nx = Nx; a.K = n_widths;
    a.gauss = chi ? 0 : 1;
    a.p = chi ? (int)likelihood_p : 1;
    for (int k = 0; k < n_widths; k++) { a.W[k] = W[k]; h->shape[k] = tmw_shape(W[k], a.p); }
    a.tiles = (int32_t)tmn_tiles(Nx, W[0]);
    h->C = tmn_chunk(a.tiles, a.K);
    const size_t np = (size_t)h->C * (size_t)a.tiles * (size_t)a.K * 2, ne = (size_t)h->C * (size_t)a.K * 2;
    try { h->h_val.resize(ne); h->h_pos.resize(ne); } catch (const std::bad_alloc &) { delete h; return TAMCMC_E_NOMEM; }
    auto fail = [&](int rc) { (void)hipGetLastError(); null_free(h); return rc; };
    if (hipSetDevice(device_id) != hipSuccess) return fail(TAMCMC_E_NODEVICE);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { h->stream = nullptr; return fail(TAMCMC_E_HIP); }
    if (hipMalloc(&a.part_val, np * sizeof(double)) != hipSuccess || hipMalloc(&a.part_pos, np * sizeof(long long)) != hipSuccess ||
        hipMalloc(&a.ext_val, ne * sizeof(double)) != hipSuccess || hipMalloc(&a.ext_pos, ne * sizeof(long long)) != hipSuccess)
        return fail(TAMCMC_E_NOMEM);
    *out = h;
    return TAMCMC_OK;
}

extern "C" int tamcmc_scan_null_run(tamcmc_scan_null *h, int64_t n_replicates)
{
    if (!h || n_replicates < 1 || n_replicates > TM_NULL_MAX_REPLICATES - h->R) return TAMCMC_E_INVALID;
    const int K = h->a.K;
    const size_t want = (size_t)(h->R + n_replicates);
    try {
        for (int s = 0; s < 2; s++)
            for (int k = 0; k < K; k++) { h->ext[s][k].reserve(want); h->mlog[s][k].reserve(want); h->pos[s][k].reserve(want); }
    } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    TM_HIP(hipSetDevice(h->device));
    for (long long done = 0; done < n_replicates;) {
        const long long n = n_replicates - done < h->C ? n_replicates - done : h->C;
        TmNullArgs a = h->a;
        a.rep0 = (unsigned long long)(h->first + h->R);
        a.n = (int32_t)n;
        if (h->profile) { const int rc = h->timer.begin(h->stream); if (rc != TAMCMC_OK) return rc; }
        const int hr = tm_launch_scan_null(a, h->stream);
        if (hr != 0) return tm_launch_failed("scan null", hr);
        if (h->profile) { const int rc = h->timer.end(h->stream); if (rc != TAMCMC_OK) return rc; }
        const size_t ne = (size_t)n * (size_t)K * 2;
        TM_HIP(hipMemcpyAsync(h->h_val.data(), a.ext_val, ne * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        TM_HIP(hipMemcpyAsync(h->h_pos.data(), a.ext_pos, ne * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
        TM_HIP(hipStreamSynchronize(h->stream));
        for (long long r = 0; r < n; r++)
            for (int k = 0; k < K; k++)
                for (int s = 0; s < 2; s++) {
                    const size_t o = ((size_t)r * (size_t)K + (size_t)k) * 2 + (size_t)s;
                    const double S = h->h_val[o];
                    h->ext[s][k].push_back(S);
                    h->pos[s][k].push_back((int64_t)h->h_pos[o]);
                    h->mlog[s][k].push_back(tmn_min_log(h->a.gauss != 0, h->shape[k], h->a.p, s, S));
                }
        h->R += n;
        done += n;
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_scan_null_replicates(const tamcmc_scan_null *h, int64_t *R)
{
    if (!h || !R) return TAMCMC_E_INVALID;
    *R = (int64_t)h->R;
    return TAMCMC_OK;
}

extern "C" int tamcmc_scan_null_result(tamcmc_scan_null *h, int32_t k, int32_t which, double *ext_sum, int64_t *pos, double *min_log)
{
    if (!h || k < 0 || k >= h->a.K || which < 0 || which > 1) return TAMCMC_E_INVALID;
    const size_t R = (size_t)h->R;
    if (ext_sum) std::copy(h->ext[which][k].begin(), h->ext[which][k].begin() + R, ext_sum);
    if (pos) std::copy(h->pos[which][k].begin(), h->pos[which][k].begin() + R, pos);
    if (min_log) std::copy(h->mlog[which][k].begin(), h->mlog[which][k].begin() + R, min_log);
    return TAMCMC_OK;
}

// the side's calibration over all replicates done (at least one)
static int null_calib(tamcmc_scan_null *h, int32_t which, const TmNullCalib **out)
{
    TmNullCalib &c = h->calib[which];
    if (c.R != h->R) {
        try { c.build(h->a.K, h->R, h->mlog[which]); } catch (const std::bad_alloc &) { c.R = 0; return TAMCMC_E_NOMEM; }
    }
    *out = &c;
    return TAMCMC_OK;
}

extern "C" int tamcmc_scan_null_line(tamcmc_scan_null *h, int32_t k, int32_t which, double alpha, int32_t joint, double *log_below)
{
    if (!h || k < 0 || k >= h->a.K || which < 0 || which > 1 || !log_below || h->R < 1) return TAMCMC_E_INVALID;
    const TmNullCalib *c;
    const int rc = null_calib(h, which, &c);
    if (rc != TAMCMC_OK) return rc;
    const long long j = c->rank(alpha);
    if (j < 1) return TAMCMC_E_INVALID;
    *log_below = c->line(k, j, joint != 0);
    return TAMCMC_OK;
}

extern "C" int tamcmc_scan_null_pvalue(tamcmc_scan_null *h, int32_t k, int32_t which, double value, double *p_width, double *p_joint)
{
    if (!h || k < 0 || k >= h->a.K || which < 0 || which > 1 || !p_width || !p_joint || h->R < 1 || std::isnan(value)) return TAMCMC_E_INVALID;
    const TmNullCalib *c;
    const int rc = null_calib(h, which, &c);
    if (rc != TAMCMC_OK) return rc;
    c->pvalue(k, value, p_width, p_joint);
    return TAMCMC_OK;
}

extern "C" int tamcmc_scan_null_variates(tamcmc_scan_null *h, int64_t r, double *q)
{
    if (!h || !q || r < 0 || r >= TM_NULL_MAX_REPLICATES) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(h->device));
    const size_t bytes = (size_t)h->a.Nx * sizeof(double);
    if (!h->d_q && hipMalloc(&h->d_q, bytes) != hipSuccess) { (void)hipGetLastError(); h->d_q = nullptr; return TAMCMC_E_NOMEM; }
    const int hr = tm_launch_scan_null_variates(h->a, (unsigned long long)(h->first + r), h->d_q, h->stream);
    if (hr != 0) return tm_launch_failed("scan null variates", hr);
    TM_HIP(hipMemcpyAsync(q, h->d_q, bytes, hipMemcpyDeviceToHost, h->stream));
    TM_HIP(hipStreamSynchronize(h->stream));
    return TAMCMC_OK;
}

extern "C" int tamcmc_scan_null_profile(tamcmc_scan_null *h, int enable)
{
    if (!h) return TAMCMC_E_INVALID;
    h->profile = enable != 0;
    h->timer.used = 0;
    return TAMCMC_OK;
}

extern "C" int tamcmc_scan_null_kernel_time(tamcmc_scan_null *h, double *total_ms, int64_t *launches)
{
    if (!h || !total_ms || !launches) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(h->device));
    TM_HIP(hipStreamSynchronize(h->stream));
    return h->timer.total(total_ms, launches);
}

extern "C" int tamcmc_scan_null_destroy(tamcmc_scan_null *h)
{
    if (!h) return TAMCMC_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    null_free(h);
    return TAMCMC_OK;
}
