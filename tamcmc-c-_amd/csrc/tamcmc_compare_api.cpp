// tamcmc_compare_api.cpp -- the host side of the comparison of fits (tamcmc_compare_* in include/tamcmc_accel_compare.h,
// tamcmc_compare.h): an object of its own, bound to a device and to no context or chain.  create() copies the inputs, counts
// the included units and puts elpd on the device.  diff() is the host's long-double walk.  bootstrap() works the replicates
// in chunks (tmc_chunk): the sums and the finish kernel of tamcmc_compare.hip on the object's stream, the chunk's z copied
// back; prob, interval and the weights are counting over the z so far.  stacking() runs the prepare kernel when the table of
// P fits, then groups of iterations, looking at the device's state after each group.
#include <hip/hip_runtime.h>
#include <cmath>
#include <new>

#pragma clang fp contract(off)

#include "tamcmc_host.h"
#include "tamcmc_compare.h"

struct tamcmc_compare {
    int device = 0;
    int K = 0;
    long long N = 0, Np = 0;
    double scale = 1.0;
    unsigned long long seed = 0;
    long long first = 0;                 // global replicate of replicate 0
    long long R = 0;                     // replicates done
    std::vector<double> elpd, khat;      // [K][N]; khat empty: none given
    std::vector<double> z;               // [R][K - 1]
    std::vector<double> h_z;             // staging of a chunk
    hipStream_t stream = nullptr;
    double *d_elpd = nullptr;
    double *d_part = nullptr, *d_z = nullptr;
    long long C = 0;                     // replicates the partials and d_z have room for
    double *d_e = nullptr;               // [N], allocated by the first _variates
    double *d_P = nullptr;               // [K][N], allocated by the first stacking that keeps the table
    double *d_spart = nullptr;           // [stack tiles][TM_CMP_STACK_COLS]
    TmCmpStack *d_state = nullptr;
    int cadence = 16;
    bool have_stack = false;
    double stack_w[TM_CMP_MAX_FITS] = {0.0};
    bool profile = false;
    TmTimer timer[2];                    // 0: one event pair per chunk of the bootstrap; 1: per launch group of the stacking
};

static void compare_free(tamcmc_compare *h)
{
    (void)hipFree(h->d_elpd); (void)hipFree(h->d_part); (void)hipFree(h->d_z); (void)hipFree(h->d_e); (void)hipFree(h->d_P);
    (void)hipFree(h->d_spart); (void)hipFree(h->d_state);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    h->timer[0].destroy(); h->timer[1].destroy();
    delete h;
}

extern "C" int tamcmc_compare_create(tamcmc_compare **out, int device_id, int32_t K, int64_t N, const double *elpd, const double *pareto_k,
                                     double scale, uint64_t seed, int64_t first_replicate)
{
    if (!out) return TAMCMC_E_INVALID;
    *out = nullptr;
    if (K < 2 || K > TAMCMC_COMPARE_MAX_FITS || N < 1 || N > 0x7FFFFFFFLL || !elpd || !(scale > 0.0) || !tmc_finite(scale) || first_replicate < 0)
        return TAMCMC_E_INVALID;
    const int ndev = tamcmc_device_count();
    if (ndev <= 0 || device_id < 0 || device_id >= ndev) return TAMCMC_E_NODEVICE;

    tamcmc_compare *h = new (std::nothrow) tamcmc_compare();
    if (!h) return TAMCMC_E_NOMEM;
    h->device = device_id; h->K = K; h->N = N; h->scale = scale; h->seed = seed; h->first = first_replicate;
    const size_t n = (size_t)K * (size_t)N;
    try {
        h->elpd.assign(elpd, elpd + n);
        if (pareto_k) h->khat.assign(pareto_k, pareto_k + n);
    } catch (const std::bad_alloc &) { delete h; return TAMCMC_E_NOMEM; }
    for (long long i = 0; i < N; i++) h->Np += tmc_included(K, h->elpd.data(), N, i) ? 1 : 0;
    auto fail = [&](int rc) { (void)hipGetLastError(); compare_free(h); return rc; };
    if (hipSetDevice(device_id) != hipSuccess) return fail(TAMCMC_E_NODEVICE);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { h->stream = nullptr; return fail(TAMCMC_E_HIP); }
    if (hipMalloc(&h->d_elpd, n * sizeof(double)) != hipSuccess) return fail(TAMCMC_E_NOMEM);
    if (hipMemcpyAsync(h->d_elpd, h->elpd.data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
        return fail(TAMCMC_E_HIP);
    *out = h;
    return TAMCMC_OK;
}

extern "C" int tamcmc_compare_info(const tamcmc_compare *h, int64_t *n_included, int64_t *n_excluded)
{
    if (!h || !n_included || !n_excluded) return TAMCMC_E_INVALID;
    *n_included = (int64_t)h->Np;
    *n_excluded = (int64_t)(h->N - h->Np);
    return TAMCMC_OK;
}

extern "C" int tamcmc_compare_diff(const tamcmc_compare *h, int32_t a, int32_t b, tamcmc_compare_totals *totals)
{
    if (!h || !totals || a < 0 || a >= h->K || b < 0 || b >= h->K) return TAMCMC_E_INVALID;
    const TmCmpTotals t = tmc_pair_totals(h->K, h->N, h->elpd.data(), h->khat.empty() ? nullptr : h->khat.data(), a, b);
    totals->n_included = t.n_included; totals->n_excluded = t.n_excluded; totals->n_better = t.n_better; totals->n_worse = t.n_worse;
    totals->n_k_high = t.n_k_high; totals->elpd_diff = t.elpd_diff; totals->se_diff = t.se_diff; totals->diff_k_high = t.diff_k_high;
    return TAMCMC_OK;
}

static TmCmpArgs compare_args(const tamcmc_compare *h)
{
    TmCmpArgs a{};
    a.elpd = h->d_elpd; a.part = h->d_part; a.z = h->d_z; a.seed = h->seed; a.N = h->N; a.Np = h->Np; a.K = h->K;
    a.tiles = (int32_t)tmc_tiles(h->N);
    return a;
}

extern "C" int tamcmc_compare_bootstrap(tamcmc_compare *h, int64_t n_replicates, int64_t scratch_bytes)
{
    if (!h || n_replicates < 1 || n_replicates > TM_CMP_MAX_REPLICATES - h->R || scratch_bytes < 0 || h->Np < 1) return TAMCMC_E_INVALID;
    const int K = h->K;
    const long long tiles = tmc_tiles(h->N);
    const long long C = tmc_chunk(scratch_bytes, tiles, K);
    try { h->z.reserve((size_t)(h->R + n_replicates) * (size_t)(K - 1)); h->h_z.resize((size_t)C * (size_t)(K - 1)); }
    catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    TM_HIP(hipSetDevice(h->device));
    if (C > h->C) {
        TM_HIP(hipStreamSynchronize(h->stream));
        (void)hipFree(h->d_part); (void)hipFree(h->d_z);
        h->d_part = h->d_z = nullptr; h->C = 0;
        const size_t np = (size_t)tmc_slots_max(C) * 2 * (size_t)tiles * (size_t)K;
        if (hipMalloc(&h->d_part, np * sizeof(double)) != hipSuccess || hipMalloc(&h->d_z, (size_t)C * (size_t)(K - 1) * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(h->d_part); (void)hipFree(h->d_z);
            h->d_part = h->d_z = nullptr;
            return TAMCMC_E_NOMEM;
        }
        h->C = C;
    }
    for (long long done = 0; done < n_replicates;) {
        const long long n = n_replicates - done < C ? n_replicates - done : C;
        TmCmpArgs a = compare_args(h);
        a.g0 = (unsigned long long)(h->first + h->R);
        a.n = (int32_t)n;
        if (h->profile) { const int rc = h->timer[0].begin(h->stream); if (rc != TAMCMC_OK) return rc; }
        const int hr = tm_launch_compare_bootstrap(a, h->stream);
        if (hr != 0) return tm_launch_failed("compare bootstrap", hr);
        if (h->profile) { const int rc = h->timer[0].end(h->stream); if (rc != TAMCMC_OK) return rc; }
        const size_t nz = (size_t)n * (size_t)(K - 1);
        TM_HIP(hipMemcpyAsync(h->h_z.data(), h->d_z, nz * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        TM_HIP(hipStreamSynchronize(h->stream));
        h->z.insert(h->z.end(), h->h_z.begin(), h->h_z.begin() + nz);
        h->R += n;
        done += n;
    }
    return TAMCMC_OK;
}

extern "C" int tamcmc_compare_replicates(const tamcmc_compare *h, int64_t *R)
{
    if (!h || !R) return TAMCMC_E_INVALID;
    *R = (int64_t)h->R;
    return TAMCMC_OK;
}

extern "C" int tamcmc_compare_z(const tamcmc_compare *h, int32_t k, double *out)
{
    if (!h || !out || k < 0 || k >= h->K) return TAMCMC_E_INVALID;
    for (long long r = 0; r < h->R; r++) out[r] = tmc_z_at(h->z.data(), h->K, r, k);
    return TAMCMC_OK;
}

extern "C" int tamcmc_compare_prob(const tamcmc_compare *h, int32_t a, int32_t b, int64_t *n_greater, int64_t *n_equal)
{
    if (!h || !n_greater || !n_equal || a < 0 || a >= h->K || b < 0 || b >= h->K || h->R < 1) return TAMCMC_E_INVALID;
    long long gt, eq;
    tmc_prob(h->z.data(), h->K, h->R, a, b, &gt, &eq);
    *n_greater = (int64_t)gt; *n_equal = (int64_t)eq;
    return TAMCMC_OK;
}

extern "C" int tamcmc_compare_interval(const tamcmc_compare *h, int32_t a, int32_t b, double q, double *value)
{
    if (!h || !value || a < 0 || a >= h->K || b < 0 || b >= h->K || h->R < 1 || !(q >= 0.0 && q <= 1.0)) return TAMCMC_E_INVALID;
    try { *value = tmc_interval(h->z.data(), h->K, h->R, a, b, q); } catch (const std::bad_alloc &) { return TAMCMC_E_NOMEM; }
    return TAMCMC_OK;
}

extern "C" int tamcmc_compare_weights(const tamcmc_compare *h, int32_t method, double *w)
{
    if (!h || !w) return TAMCMC_E_INVALID;
    const int K = h->K;
    if (method == TAMCMC_COMPARE_PSEUDO_BMA) {
        if (h->Np < 1) return TAMCMC_E_INVALID;
        double x[TM_CMP_MAX_FITS];
        for (int k = 0; k < K; k++) x[k] = h->scale * tmc_pair_totals(K, h->N, h->elpd.data(), nullptr, k, 0).elpd_diff;
        tmc_softmax(K, x, w);
        return TAMCMC_OK;
    }
    if (method == TAMCMC_COMPARE_PSEUDO_BMA_PLUS) {
        if (h->R < 1) return TAMCMC_E_INVALID;
        tmc_bma_plus(h->z.data(), K, h->R, h->scale, w);
        return TAMCMC_OK;
    }
    if (method == TAMCMC_COMPARE_STACKING) {
        if (!h->have_stack) return TAMCMC_E_INVALID;
        for (int k = 0; k < K; k++) w[k] = h->stack_w[k];
        return TAMCMC_OK;
    }
    return TAMCMC_E_INVALID;
}

extern "C" int tamcmc_compare_stacking_cadence(tamcmc_compare *h, int32_t iterations_per_look)
{
    if (!h || iterations_per_look < 1 || iterations_per_look > 4096) return TAMCMC_E_INVALID;
    h->cadence = iterations_per_look;
    return TAMCMC_OK;
}

extern "C" int tamcmc_compare_stacking(tamcmc_compare *h, double tol, int64_t max_iter, int64_t scratch_bytes, double *w,
                                       tamcmc_compare_stacking_info *info)
{
    if (!h || !w || !(tol >= 0.0) || !tmc_finite(tol) || max_iter < 1 || max_iter > ((int64_t)1 << 24) || scratch_bytes < 0 || h->Np < 1)
        return TAMCMC_E_INVALID;
    const int K = h->K;
    const long long tiles = tmc_stack_tiles(h->N);
    const size_t table_bytes = (size_t)K * (size_t)h->N * sizeof(double);
    const bool table = table_bytes <= (size_t)(scratch_bytes > 0 ? scratch_bytes : TM_CMP_STACK_SCRATCH);
    TM_HIP(hipSetDevice(h->device));
    auto nomem = [&]() { (void)hipGetLastError(); return TAMCMC_E_NOMEM; };
    if (!h->d_spart && hipMalloc(&h->d_spart, (size_t)tiles * TM_CMP_STACK_COLS * sizeof(double)) != hipSuccess) { h->d_spart = nullptr; return nomem(); }
    if (!h->d_state && hipMalloc(&h->d_state, sizeof(TmCmpStack)) != hipSuccess) { h->d_state = nullptr; return nomem(); }
    if (table && !h->d_P && hipMalloc(&h->d_P, table_bytes) != hipSuccess) { h->d_P = nullptr; return nomem(); }

    TmCmpStackArgs a{};
    a.elpd = h->d_elpd; a.P = table ? h->d_P : nullptr; a.part = h->d_spart; a.state = h->d_state;
    a.scale = h->scale; a.tol = tol; a.N = h->N; a.Np = h->Np; a.max_iter = max_iter; a.K = K; a.tiles = (int32_t)tiles;
    TmCmpStack st;
    tmc_em_init(K, &st);
    TM_HIP(hipMemcpyAsync(h->d_state, &st, sizeof(st), hipMemcpyHostToDevice, h->stream));
    TM_HIP(hipStreamSynchronize(h->stream));                 // (st is on this frame)
    if (table) {
        if (h->profile) { const int rc = h->timer[1].begin(h->stream); if (rc != TAMCMC_OK) return rc; }
        const int hr = tm_launch_compare_prepare(a, h->stream);
        if (hr != 0) return tm_launch_failed("compare prepare", hr);
        if (h->profile) { const int rc = h->timer[1].end(h->stream); if (rc != TAMCMC_OK) return rc; }
    }
    for (long long launched = 0; !st.frozen && launched < max_iter;) {
        const long long left = max_iter - launched;
        const int n = (int)(left < h->cadence ? left : h->cadence);
        if (h->profile) { const int rc = h->timer[1].begin(h->stream); if (rc != TAMCMC_OK) return rc; }
        const int hr = tm_launch_compare_iterations(a, n, h->stream);
        if (hr != 0) return tm_launch_failed("compare stacking", hr);
        if (h->profile) { const int rc = h->timer[1].end(h->stream); if (rc != TAMCMC_OK) return rc; }
        TM_HIP(hipMemcpyAsync(&st, h->d_state, sizeof(st), hipMemcpyDeviceToHost, h->stream));
        TM_HIP(hipStreamSynchronize(h->stream));
        launched += n;
    }
    for (int k = 0; k < K; k++) { w[k] = st.w[k]; h->stack_w[k] = st.w[k]; }
    h->have_stack = true;
    if (info) { info->iterations = (int64_t)st.iterations; info->converged = st.converged; info->table = table ? 1 : 0; info->gap = st.gap; info->f = st.f; }
    return TAMCMC_OK;
}

extern "C" int tamcmc_compare_variates(tamcmc_compare *h, int64_t r, double *e)
{
    if (!h || !e || r < 0 || r >= TM_CMP_MAX_REPLICATES) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(h->device));
    const size_t bytes = (size_t)h->N * sizeof(double);
    if (!h->d_e && hipMalloc(&h->d_e, bytes) != hipSuccess) { (void)hipGetLastError(); h->d_e = nullptr; return TAMCMC_E_NOMEM; }
    const int hr = tm_launch_compare_variates(compare_args(h), (unsigned long long)(h->first + r), h->d_e, h->stream);
    if (hr != 0) return tm_launch_failed("compare variates", hr);
    TM_HIP(hipMemcpyAsync(e, h->d_e, bytes, hipMemcpyDeviceToHost, h->stream));
    TM_HIP(hipStreamSynchronize(h->stream));
    return TAMCMC_OK;
}

extern "C" int tamcmc_compare_profile(tamcmc_compare *h, int enable)
{
    if (!h) return TAMCMC_E_INVALID;
    h->profile = enable != 0;
    h->timer[0].used = 0; h->timer[1].used = 0;
    return TAMCMC_OK;
}

extern "C" int tamcmc_compare_kernel_time(tamcmc_compare *h, int32_t which, double *total_ms, int64_t *launches)
{
    if (!h || !total_ms || !launches || which < 0 || which > 1) return TAMCMC_E_INVALID;
    TM_HIP(hipSetDevice(h->device));
    TM_HIP(hipStreamSynchronize(h->stream));
    return h->timer[which].total(total_ms, launches);
}

extern "C" int tamcmc_compare_destroy(tamcmc_compare *h)
{
    if (!h) return TAMCMC_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    compare_free(h);
    return TAMCMC_OK;
}
