// tamcmc_modepdf.hip -- the kernels behind tamcmc_modepdf_* (tamcmc_modepdf.h): the histogram of a column, the joint
// histogram of a pair of columns, and the shortest window of a sorted column.  The sorted keys are those of
// tamcmc_moderank.hip's sort kernel.  fp64 and integer VALU, LDS integer atomics; no MFMA, no atomics on device memory,
// no waiting across workgroups.
//
//   hist   one workgroup of 512 threads per selected column: n_bins uint32 counters (at most 16 KiB) and below / above in
//          LDS; the column is read with coalesced 8-byte loads, 4 in flight per thread; a wave whose active lanes all
//          hit one counter (a constant column, an integer window edge) adds their number once, any other wave adds per
//          lane.  The counters leave with plain stores.
//   pair   one workgroup per pair: n_bins^2 counters of dynamic LDS (64 KiB at 128), `outside` beside them; else as hist.
//   hpd    one workgroup of 256 threads per (column, mass): each thread walks i with the workgroup's stride and keeps the
//          first (width, i) under tmp_before, then a wave reduction by shuffles and one LDS step over the four waves.
#include <hip/hip_runtime.h>
#include <cmath>

// no FMA contraction anywhere in this file
#pragma clang fp contract(off)

#include "tamcmc_modepdf.h"

// one to the counter `at` of every active lane (all lanes of a wave call this together; `live` lanes add)
__device__ __forceinline__ void pdf_add(uint32_t *cnt, const int at, const bool live)
{
    const unsigned long long act = __ballot(live);
    if (act == 0) return;
    const int lead = __ffsll((long long)act) - 1;
    const int first = __shfl(at, lead);
    if (__ballot(live && at == first) == act) {              // one counter for the whole wave
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(cnt + first, (uint32_t)__popcll(act));
    } else if (live) {
        atomicAdd(cnt + at, 1u);
    }
}

__global__ __launch_bounds__(TM_PDF_THREADS) void tamcmc_modepdf_hist_kernel(const TmPdfHistArgs a)
{
    __shared__ uint32_t s_cnt[TM_PDF_MAX_BINS + 2];          // the classes, then below, above
    const int c = blockIdx.x, tid = threadIdx.x;
    if (c >= a.n_sel) return;
    const int nb = a.n_bins;
    for (int b = tid; b < nb + 2; b += TM_PDF_THREADS) s_cnt[b] = 0;
    __syncthreads();
    if (a.status[c] == 0) {
        const double *__restrict__ v = a.table + (size_t)a.sel[c] * (size_t)a.max_samples;
        const double lo = a.lo[c], hi = a.hi[c], s = a.s[c];
        for (long long t0 = 0; t0 < a.n; t0 += (long long)TM_PDF_THREADS * TM_PDF_UNROLL) {
            double x[TM_PDF_UNROLL];
#pragma unroll
            for (int u = 0; u < TM_PDF_UNROLL; u++) {
                const long long t = t0 + (long long)u * TM_PDF_THREADS + tid;
                x[u] = v[t < a.n ? t : a.n - 1];             // (past the end: the last value again, not counted)
            }
#pragma unroll
            for (int u = 0; u < TM_PDF_UNROLL; u++) {
                const long long t = t0 + (long long)u * TM_PDF_THREADS + tid;
                const long long k = tmp_class(x[u], lo, hi, s, nb);
                const int at = k == TM_PDF_BELOW ? nb : (k == TM_PDF_ABOVE ? nb + 1 : (int)k);
                pdf_add(s_cnt, at, t < a.n);
            }
        }
    }
    __syncthreads();
    uint32_t *out = a.out + (size_t)c * (size_t)(nb + 2);
    for (int b = tid; b < nb + 2; b += TM_PDF_THREADS) out[b] = s_cnt[b];
}

__global__ __launch_bounds__(TM_PDF_THREADS) void tamcmc_modepdf_pair_kernel(const TmPdfPairArgs a)
{
    extern __shared__ uint32_t s_cell[];                     // [n_bins * n_bins + 1]: the cells, then outside
    const int p = blockIdx.x, tid = threadIdx.x;
    if (p >= a.n_pairs) return;
    const int nb = a.n_bins, cells = nb * nb;
    for (int b = tid; b < cells + 1; b += TM_PDF_THREADS) s_cell[b] = 0;
    __syncthreads();
    if (a.status[p] == 0) {
        const double *__restrict__ vx = a.table + (size_t)a.pairs[2 * p] * (size_t)a.max_samples;
        const double *__restrict__ vy = a.table + (size_t)a.pairs[2 * p + 1] * (size_t)a.max_samples;
        const double lox = a.lo[2 * p], hix = a.hi[2 * p], sx = a.s[2 * p];
        const double loy = a.lo[2 * p + 1], hiy = a.hi[2 * p + 1], sy = a.s[2 * p + 1];
        for (long long t0 = 0; t0 < a.n; t0 += (long long)TM_PDF_THREADS * TM_PDF_UNROLL) {
            double x[TM_PDF_UNROLL], y[TM_PDF_UNROLL];
#pragma unroll
            for (int u = 0; u < TM_PDF_UNROLL; u++) {
                const long long t = t0 + (long long)u * TM_PDF_THREADS + tid;
                x[u] = vx[t < a.n ? t : a.n - 1];
                y[u] = vy[t < a.n ? t : a.n - 1];
            }
#pragma unroll
            for (int u = 0; u < TM_PDF_UNROLL; u++) {
                const long long t = t0 + (long long)u * TM_PDF_THREADS + tid;
                const long long ka = tmp_class(x[u], lox, hix, sx, nb), kb = tmp_class(y[u], loy, hiy, sy, nb);
                const int at = (ka < 0 || kb < 0) ? cells : (int)ka * nb + (int)kb;
                pdf_add(s_cell, at, t < a.n);
            }
        }
    }
    __syncthreads();
    uint32_t *out = a.out + (size_t)p * (size_t)(cells + 1);
    for (int b = tid; b < cells + 1; b += TM_PDF_THREADS) out[b] = s_cell[b];
}

__global__ __launch_bounds__(TM_PDF_HPD_THREADS) void tamcmc_modepdf_hpd_kernel(const TmPdfHpdArgs a)
{
    __shared__ double s_w[TM_PDF_HPD_THREADS / 64];
    __shared__ long long s_i[TM_PDF_HPD_THREADS / 64];
    const int c = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
    if (c >= a.w || m >= a.n_mass) return;
    const uint64_t *__restrict__ sk = a.keys + (size_t)c * (size_t)a.P;
    const long long k = a.k[m], last = a.n - k;              // i = 0 ... last
    // every thread starts from i = 0, which exists: a thread with no i of its own changes nothing
    double bw = tmp_width(sk, 0, k);
    long long bi = 0;
    for (long long i = tid; i <= last; i += TM_PDF_HPD_THREADS) {
        const double w = tmp_width(sk, i, k);
        if (tmp_before(w, i, bw, bi)) { bw = w; bi = i; }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const double ow = __shfl_down(bw, d);
        const long long oi = __shfl_down(bi, d);
        if (tmp_before(ow, oi, bw, bi)) { bw = ow; bi = oi; }
    }
    if ((tid & 63) == 0) { s_w[tid >> 6] = bw; s_i[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int j = 1; j < TM_PDF_HPD_THREADS / 64; j++)
            if (tmp_before(s_w[j], s_i[j], bw, bi)) { bw = s_w[j]; bi = s_i[j]; }
        const size_t at = (size_t)m * (size_t)a.w + (size_t)c;
        a.start[at] = bi;
        a.lo[at] = tmq_unkey(sk[bi]);
        a.hi[at] = tmq_unkey(sk[bi + k - 1]);
    }
}

int tm_launch_modepdf_hist(const TmPdfHistArgs &a, void *stream)
{
    if (a.n_sel < 1 || a.n_bins < 1 || a.n_bins > TM_PDF_MAX_BINS || a.n < 1 || a.n > a.max_samples) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_modepdf_hist_kernel, dim3((unsigned)a.n_sel), dim3(TM_PDF_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_modepdf_pair(const TmPdfPairArgs &a, void *stream)
{
    if (a.n_pairs < 1 || a.n_bins < 1 || a.n_bins > TM_PDF_MAX_BINS2D || a.n < 1 || a.n > a.max_samples) return (int)hipErrorInvalidValue;
    const size_t lds = ((size_t)a.n_bins * (size_t)a.n_bins + 1) * sizeof(uint32_t);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(tamcmc_modepdf_pair_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(tamcmc_modepdf_pair_kernel, dim3((unsigned)a.n_pairs), dim3(TM_PDF_THREADS), lds, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int tm_launch_modepdf_hpd(const TmPdfHpdArgs &a, void *stream)
{
    if (a.w < 1 || a.n_mass < 1 || a.n_mass > TM_PDF_MAX_MASS || a.n < 1 || a.n > a.P) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_modepdf_hpd_kernel, dim3((unsigned)a.w, (unsigned)a.n_mass), dim3(TM_PDF_HPD_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
