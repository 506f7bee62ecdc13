// tamcmc_loo.h -- PSIS-LOO of a stored chain (tamcmc_summary_loo_* in include/tamcmc_accel.h): leave-one-out
// cross-validation by Pareto-smoothed importance sampling (Vehtari, Gelman & Gabry 2017; Vehtari et al. 2024), per bin,
// with the Pareto shape k-hat as the bin's diagnostic.
//
// The per-bin arithmetic below is plain C++17: the kernels (tamcmc_loo.hip) and the stand-alone check
// (tests/cpp/loo_core_check.cpp, built with g++) call these same functions.  tamcmc_loo.hip includes this header under
// `#pragma clang fp contract(off)`, so on the device none of it is contracted into FMAs.
//
//   x_s = -l_is over the n accepted samples (l = tms_like, tamcmc_summary_walk.h), xmax = max x, z = x - xmax
//   M        = (int64)ceil(fmin(n / 5.0, 3.0 * sqrt((double)n)))                                         tml_tail_M
//   top set  the exact multiset of the M + 1 largest x seen so far: a binary min-heap of M + 1 slots, slot k of bin i at
//            heap[k * stride + i]; its root (the (M+1)-th largest = the cutoff) is also kept in a register by the caller,
//            so a sample with x <= root touches no memory                                                tml_heap_*
//   body     everything that left the set or never entered it, as a running-maximum log-sum-exp (a, r, c):
//            sum exp x = (r - c) exp(a); r = 0 marks "nothing yet".  Two departures from the fold kernel's recurrence,
//            because a body takes tens of thousands of terms and every value the set gives up is a new maximum: r is a
//            Kahan sum with compensation c, and a follows the maximum lazily -- it moves (and r, c are rescaled) only
//            when a value exceeds it by more than TML_LSE_SLACK, so a stays within that of the maximum and r is not
//            multiplied at every replacement (DESIGN.md section 4 has the measurement against the plain recurrence) tml_lse_add
//   finalize the M candidates above the root sorted ascending -> tail {z > c}, c = max(z_root, log DBL_MIN), the
//            generalised Pareto fit of Zhang & Stephens, the smoothed tail, elpd_loo                      tml_finalize
// tml_finalize is written for W lanes that walk the tail with stride W and meet in W::sum (a fixed-order reduction that
// returns the same bits to every lane) and W::sync; the kernel's W is a wave of 64, the host's a single lane.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TML_FN __host__ __device__ inline
#else
#define TML_FN inline
#endif

#define TM_LOO_MAX_TAIL 2048      // TAMCMC_SUMMARY_LOO_MAX_TAIL: M at most, i.e. n_used <= 466 033
#define TM_LOO_MAX_THETA 76       // m = 30 + floor(sqrt(L)) <= 30 + 45
#define TM_LOO_THREADS 64         // tail kernel: one bin per thread; finalize kernel: one wave per bin
#define TM_LOO_UNROLL 8           // row loads in flight per thread

TML_FN int64_t tml_tail_M(int64_t n)
{
    return (int64_t)ceil(fmin((double)n / 5.0, 3.0 * sqrt((double)n)));
}

#define TML_LSE_SLACK 1.0
TML_FN void tml_lse_add(double *a, double *r, double *c, const double x)
{
    double v;
    if (*r == 0.0) { *a = x; v = 1.0; }
    else if (x > *a + TML_LSE_SLACK) {
        const double e = exp(*a - x);
        *r *= e; *c *= e; *a = x;
        v = 1.0;
    } else v = exp(x - *a);
    const double yv = v - *c, t = *r + yv;
    *c = (t - *r) - yv;
    *r = t;
}

// The heap holds cnt values; x becomes value cnt + 1 (the caller has checked cnt < capacity).  *root follows heap[0].
TML_FN void tml_heap_insert(double *heap, const size_t stride, const int cnt, const double x, double *root)
{
    int i = cnt;
    while (i > 0) {
        const int p = (i - 1) >> 1;
        const double hp = heap[(size_t)p * stride];
        if (!(x < hp)) break;
        heap[(size_t)i * stride] = hp;
        i = p;
    }
    heap[(size_t)i * stride] = x;
    if (i == 0) *root = x;
}

// The heap is full (cnt values) and x > *root: the root leaves, x enters.  *root follows heap[0].
TML_FN void tml_heap_replace_root(double *heap, const size_t stride, const int cnt, const double x, double *root)
{
    int i = 0;
    double top = x;
    for (;;) {
        int c = 2 * i + 1;
        if (c >= cnt) break;
        double hc = heap[(size_t)c * stride];
        if (c + 1 < cnt) {
            const double h1 = heap[(size_t)(c + 1) * stride];
            if (h1 < hc) { hc = h1; c++; }
        }
        if (!(hc < x)) break;
        heap[(size_t)i * stride] = hc;
        if (i == 0) top = hc;
        i = c;
    }
    heap[(size_t)i * stride] = x;
    *root = top;
}

// One sample of one bin: n accepted samples came before it, cap = M + 1 slots.
TML_FN void tml_top_push(double *heap, const size_t stride, const int cap, const long long n, const double x, double *root, double *a, double *r, double *c)
{
    if (n < (long long)cap) tml_heap_insert(heap, stride, (int)n, x, root);
    else if (x > *root) {
        tml_lse_add(a, r, c, *root);
        tml_heap_replace_root(heap, stride, cap, x, root);
    } else tml_lse_add(a, r, c, x);
}

struct TmlBin {
    double elpd_loo, pareto_k, cutoff;
    int32_t tail_len;
};

// s[0 .. ncand): the values of the top set above its root, sorted ascending; root: the set's smallest value; has_rule:
// n > M (the root is the (M+1)-th largest x); (body_a, body_r): the body's log-sum-exp, body_r = r - c; t[ncand], theta / ell
// [TM_LOO_MAX_THETA]: work space shared by the lanes.  Every lane returns the same bits.  On return t[0 .. L) holds the
// log weights zt_(j) of the tail, ascending (zt = z where there is no usable fit), each written by the lane that owns j: a
// caller that reads them across lanes calls w.sync() first.
template <class W>
TML_FN TmlBin tml_finalize(W &w, const double *s, const int ncand, const double root, const bool has_rule, const long long n,
                           const double body_a, const double body_r, double *t, double *theta, double *ell)
{
    const int lane = w.lane(), lanes = w.lanes();
    TmlBin out;
    const double xmax = ncand > 0 ? s[ncand - 1] : root;
    const double zroot = root - xmax;
    const double c = has_rule ? fmax(zroot, log(DBL_MIN)) : (double)INFINITY;
    // the tail is the suffix of s with z > c (strictly: ties with the cutoff are body)
    double cb = 0.0, sb = 0.0;
    for (int j = lane; j < ncand; j += lanes) {
        const double z = s[j] - xmax;
        if (!(z > c)) { cb += 1.0; sb += exp(z); }
    }
    const int nb = (int)w.sum(cb);
    const int L = ncand - nb;
    double body = (body_r > 0.0 ? body_r * exp(body_a - xmax) : 0.0) + exp(zroot);
    body += w.sum(sb);
    const double n_body = (double)(n - (long long)L);
    const double *zs = s + nb;            // z_(j) = zs[j - 1] - xmax, j = 1 ... L
    double khat = (double)INFINITY, sigma = 0.0;
    const double ec = exp(c);
    if (L >= 5) {
        const double dL = (double)L;
        for (int j = lane; j < L; j += lanes) t[j] = exp(zs[j] - xmax) - ec;
        w.sync();
        const int m = 30 + (int)floor(sqrt(dL));
        const int q = (int)floor(dL / 4.0 + 0.5);
        const double tq = t[q - 1], tL = t[L - 1];
        for (int j = 1; j <= m; j++) {
            const double th = (1.0 - sqrt((double)m / ((double)j - 0.5))) / (3.0 * tq) + 1.0 / tL;
            double acc = 0.0;
            for (int i = lane; i < L; i += lanes) acc += log1p(-th * t[i]);
            const double kj = w.sum(acc) / dL;
            if (lane == 0) {
                theta[j - 1] = th;
                ell[j - 1] = dL * (log(-th / kj) - kj - 1.0);
            }
        }
        w.sync();
        // w_j = 1 / sum_i exp(l_i - l_j); weights under 10 eps are dropped, the rest renormalised
        double wsum = 0.0, wth = 0.0;
        for (int j = lane; j < m; j += lanes) {
            double den = 0.0;
            for (int i = 0; i < m; i++) den += exp(ell[i] - ell[j]);
            const double wj = 1.0 / den;
            if (!(wj < 10.0 * DBL_EPSILON)) { wsum += wj; wth += wj * theta[j]; }
        }
        wsum = w.sum(wsum);
        wth = w.sum(wth);
        const double that = wth / wsum;
        double acc = 0.0;
        for (int i = lane; i < L; i += lanes) acc += log1p(-that * t[i]);
        const double k = w.sum(acc) / dL;
        sigma = -k / that;
        khat = (dL * k + 5.0) / (dL + 10.0);
    }
    // sum_T exp(zt - z) and sum_T exp(zt), zt the smoothed tail (zt = z where there is no usable fit)
    double s1 = 0.0, s2 = 0.0;
    if (L >= 5 && isfinite(khat)) {
        const double dL = (double)L;
        for (int j = lane; j < L; j += lanes) {
            const double lp = log1p(-((double)(j + 1) - 0.5) / dL);
            const double inner = khat == 0.0 ? -sigma * lp : sigma / khat * expm1(-khat * lp);
            const double zt = fmin(log(inner + ec), 0.0);
            s1 += exp(zt - (zs[j] - xmax));
            s2 += exp(zt);
            t[j] = zt;                    // (the fit is done with t: it leaves as the smoothed tail, for tamcmc_loopit.h)
        }
    } else {
        for (int j = lane; j < L; j += lanes) { s1 += 1.0; s2 += exp(zs[j] - xmax); t[j] = zs[j] - xmax; }
    }
    s1 = w.sum(s1);
    s2 = w.sum(s2);
    out.elpd_loo = log(n_body + s1) - xmax - log(body + s2);
    out.pareto_k = khat;
    out.cutoff = has_rule ? root : (double)NAN;
    out.tail_len = (int32_t)L;
    return out;
}

#if defined(__HIPCC__)
// One wave: the ncand values above the root of a bin's heap column (heap: the bin's slot 0, slots nx doubles apart) into
// s[0 .. P), P the power of two >= ncand, padded with +inf, sorted ascending by a bitonic network.  Ends behind a barrier.
__device__ __forceinline__ void tml_load_sorted(const double *heap, const size_t nx, const int ncand, double *s)
{
    const int lane = (int)threadIdx.x;
    int P = 1;
    while (P < ncand) P <<= 1;
    for (int j = lane; j < P; j += TM_LOO_THREADS) s[j] = j < ncand ? heap[(size_t)(j + 1) * nx] : (double)INFINITY;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < P; i += TM_LOO_THREADS) {
                const int o = i ^ j;
                if (o > i) {
                    const double u = s[i], v = s[o];
                    if ((u > v) == ((i & k) == 0)) { s[i] = v; s[o] = u; }
                }
            }
            __syncthreads();
        }
}

// the finalize kernel's wave (also tamcmc_loopit.hip's prepare kernel)
struct TmlWave {
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int lanes() const { return TM_LOO_THREADS; }
    __device__ double sum(double v) const
    {
#pragma unroll
        for (int o = TM_LOO_THREADS / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, TM_LOO_THREADS);
        return v;
    }
    __device__ void sync() const { __syncthreads(); }
};
#endif

// ---- launch arguments (tamcmc_loo.hip) ----
struct TmLooArgs {
    const double *rows;           // [B][Nx] model rows of the block (stage 1)
    const int32_t *status;        // [B]
    const double *y, *isig2;      // as TmSummaryArgs
    double *heap;                 // [cap][Nx]
    double *body;                 // [3][Nx]: a | r | c
    const long long *cnt_in;      // {accepted, rejected} of this pass before the block / after it (as TmSummaryArgs)
    long long *cnt_out;
    double *elpd, *khat, *cutoff; // [Nx] each, written by the finalize kernel
    int32_t *tail_len;            // [Nx]
    long long n;                  // finalize: the pass's accepted samples
    int32_t Nx, B;
    int32_t likelihood_case, cap; // cap = M + 1
    double like_p;
};

int tm_launch_loo_tail(const TmLooArgs &a, void *stream);             // return a hipError_t
int tm_launch_loo_finalize(const TmLooArgs &a, void *stream);
