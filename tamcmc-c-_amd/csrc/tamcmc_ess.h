// tamcmc_ess.h -- effective sample size, MCSE and split R-hat of a stored chain (tamcmc_summary_ess_* in
// include/tamcmc_accel.h): per bin the autocovariance over the sample order of two series, Geyer's initial monotone
// sequence on it, and the two half-chain moments of the model series.
//
// The arithmetic below is plain C++17: the kernels (tamcmc_ess.hip), the host side (tamcmc_summary_api.cpp) and the
// stand-alone check (tests/cpp/ess_core_check.cpp, built with g++) call these same functions.  tamcmc_ess.hip includes this
// header under `#pragma clang fp contract(off)`; g++ builds it with -ffp-contract=off.  Nothing here is contracted by the
// compiler: the only fused operation is the one written out as fma() in tme_acc.
//
//   series   model        a_t = M_t - mean_M                                                              tme_centre_model
//            likelihood   u_t = exp(l_t - lppd) - 1.0, l = tms_like (tamcmc_summary_walk.h)                tme_centre_like
//            t = 0 ... n - 1 counts ACCEPTED samples in push order; mean_M and lppd are the frozen fold results
//   lags     L = the largest odd number <= min(max_lag | 1, n - 1), max_lag = 0 meaning TM_ESS_DEFAULT_LAG   tme_lag_limit
//   A_k      = sum_{t=k}^{n-1} d_t d_{t-k}, k = 0 ... L.  ACCUMULATION RULE: one accumulator per (bin, k), started at +0.0 and
//            advanced in ascending t by A = fma(d_t, d_{t-k}, A) -- the product is NOT rounded before it is added.  Samples
//            t < k add nothing (no 0 x inf is ever formed).                                               tme_acc
//   storage  acc[k][Nx] and a ring[R][Nx] of the centred values, R = L + TM_ESS_CHUNK slots, d_t in slot t mod R: a pass is
//            cut into chunks of at most TM_ESS_CHUNK pushed samples; a chunk's centred values are written first (behind the
//            L values before them, which are the carry that bridges chunks, blocks and pushes), then every (bin, group of
//            TM_ESS_G consecutive lags) walks the chunk's accepted samples                                tme_lag_group
//   finish   Geyer's initial monotone sequence, in double, in this order                                   tme_finish
//   R-hat    of the two half-chain Welford moments of M                                                   tme_welford, tme_rhat
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TME_FN __host__ __device__ inline
#else
#define TME_FN inline
#endif

#define TM_ESS_MAX_LAG 1023       // TAMCMC_SUMMARY_ESS_MAX_LAG
#define TM_ESS_DEFAULT_LAG 255
#define TM_ESS_G 16               // consecutive lags owned by one thread
#define TM_ESS_CHUNK 64           // pushed samples per pair of launches (centre, lags)
#define TM_ESS_BINS 64            // lag kernel: a workgroup is TM_ESS_BINS bins x TM_ESS_GROUPS lag groups, one wave per group
#define TM_ESS_GROUPS 4
#define TM_ESS_THREADS 256        // centre and finish kernels: one thread per bin

// the four half-chain moments of the model series, [TM_ESS_NHALF][Nx]
enum { TM_ESS_H1_MEAN = 0, TM_ESS_H1_M2, TM_ESS_H2_MEAN, TM_ESS_H2_M2, TM_ESS_NHALF };

TME_FN int tme_lag_limit(const int max_lag, const long long n)
{
    long long m = (max_lag == 0 ? TM_ESS_DEFAULT_LAG : max_lag) | 1;
    if (m > n - 1) m = n - 1;
    if ((m & 1) == 0) m -= 1;
    return (int)m;
}

TME_FN int tme_ring_slots(const int L) { return L + TM_ESS_CHUNK; }

TME_FN double tme_centre_model(const double M, const double mean_M) { return M - mean_M; }
TME_FN double tme_centre_like(const double l, const double lppd) { return exp(l - lppd) - 1.0; }

// the accumulation rule
TME_FN double tme_acc(const double A, const double d_t, const double d_old) { return fma(d_t, d_old, A); }

TME_FN void tme_welford(double *mean, double *M2, const long long count, const double v)
{
    const double d = v - *mean;
    *mean += d / (double)count;
    *M2 += d * (v - *mean);
}

// One bin and one group of lags k0 ... min(k0 + TM_ESS_G - 1, L) over the accepted samples t0 ... t1 - 1, whose centred
// values are in the ring (ring: the bin's slot 0, slots `stride` doubles apart, R slots) together with the L values
// before t0.  acc: the bin's accumulator of lag k0, lags `stride` doubles apart.  0 <= t0 <= t1 <= t0 + TM_ESS_CHUNK.
// Two walks that add the same terms in the same order: TM_ESS_G samples at a time with the window of past values held by
// name (a full group, every lag already within the series), and one sample at a time with the window shifted and every
// term guarded (the first L samples, the last group of a short L, the rest of a chunk).
TME_FN void tme_lag_group(const double *ring, const size_t stride, const int R, const long long t0, const long long t1,
                          const int k0, const int L, double *acc)
{
    constexpr int G = TM_ESS_G;
    const int ng = L + 1 - k0 < G ? L + 1 - k0 : G;
    int st = (int)(t0 % R);                                   // the slot of sample t; every distance back is <= L + 1 < R
    double A[G], w[G];          // w[j] = d_{t - 1 - k0 - j} before sample t (w[G - 1] is never used)
#pragma unroll
    for (int j = 0; j < G; j++) {
        A[j] = j < ng ? acc[(size_t)j * stride] : 0.0;
        const int back = 1 + k0 + j, slot = st - back < 0 ? st - back + R : st - back;
        w[j] = (j < G - 1 && j < ng && t0 >= back) ? ring[(size_t)slot * stride] : 0.0;
    }
    long long t = t0;
    if (t0 >= L && ng == G) {
        int so = st - k0 < 0 ? st - k0 + R : st - k0;
        for (; t + G <= t1; t += G) {
            double dt[G], dn[G];
#pragma unroll
            for (int i = 0; i < G; i++) {
                const int a = st + i >= R ? st + i - R : st + i, b = so + i >= R ? so + i - R : so + i;
                dt[i] = ring[(size_t)a * stride];
                dn[i] = ring[(size_t)b * stride];
            }
#pragma unroll
            for (int i = 0; i < G; i++)
#pragma unroll
                for (int j = 0; j < G; j++)
                    A[j] = tme_acc(A[j], dt[i], i >= j ? dn[i - j] : w[j - i - 1]);
#pragma unroll
            for (int j = 0; j < G; j++) w[j] = dn[G - 1 - j];
            st = st + G >= R ? st + G - R : st + G;
            so = so + G >= R ? so + G - R : so + G;
        }
    }
    for (; t < t1; t++) {
        const int so = st - k0 < 0 ? st - k0 + R : st - k0;
        const double dt = ring[(size_t)st * stride];
        const double dn = t >= k0 ? ring[(size_t)so * stride] : 0.0;
#pragma unroll
        for (int j = G - 1; j > 0; j--) w[j] = w[j - 1];
        w[0] = dn;
#pragma unroll
        for (int j = 0; j < G; j++)
            if (j < ng && t >= k0 + j) A[j] = tme_acc(A[j], dt, w[j]);
        st = st + 1 == R ? 0 : st + 1;
    }
#pragma unroll
    for (int j = 0; j < G; j++)
        if (j < ng) acc[(size_t)j * stride] = A[j];
}

// Geyer's initial monotone sequence on A_0 ... A_L (A: the bin's A_0, lags `stride` doubles apart; L odd).  dn = (double)n,
// tau_floor = 1 / log10(n) as the host evaluates it.
//   rho_k = A_k / A_0;  P_m = rho_{2m} + rho_{2m+1}, m = 0 ... (L-1)/2;  K = the first m for which P_m >= 0 does not hold (a
//   NaN stops the sum too), or (L+1)/2;  P_m = min(P_m, P_{m-1});  tau = -1 + 2 sum_{m<K} P_m in ascending m;
//   tau = max(tau, tau_floor);  ess = n / tau;  cut = 2K (cut = L + 1: truncated).  A_0 zero or not finite: NaN, NaN, 0.
struct TmeFinish {
    double tau, ess;
    int32_t cut;
};

TME_FN TmeFinish tme_finish(const double *A, const size_t stride, const int L, const double dn, const double tau_floor)
{
    TmeFinish f;
    const double A0 = A[0];
    if (A0 == 0.0 || !(fabs(A0) <= 1.79769313486231570815e308)) {
        f.tau = f.ess = (double)NAN; f.cut = 0;
        return f;
    }
    const int M = (L + 1) / 2;
    int K = M;
    double sum = 0.0, prev = 0.0;
    for (int m = 0; m < M; m++) {
        const double r0 = A[(size_t)(2 * m) * stride] / A0, r1 = A[(size_t)(2 * m + 1) * stride] / A0;
        double P = r0 + r1;
        if (!(P >= 0.0)) { K = m; break; }
        if (m > 0 && prev < P) P = prev;
        sum += P;
        prev = P;
    }
    double tau = -1.0 + 2.0 * sum;
    if (tau < tau_floor) tau = tau_floor;
    f.tau = tau;
    f.ess = dn / tau;
    f.cut = 2 * K;
    return f;
}

// Split R-hat from the Welford moments of the two halves of h samples each (h >= 2):
//   W = (s1^2 + s2^2) / 2, s^2 = M2 / (h - 1);  Bn = (m1 - mb)^2 + (m2 - mb)^2, mb = (m1 + m2) / 2;
//   rhat = sqrt(((h - 1) / h * W + Bn) / W);  W = 0: NaN.
TME_FN double tme_rhat(const double m1, const double M2_1, const double m2, const double M2_2, const long long h)
{
    const double dh = (double)h;
    const double s1 = M2_1 / (dh - 1.0), s2 = M2_2 / (dh - 1.0);
    const double W = (s1 + s2) / 2.0;
    if (W == 0.0) return (double)NAN;
    const double mb = (m1 + m2) / 2.0;
    const double Bn = (m1 - mb) * (m1 - mb) + (m2 - mb) * (m2 - mb);
    return sqrt(((dh - 1.0) / dh * W + Bn) / W);
}

#if defined(TME_HOST_FEED)
// One bin of one series on the host, fed in pieces: the chunking, the ring and the lag groups of the device path
// (tests/cpp/ess_core_check.cpp).
#include <vector>
struct TmeHostSeries {
    int L, R;
    long long t = 0;
    std::vector<double> ring, acc;
    explicit TmeHostSeries(const int L_) : L(L_), R(tme_ring_slots(L_)), ring((size_t)R, 0.0), acc((size_t)L_ + 1, 0.0) {}
    void push(const double *d, long long m)
    {
        while (m > 0) {
            const long long c = m < TM_ESS_CHUNK ? m : TM_ESS_CHUNK;
            for (long long i = 0; i < c; i++) ring[(size_t)((t + i) % R)] = d[i];
            for (int k0 = 0; k0 <= L; k0 += TM_ESS_G) tme_lag_group(ring.data(), 1, R, t, t + c, k0, L, acc.data() + k0);
            t += c; d += c; m -= c;
        }
    }
};
#endif

struct TmEssArgs {
    const double *rows;           // [B][Nx] model rows of the chunk
    const int32_t *status;        // [B] of the chunk's samples, device memory
    const double *y, *isig2;      // the context's spectrum; 1 / sigma^2 (chi_square only, else NULL)
    const double *mean_M, *lppd;  // [Nx] each: the frozen fold results
    double *ring;                 // [2][R][Nx]: model series, likelihood series
    double *acc;                  // [2][L + 1][Nx]
    double *half;                 // [TM_ESS_NHALF][Nx]
    double *tau, *ess;            // [2][Nx] each (finish)
    int32_t *cut;                 // [2][Nx]
    const long long *cnt_in;      // {accepted, rejected} before the chunk / after it, as TmSummaryArgs
    long long *cnt_out;
    long long n, h;               // the fold pass's accepted samples; floor(n / 2)
    int32_t Nx, B;                // B <= TM_ESS_CHUNK samples in this chunk
    int32_t L, R;
    int32_t likelihood_case, pad;
    double like_p;
    double tau_floor;             // 1 / log10(n), formed on the host
};

// tamcmc_ess.hip; each returns a hipError_t
int tm_launch_ess_chunk(const TmEssArgs &a, void *stream);        // centre kernel, then lag kernel
int tm_launch_ess_finish(const TmEssArgs &a, void *stream);
