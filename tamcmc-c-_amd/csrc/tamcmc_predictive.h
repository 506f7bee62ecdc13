// tamcmc_predictive.h -- posterior predictive check of a stored chain (tamcmc_summary_predictive_* in
// include/tamcmc_accel.h): per bin the predictive CDF and survival function of the datum, averaged over the accepted
// samples, as LOGARITHMS that stay meaningful far below 1e-300 -- a missed mode has y / M of a few thousand.
//
// The per-sample arithmetic below is plain C++17: the kernel (tamcmc_predictive.hip) and the stand-alone check
// (tests/cpp/predictive_core_check.cpp, built with g++) call these same functions.  tamcmc_predictive.hip includes this
// header under `#pragma clang fp contract(off)`, so on the device none of it is contracted into FMAs.
//
//   chi(2,2p)    under a sample's model M the datum is Gamma(shape p, scale M / p), p = like_p, an integer in 1 ... 64.
//                z = p y / M;  P = P(p, z), Q = Q(p, z) = exp(-z) sum_{k<p} z^k / k!, the regularised incomplete gamma
//                functions;  z <= 0 (y <= 0): P = 0, Q = 1.                                        tmp_chi_p1, tmp_chi_p
//   chi_square   the library's l = -(y - M)^2 / sigma^2 (the reference's convention: no factor 1/2) is the logarithm of
//                a Gaussian density with standard deviation sigma / sqrt(2) -- NOT sigma.  The check takes the likelihood
//                at its word: r = (y - M) / sigma, P = erfc(-r) / 2, Q = erfc(r) / 2.  r is formed as (y - M) sqrt(1 /
//                sigma^2) from the context's 1 / sigma^2, the only form of sigma on the device.             tmp_gauss
// Both tails are computed as logarithms and directly, each by adding terms of one sign; log P is never log(1 - Q) where
// Q is the larger of the two, and no intermediate overflows or underflows for any finite z >= 0 or any |r| < 1.3e154
// (beyond that r^2 is not a double, the true log tail is below -DBL_MAX and -inf is its correct rounding):
//   p = 1        log Q = -z;  log P = log1mexp(z) = log(-expm1(-z)) for z <= ln 2, log1p(-exp(-z)) above.  No loop.
//   p > 1        log Q = -z + log S, S = sum_{k<p} z^k / k! by Horner's rule with p - 1 steps: ascending,
//                1 + z/1 (1 + z/2 (... (1 + z/(p-1)))), for z < p - 1;  for z >= p - 1 the largest term is factored out,
//                log S = (p-1) log z - log (p-1)! + log(1 + (p-1)/z (1 + (p-2)/z (... (1 + 1/z)))), whose bracket is at
//                most p: z = 1e300 gives a finite log Q.  Every lane runs the one loop of p - 1 steps and selects its
//                ratio (z / k or k / z) per step: z has mean p under the model, so nearly every wave holds lanes of both
//                kinds and a branch would run both loops.
//                log P = -z + p log z - log p! + log sum_{j>=0} z^j / ((p+1) ... (p+j)) for z <= p, with a number of
//                terms fixed by p alone (tmp_series_terms: the first J whose term at z = p is below 2^-58; 81 at p = 64),
//                so the trip count is the same in every lane;  log P = log1p(-Q) for z > p, where Q < 1/2.  This branch
//                is lane-dependent; its loop costs a divergent wave what it would cost without the branch, and a wave
//                wholly above p nothing.
//                log (p-1)! and log p! come from the host (tmp_log_factorial) in the launch arguments.
//   Gaussian     f(r) = log(erfc(r) / 2):  r < 0: log1p(-erfc(-r) / 2);  0 <= r <= 26: log(erfc(r) / 2) (erfc(26) = 6e-296
//                is still a normal double);  r > 26: -r^2 - log(K sqrt(pi)) - log 2 with eight levels of the continued
//                fraction erfc(r) = exp(-r^2) / (sqrt(pi) K), K = r + (1/2) / (r + 1 / (r + (3/2) / (r + ...))), truncated
//                with a relative error below 8! / (2 r^2)^8 < 1e-20.  log P = f(-r), log Q = f(r).
// Measured against long double (tests/cpp/predictive_core_check.cpp): p = 1 and the Gaussian within a few ulp of
// max(1, |value|); p > 1 within 4 ulp(256) = 2^-42 -- at p = 64, z near p, the three terms -z, (p-1) log z and log (p-1)!
// are 200 ... 260 each and cancel to a value of order 1.
//
// Per bin over the accepted samples, in push order:
//   log_cdf = log((1/n) sum_s P_is),  log_sf = log((1/n) sum_s Q_is): each a running-maximum log-sum-exp (a, r, c), sum =
//            (r - c) exp(a), by the fold kernel's recurrence (tamcmc_summary.hip) with four additions:   tmp_lse_step
//              a term of -inf adds nothing (it is skipped before any difference is formed, so (-inf) - (-inf) never is);
//              r = 0 marks "no finite term yet" -- the state starts as zeros -- and the first finite term sets a = x, r = 1;
//              an empty sum (r = 0 with n > 0: every term was -inf) gives -inf;                           tmp_lse_result
//              r is a Kahan sum with compensation c (rescaled with r when the maximum moves), as the body sum of
//              tamcmc_loo.h is.  Where a bin is explained -- every P_is near 1, log_cdf of order -1e-9 -- the terms
//              exp(x - a) are all near 1 and the plain sum loses ulp(r) / 2 = n 2^-53 at each of its n additions, an
//              absolute error of sqrt(n) 2^-53 ... n 2^-53 in a logarithm whose value is a billionth (4e-16 at n = 37
//              on an MI355X; 7e-17 with the compensation).  For the same reason the host
//              forms log((r - c) / n) as log1p(((r - c) - n) / n) where r - c > n / 2.
//   mean_resid    a Welford mean of y / M (chi(2,2p)) or of r (chi_square).
// State: TM_PRED_NSTATE blocks of Nx doubles.  The number of accepted samples is the fold kernel's (TmSummaryArgs::cnt_in):
// the predictive kernel runs behind the fold kernel of the same block and reads the pair that one read.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TMP_FN __host__ __device__ inline
#else
#define TMP_FN inline
#endif

#define TM_PRED_MAX_P 64          // TAMCMC_SUMMARY_PREDICTIVE_MAX_P
#define TM_PRED_THREADS 256       // one thread owns one bin, as in the fold kernel
#define TM_PRED_UNROLL 8          // row loads in flight per thread

enum {
    TM_PRED_CDF_A = 0, TM_PRED_CDF_R, TM_PRED_CDF_C,     // sum_s P_is = (r - c) exp(a)
    TM_PRED_SF_A, TM_PRED_SF_R, TM_PRED_SF_C,            // sum_s Q_is
    TM_PRED_MEAN_RESID,
    TM_PRED_NSTATE
};

#define TMP_LN2 0.693147180559945309417
#define TMP_LOG_SQRT_PI 0.572364942924700087072      // log(sqrt(pi))
#define TMP_GAUSS_SWITCH 26.0

// log(1 - exp(-z)), z > 0
TMP_FN double tmp_log1mexp(const double z)
{
    return z <= TMP_LN2 ? log(-expm1(-z)) : log1p(-exp(-z));
}

// p = 1: the exponential distribution.  No loop.
TMP_FN void tmp_chi_p1(const double z, double *logP, double *logQ)
{
    if (z <= 0.0) { *logP = -(double)INFINITY; *logQ = 0.0; return; }
    *logQ = -z;
    *logP = tmp_log1mexp(z);
}

// host: log k!
inline double tmp_log_factorial(const int k) { return lgamma((double)k + 1.0); }

// host: the number of terms of the series for P(p, z), z <= p: the first J whose term at z = p, prod_{i<=J} p / (p + i),
// is below 2^-58 (the terms after it sum to less than twice that)
inline int tmp_series_terms(const int p)
{
    double t = 1.0;
    int j = 0;
    while (t >= 0x1p-58) { j++; t *= (double)p / (double)(p + j); }
    return j;
}

// 2 <= p <= TM_PRED_MAX_P; lf_pm1 = log (p-1)!, lf_p = log p!, nterms = tmp_series_terms(p)
TMP_FN void tmp_chi_p(const int p, const double lf_pm1, const double lf_p, const int nterms, const double z, double *logP, double *logQ)
{
    if (z <= 0.0) { *logP = -(double)INFINITY; *logQ = 0.0; return; }
    const double lz = log(z);
    const bool asc = z < (double)(p - 1);
    double s = 1.0;
    for (int i = 1; i < p - 1; i++) {
        // ascending: k = p - 1 ... 2, ratio z / k;   factored: k = 1 ... p - 2, ratio k / z < 1
        const double k = (double)(asc ? p - i : i);
        s = 1.0 + s * (asc ? z / k : k / z);
    }
    // the last step (k = 1 / k = p - 1) stays apart: the bracket is 1 + u, and log1p(u) keeps a small z's digits
    const double u = s * (asc ? z : (double)(p - 1) / z);
    // (where Q is 1 to within the cancellation of -z against log1p(u), the rounding must not lift log Q above 0)
    const double lq = fmin(asc ? -z + log1p(u) : (-z + ((double)(p - 1) * lz - lf_pm1)) + log1p(u), 0.0);
    *logQ = lq;
    if (z <= (double)p) {
        double t = 1.0, sum = 1.0;
        for (int j = 1; j <= nterms; j++) {
            t *= z / (double)(p + j);
            sum += t;
        }
        *logP = (-z + ((double)p * lz - lf_p)) + log(sum);
    } else *logP = log1p(-exp(lq));
}

// log(erfc(r) / 2)
TMP_FN double tmp_log_half_erfc(const double r)
{
    if (r < 0.0) return log1p(-0.5 * erfc(-r));
    if (r <= TMP_GAUSS_SWITCH) return log(0.5 * erfc(r));
    double K = r;
    for (int k = 8; k >= 1; k--) K = r + (0.5 * (double)k) / K;
    return (-(r * r) - (log(K) + TMP_LOG_SQRT_PI)) - TMP_LN2;
}

TMP_FN void tmp_gauss(const double r, double *logP, double *logQ)
{
    *logP = tmp_log_half_erfc(-r);
    *logQ = tmp_log_half_erfc(r);
}

// One more term x = log t of sum t = (r - c) exp(a).
TMP_FN void tmp_lse_step(double *a, double *r, double *c, const double x)
{
    if (x == -(double)INFINITY) return;
    double v;
    if (*r == 0.0) { *a = x; v = 1.0; }
    else if (x > *a) {
        const double e = exp(*a - x);
        *r *= e; *c *= e; *a = x;
        v = 1.0;
    } else v = exp(x - *a);
    const double yv = v - *c, t = *r + yv;
    *c = (t - *r) - yv;
    *r = t;
}

// host: log((1/n) sum)
inline double tmp_lse_result(const double a, const double r, const double c, const long long n)
{
    if (n < 1) return (double)NAN;
    if (r == 0.0) return -(double)INFINITY;
    const double s = r - c, dn = (double)n;
    return a + (s > 0.5 * dn ? log1p((s - dn) / dn) : log(s / dn));
}

// ---- launch arguments (tamcmc_predictive.hip) ----
struct TmPredArgs {
    const double *rows;           // [B][Nx] model rows of the block (stage 1)
    const int32_t *status;        // [B]
    const double *y, *isig2;      // as TmSummaryArgs
    double *state;                // [TM_PRED_NSTATE][Nx]
    const long long *cnt_in;      // {accepted, rejected} before this block: the pair the block's fold launch read
    int32_t Nx, B;
    int32_t likelihood_case, p;   // p = (int)like_p, 1 ... TM_PRED_MAX_P (chi(2,2p) only)
    int32_t nterms, pad;          // tmp_series_terms(p)
    double lf_pm1, lf_p;          // log (p-1)!, log p!
};

int tm_launch_predictive(const TmPredArgs &a, void *stream);          // returns a hipError_t
