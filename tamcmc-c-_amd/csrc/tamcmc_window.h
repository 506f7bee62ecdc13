// tamcmc_window.h -- windowed posterior predictive check of a stored chain (tamcmc_summary_window_* in
// include/tamcmc_accel.h): the predictive check of tamcmc_predictive.h over disjoint groups of bins.  A mode of modest
// height has y / M of 2 ... 4 in each of its tens of bins: per bin that is log_sf of -2 ... -4 and lost in the model's own
// noise; the sum over 20 such bins has log_sf of -8.6 ... -35.8.
//
// The per-(sample, window) arithmetic below is plain C++17: the kernels (tamcmc_window.hip) and the stand-alone check
// (tests/cpp/window_core_check.cpp, built with g++) call these same functions.  tamcmc_window.hip includes this header
// under `#pragma clang fp contract(off)`, so on the device none of it is contracted into FMAs.
//
//   windows      W bins each, the first one `first` bins (1 ... W): window 0 is [0, min(first, Nx)), window w >= 1 is
//                [first + (w-1) W, min(first + w W, Nx)); n_windows = 1 + ceil(max(Nx - first, 0) / W).     tmw_partition
//                At most three distinct lengths: the first window, the full windows, the last window.
//   sums         S_sw = sum_{i in w} y_i / M_is (chi(2,2p)) or R_sw = sum_{i in w} (y_i - M_is) sqrt(isig2_i) (chi_square):
//                one division (one product) per bin, added in ascending bin order starting from the first term. tmw_sum
//   chi(2,2p)    the sum of len independent Gamma(p, M / p) data scaled by p / M is Gamma(p len, 1): z = (double)p S,
//                shape a = p len <= TM_WIN_MAX_SHAPE.  a = 1: tmp_chi_p1.  One bin per window: tmp_chi_p of
//                tamcmc_predictive.h at shape p, so that W = 1 is the per-bin check bit for bit.  Otherwise tmw_chi_a:
//                tmp_chi_p's two loops with the largest term written about its maximum (see there).  The cap on the
//                shape is the ascending Horner sum's: it reaches e^z with z < a - 1, which leaves the doubles past a
//                of about 700.  tmp_series_terms(512) = 216.                                               tmw_chi
//   chi_square   each r has standard deviation 1 / sqrt(2) (the likelihood taken at its word, as per bin), and so has
//                g = R c, c = 1 / sqrt((double)len) formed on the host: log P, log Q by tmp_gauss(g).       tmw_gauss
//   W = 1 is the per-bin check bit for bit: c = 1.0, a sum of one term is that term, S / 1 = S, and p (y / M) = (p y) / M
//   where p is a power of two.
// Measured against long double (tests/cpp/window_core_check.cpp: a log-domain sum of all a terms for Q, the series or
// 1 - Q for P; z at 1e-300, 1e-3, a/2, both sides of a - 1, a, a + 1, 2a, 4a, 1e4, 1e300 and 300 draws from Gamma(a)),
// worst error relative to max(1, |value|), and the check's bar (the power of two at or above twice the worst):
//   shape 1: 1.4e-16 (2^-51)    2: 6.6e-16 (2^-49)    3: 7.4e-16 (2^-49)    25: 2.3e-15 (2^-47)    64: 4.6e-15 (2^-46)
//   256: 1.7e-14 (2^-44)        511: 3.0e-14 (2^-43)  512: 3.2e-14 (2^-43)  Gaussian, len 1, 2, 7, 512: 2.9e-16 (2^-50)
// (tmw_chi_a; with tmp_chi_p itself shape 25 had 1.8e-14 and shape 512 6.0e-13).  What is left at shape 512 is the
// ascending branch's -z + log1p(u), two numbers of up to 511 whose difference is of order 1.
//
// Per window over the accepted samples, in push order: log_cdf and log_sf by tmp_lse_step / tmp_lse_result, mean_resid a
// Welford mean of S / len (R / len).  State: TM_PRED_NSTATE blocks of n_windows doubles, laid out as the per-bin state.
#pragma once
#include "tamcmc_predictive.h"

#define TM_WIN_MAX_BINS 512       // TAMCMC_SUMMARY_WINDOW_MAX_BINS
#define TM_WIN_MAX_SHAPE 512      // TAMCMC_SUMMARY_WINDOW_MAX_SHAPE
#define TM_WIN_THREADS 256
#define TM_WIN_TILE_BINS 4096     // bins of one sample a workgroup of the sums kernel stages through LDS, at most
// a window's slot in LDS is W | 1 doubles: an odd stride keeps the 32 lanes of a half-wave, each reading its own
// window, on 32 different bank pairs
#define TM_WIN_LDS_DOUBLES (TM_WIN_TILE_BINS + TM_WIN_THREADS)

// the three window lengths of a partition: index 0 the first window, 1 the full windows, 2 the last window
struct TmWinShape {
    int32_t len;                  // bins
    int32_t a;                    // chi(2,2p): the shape p len
    int32_t nterms, pad;          // tmp_series_terms(a)
    double lf_am1, lf_a;          // log (a-1)!, log a!
    double cq, cp;                // m log m - m - log m! at m = a - 1 and at m = a (tmw_chi_a), formed in long double
    double c;                     // 1 / sqrt((double)len)
};

// host: first = 0 means W.  Returns n_windows and the three lengths.
inline long long tmw_partition(const long long Nx, const int W, int *first, int len[3])
{
    if (*first == 0) *first = W;
    const long long f = *first, rest = Nx > f ? Nx - f : 0;
    const long long nw = 1 + (rest + W - 1) / W;
    len[0] = (int)(Nx < f ? Nx : f);
    len[1] = W;
    len[2] = nw >= 2 ? (int)(Nx - (f + (nw - 2) * W)) : len[0];
    return nw;
}

inline TmWinShape tmw_shape(const int len, const int p)
{
    TmWinShape s{};
    s.len = len;
    s.a = p * len;
    s.nterms = tmp_series_terms(s.a);
    s.lf_am1 = tmp_log_factorial(s.a - 1);
    s.lf_a = tmp_log_factorial(s.a);
    const long double m = (long double)(s.a - 1), n = (long double)s.a;
    s.cq = s.a >= 2 ? (double)(m * logl(m) - m - lgammal(m + 1.0L)) : 0.0;
    s.cp = (double)(n * logl(n) - n - lgammal(n + 1.0L));
    s.c = 1.0 / sqrt((double)len);
    return s;
}

// the first bin of window w and the bin after its last
TMP_FN long long tmw_begin(const long long w, const int W, const int first) { return w == 0 ? 0 : (long long)first + (w - 1) * W; }
TMP_FN long long tmw_end(const long long w, const int W, const int first, const long long Nx)
{
    const long long e = (long long)first + w * W;
    return e < Nx ? e : Nx;
}

// 0: the first window, 2: the last of two or more, 1: the others
TMP_FN int tmw_kind(const long long w, const long long n_windows) { return w == 0 ? 0 : (w == n_windows - 1 ? 2 : 1); }

// the window sum: len >= 1 terms at q, ascending
TMP_FN double tmw_sum(const double *q, const int len)
{
    double s = q[0];
    for (int i = 1; i < len; i++) s += q[i];
    return s;
}

// Shape a >= 2 of a window of two or more bins: tmp_chi_p with its largest terms written about their maximum.  tmp_chi_p
// forms m log z - log m! - z (m = a - 1 for Q, a for P): the error of log z, times m, in every sample.  A device's log is
// a 1-ulp function whose error has a mean over a range of z -- measured on an MI355X at a = 21, z in 14 ... 21: log P low by
// 3.6e-15 on average -- so that term does not average out over a chain.  Here the same quantity is
//     m log1p(x) - d + (m log m - m - log m!),   d = z - m,  x = d / m,
// whose logarithm is of a number near 1 where the probability lives (|x| of order 1 / sqrt(m): the error is that much
// smaller) and whose constant, about -log(2 pi m) / 2, comes from the host in long double.  Below a / 2 the series for P
// keeps tmp_chi_p's form (z - a would lose z's digits; |log P| is at least 0.19 a there and the error relative to it).
// The loops are tmp_chi_p's: one select per step, trip counts fixed by a.
TMP_FN void tmw_chi_a(const TmWinShape &sh, const double z, double *logP, double *logQ)
{
    if (z <= 0.0) { *logP = -(double)INFINITY; *logQ = 0.0; return; }
    const int a = sh.a;
    const double m = (double)(a - 1), da = (double)a;
    const bool asc = z < m;
    double s = 1.0;
    for (int i = 1; i < a - 1; i++) {
        const double k = (double)(asc ? a - i : i);
        s = 1.0 + s * (asc ? z / k : k / z);
    }
    const double u = s * (asc ? z : m / z);
    const double dq = z - m;
    const double lq = fmin(asc ? -z + log1p(u) : ((m * log1p(dq / m) - dq) + sh.cq) + log1p(u), 0.0);
    *logQ = lq;
    if (z <= da) {
        double t = 1.0, sum = 1.0;
        for (int j = 1; j <= sh.nterms; j++) {
            t *= z / (double)(a + j);
            sum += t;
        }
        const double dp = z - da;
        const double head = z < 0.5 * da ? -z + (da * log(z) - sh.lf_a) : (da * log1p(dp / da) - dp) + sh.cp;
        *logP = head + log(sum);
    } else *logP = log1p(-exp(lq));
}

// a = 1: the exponential; one bin per window: the per-bin check's own call, bit for bit; otherwise tmw_chi_a
TMP_FN void tmw_chi(const TmWinShape &sh, const int p, const double S, double *logP, double *logQ)
{
    const double z = (double)p * S;
    if (sh.a == 1) tmp_chi_p1(z, logP, logQ);
    else if (sh.len == 1) tmp_chi_p(sh.a, sh.lf_am1, sh.lf_a, sh.nterms, z, logP, logQ);
    else tmw_chi_a(sh, z, logP, logQ);
}

TMP_FN void tmw_gauss(const TmWinShape &sh, const double R, double *logP, double *logQ)
{
    tmp_gauss(R * sh.c, logP, logQ);
}

// ---- launch arguments (tamcmc_window.hip) ----
struct TmWinArgs {
    const double *rows;           // [B][Nx] model rows of the block (stage 1)
    const int32_t *status;        // [B]
    const double *y, *isig2;      // as TmSummaryArgs
    double *state;                // [TM_PRED_NSTATE][n_windows]
    double *scratch;              // [3][Bcap][n_windows]: log P, log Q, the sum, of every (sample, window) of the block
    const long long *cnt_in;      // {accepted, rejected} before this block: the pair the block's fold launch read
    int32_t Nx, B;
    int32_t Bcap;                 // block_chains: the scratch's stride
    int32_t n_windows;
    int32_t W, first;
    int32_t likelihood_case, p;
    TmWinShape shape[3];
};

// sums kernel, tails kernel, fold kernel, in that order on `stream`; returns a hipError_t
int tm_launch_window(const TmWinArgs &a, void *stream);
