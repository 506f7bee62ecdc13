// tamcmc_modediag.h -- diagnostics of the posterior mode table's columns (tamcmc_modediag_* in include/tamcmc_accel.h):
// effective sample size, Monte-Carlo standard error and split R-hat of every column, and the covariances and correlations
// between columns, all from the accepted rows the table keeps on the device, column-major (table[col * max_samples + t]).
//
// Everything below is plain C++17: the kernels (tamcmc_modediag.hip), the host side (tamcmc_modediag_api.cpp) and the
// stand-alone check (tests/cpp/modediag_core_check.cpp, built with g++) call these same functions.  The kernels' file
// includes this header and tamcmc_ess.h under `#pragma clang fp contract(off)`; g++ builds them with -ffp-contract=off.  The
// only fused operation is the one written out as fma() (tme_acc of tamcmc_ess.h, tmd_cov_acc here).
//
//   n        accepted rows in the table; v_t = column c of the t-th accepted row, t = 0 ... n - 1
//   d_t      = v_t - mean_c, mean_c the table's own Welford mean (what tamcmc_modetable_result returns)       tmd_centre
//   A_k      = sum_{t=k}^{n-1} d_t d_{t-k}, k = 0 ... L, L = tme_lag_limit(max_lag, n): one accumulator per (column, k), from +0.0,
//            in ascending t by tme_acc; terms with t < k are not formed                                     tmd_lag_serial
//   S_ij     = sum_t d_{i,t} d_{j,t}, from +0.0 in ascending t by fma(d_i, d_j, S)                          tmd_cov_serial
//            (fma(a, b, S) = fma(b, a, S), so S_ij = S_ji and S_ii = A_0 of column i, bit for bit)
//   finish   tme_finish and tme_rhat of tamcmc_ess.h, the halves [0, h) and [n - h, n), h = floor(n / 2), by tme_welford on d_t
//            (R-hat is unchanged by the shift; the recurrence then rounds at the size of the spread, not of the value)
//   r_ij     = cov_ij / (sqrt(cov_ii) sqrt(cov_jj)), clamped to [-1, 1]                                     tmd_corr
//
// Lag kernel's walk.  A workgroup is one wave: one column, TM_MD_BLOCK_LAGS = 256 consecutive lags, lane i owning the
// TM_MD_G = 4 lags k0 = kb + 4 i ... k0 + 3 with their accumulators in registers.  The column's centred values pass through
// LDS in tiles of TM_MD_TILE samples behind a halo of the TM_MD_HALO values before them: buf[TM_MD_HALO + i] = d_{t0 + i},
// buf[TM_MD_HALO - b] = d_{t0 - b}.  Before the next tile the last TM_MD_HALO values move to the front (tmd_halo_src).  Within
// a tile a lane walks the samples in ascending t (tmd_lag_tile): four at a time with the window of past values held by name
// once every lag of the lane lies within the series, one at a time with every term guarded before that.  Either way an
// accumulator takes its terms in ascending t, so the result is that of tmd_lag_serial bit for bit.
//
// Covariance kernel's walk.  The selected columns are cut into strips of TM_MD_CT = 32; a workgroup of 256 threads owns one
// pair of strips (bi <= bj) of the upper triangle (tmd_tile_pair), thread (ty, tx) the 2 x 2 pairs of columns 2 ty, 2 ty + 1
// of strip bi with 2 tx, 2 tx + 1 of strip bj.  The two strips pass through LDS in stages of TM_MD_CS samples, t-major with
// a row of TM_MD_CROW doubles; every pair takes its terms in ascending t.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "tamcmc_ess.h"

#define TMD_FN TME_FN

#define TM_MD_MAX_LAG 1023        // TAMCMC_MODEDIAG_MAX_LAG
#define TM_MD_MAX_COLS 1024       // TAMCMC_MODEDIAG_MAX_COLS
#define TM_MD_G 4                 // consecutive lags owned by one lane
#define TM_MD_LANES 64            // lag kernel: one wave per workgroup
#define TM_MD_BLOCK_LAGS (TM_MD_G * TM_MD_LANES)
#define TM_MD_TILE 1024           // samples per LDS tile, a multiple of TM_MD_G and of TM_MD_LANES, >= TM_MD_HALO
#define TM_MD_HALO 1024           // values kept before a tile, > TM_MD_MAX_LAG and a multiple of TM_MD_G
#define TM_MD_FIN_THREADS 64      // finish kernel: one thread per column
#define TM_MD_FIN_UNROLL 8        // loads in flight per half
#define TM_MD_CT 32               // covariance kernel: columns per strip
#define TM_MD_CS 64               // ... samples per stage
#define TM_MD_CROW (TM_MD_CT + 2) // ... doubles per LDS row (16-byte aligned pairs; rows land in different banks)
#define TM_MD_CTHREADS 256

enum { TM_MD_TAU = 0, TM_MD_ESS, TM_MD_RHAT, TM_MD_NFIN };   // the finish kernel's arrays, [TM_MD_NFIN][n_cols] behind the lag products

TMD_FN double tmd_centre(const double v, const double mean) { return v - mean; }
TMD_FN double tmd_cov_acc(const double S, const double a, const double b) { return fma(a, b, S); }

// lag blocks of a call; samples of the tile that starts at t0; where slot j of the halo comes from when a tile is left
TMD_FN int tmd_lag_blocks(const int L) { return (L + TM_MD_BLOCK_LAGS) / TM_MD_BLOCK_LAGS; }
TMD_FN int tmd_tile_len(const long long n, const long long t0) { return n - t0 < TM_MD_TILE ? (int)(n - t0) : TM_MD_TILE; }
TMD_FN int tmd_halo_src(const int j) { return TM_MD_TILE + j; }

// One lane's walk over one tile.  cur points at d_{t0}: cur[i] = d_{t0 + i} for 0 <= i < m, cur[-b] = d_{t0 - b} for
// 1 <= b <= min(t0, TM_MD_HALO) (whatever lies before sample 0 is never used in a product).  Lags k0 ... k0 + ng - 1,
// 1 <= ng <= G, k0 + ng - 1 <= TM_MD_MAX_LAG, k0 a multiple of G; A[j] is the accumulator of lag k0 + j.
template <int G>
TMD_FN void tmd_lag_tile(const double *cur, const long long t0, const int m, const int k0, const int ng, double *A)
{
    double w[G];                  // w[j] = d_{t - 1 - k0 - j} before sample t
#pragma unroll
    for (int j = 0; j < G; j++) w[j] = (j < ng && t0 >= 1 + k0 + j) ? cur[-(1 + k0 + j)] : 0.0;
    int i = 0;
    if (ng == G && t0 >= k0 + G - 1) {
        for (; i + G <= m; i += G) {
            double dt[G], dn[G];
#pragma unroll
            for (int u = 0; u < G; u++) { dt[u] = cur[i + u]; dn[u] = cur[i + u - k0]; }
#pragma unroll
            for (int u = 0; u < G; u++)
#pragma unroll
                for (int j = 0; j < G; j++) A[j] = tme_acc(A[j], dt[u], u >= j ? dn[u - j] : w[j - u - 1]);
#pragma unroll
            for (int j = 0; j < G; j++) w[j] = dn[G - 1 - j];
        }
    }
    for (; i < m; i++) {
        const long long t = t0 + i;
        const double dt = cur[i], dn = t >= k0 ? cur[i - k0] : 0.0;
#pragma unroll
        for (int j = G - 1; j > 0; j--) w[j] = w[j - 1];
        w[0] = dn;
#pragma unroll
        for (int j = 0; j < G; j++)
            if (j < ng && t >= k0 + j) A[j] = tme_acc(A[j], dt, w[j]);
    }
}

// The plain statements.  v: the column, n values `1` apart; A: L + 1 sums, `stride` doubles apart.
inline void tmd_lag_serial(const double *v, const long long n, const double mean, const int L, double *A, const size_t stride)
{
    for (int k = 0; k <= L; k++) {
        double s = 0.0;
        for (long long t = k; t < n; t++) s = tme_acc(s, tmd_centre(v[t], mean), tmd_centre(v[t - k], mean));
        A[(size_t)k * stride] = s;
    }
}
inline double tmd_cov_serial(const double *vi, const double mean_i, const double *vj, const double mean_j, const long long n)
{
    double s = 0.0;
    for (long long t = 0; t < n; t++) s = tmd_cov_acc(s, tmd_centre(vi[t], mean_i), tmd_centre(vj[t], mean_j));
    return s;
}

// Strip pairs of the upper triangle, row by row: block b of nt (nt + 1) / 2 -> (bi, bj), bi <= bj < nt.
TMD_FN int tmd_cov_strips(const int n_sel) { return (n_sel + TM_MD_CT - 1) / TM_MD_CT; }
TMD_FN int tmd_cov_blocks(const int n_sel) { const int nt = tmd_cov_strips(n_sel); return nt * (nt + 1) / 2; }
TMD_FN void tmd_tile_pair(int b, const int nt, int *bi, int *bj)
{
    int i = 0;
    while (b >= nt - i) { b -= nt - i; i++; }
    *bi = i; *bj = i + b;
}
// whether the thread's pair (column i of the selection, column j) is this workgroup's to store, as (i, j) and (j, i)
TMD_FN bool tmd_cov_owns(const int i, const int j, const int n_sel) { return i < n_sel && j < n_sel && i <= j; }

// The correlation from the covariances.  NaN where either variance is 0 or not finite (or a NaN); the diagonal is 1.0.
TMD_FN double tmd_corr(const double cov_ij, const double cov_ii, const double cov_jj, const bool diagonal)
{
    const bool ok_i = cov_ii > 0.0 && cov_ii <= 1.79769313486231570815e308, ok_j = cov_jj > 0.0 && cov_jj <= 1.79769313486231570815e308;
    if (!ok_i || !ok_j) return (double)NAN;
    if (diagonal) return 1.0;
    const double r = cov_ij / (sqrt(cov_ii) * sqrt(cov_jj));
    return r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
}

// The totals, in column order: the first column wins a tie, a NaN is skipped.
struct TmdTotals {                // tamcmc_modediag_totals
    int64_t n_used, lag;
    double min_ess, max_rhat;
    int64_t col_min_ess, col_max_rhat, n_truncated, n_constant, n_rhat_high;
};
inline TmdTotals tmd_totals(const int n_cols, const long long n, const int L, const double *ess, const double *rhat, const int32_t *cut,
                            const double *A0)
{
    TmdTotals t{};
    t.n_used = n; t.lag = L;
    t.min_ess = t.max_rhat = (double)NAN;
    t.col_min_ess = t.col_max_rhat = -1;
    for (int c = 0; c < n_cols; c++) {
        if (t.col_min_ess < 0 ? !(ess[c] != ess[c]) : ess[c] < t.min_ess) { t.min_ess = ess[c]; t.col_min_ess = c; }
        if (t.col_max_rhat < 0 ? !(rhat[c] != rhat[c]) : rhat[c] > t.max_rhat) { t.max_rhat = rhat[c]; t.col_max_rhat = c; }
        if (cut[c] == L + 1) t.n_truncated++;
        if (A0[c] == 0.0) t.n_constant++;
        if (rhat[c] > 1.01) t.n_rhat_high++;
    }
    return t;
}

// device bytes the diagnostics add to a mode table (the header comment of tamcmc_modediag_ess states them)
inline size_t tmd_acc_bytes(const int L, const int n_cols) { return ((size_t)(L + 1) + TM_MD_NFIN) * (size_t)n_cols * sizeof(double) + (size_t)n_cols * sizeof(int32_t); }
inline size_t tmd_cov_bytes(const int n_sel) { return (size_t)n_sel * (size_t)n_sel * sizeof(double) + (size_t)n_sel * sizeof(int32_t); }

#if defined(TMD_HOST_FEED)
// The kernels' walks on the host, tile by tile and lane by lane (tests/cpp/modediag_core_check.cpp).
#include <vector>
// the lag kernel: column v (n values), every lag block and lane; A[k], k = 0 ... L
inline void tmd_host_lag_column(const double *v, const long long n, const double mean, const int L, double *A)
{
    std::vector<double> buf((size_t)TM_MD_HALO + TM_MD_TILE, 0.0);
    for (int blk = 0; blk < tmd_lag_blocks(L); blk++) {
        double acc[TM_MD_LANES][TM_MD_G] = {};
        for (int j = 0; j < TM_MD_HALO; j++) buf[(size_t)j] = 0.0;
        for (long long t0 = 0; t0 < n; t0 += TM_MD_TILE) {
            const int m = tmd_tile_len(n, t0);
            if (t0 > 0)
                for (int j = 0; j < TM_MD_HALO; j++) buf[(size_t)j] = buf[(size_t)tmd_halo_src(j)];
            for (int i = 0; i < m; i++) buf[(size_t)TM_MD_HALO + i] = tmd_centre(v[t0 + i], mean);
            for (int lane = 0; lane < TM_MD_LANES; lane++) {
                const int k0 = blk * TM_MD_BLOCK_LAGS + lane * TM_MD_G, ng = L + 1 - k0 < TM_MD_G ? L + 1 - k0 : TM_MD_G;
                if (ng > 0) tmd_lag_tile<TM_MD_G>(buf.data() + TM_MD_HALO, t0, m, k0, ng, acc[lane]);
            }
        }
        for (int lane = 0; lane < TM_MD_LANES; lane++)
            for (int j = 0; j < TM_MD_G; j++) {
                const int k = blk * TM_MD_BLOCK_LAGS + lane * TM_MD_G + j;
                if (k <= L) A[k] = acc[lane][j];
            }
    }
}
// the covariance kernel: table[col * stride + t], the selection sel[n_sel], means by column; S[n_sel][n_sel]
inline void tmd_host_cov(const double *table, const size_t stride, const long long n, const double *mean, const int32_t *sel, const int n_sel,
                         double *S)
{
    const int nt = tmd_cov_strips(n_sel);
    std::vector<double> sa((size_t)TM_MD_CS * TM_MD_CROW), sb((size_t)TM_MD_CS * TM_MD_CROW);
    for (int b = 0; b < tmd_cov_blocks(n_sel); b++) {
        int bi, bj;
        tmd_tile_pair(b, nt, &bi, &bj);
        std::vector<double> acc((size_t)TM_MD_CT * TM_MD_CT, 0.0);
        for (long long t0 = 0; t0 < n; t0 += TM_MD_CS) {
            const int m = n - t0 < TM_MD_CS ? (int)(n - t0) : TM_MD_CS;
            for (int s = 0; s < m; s++)
                for (int c = 0; c < TM_MD_CT; c++) {
                    const int i = bi * TM_MD_CT + c, j = bj * TM_MD_CT + c;
                    sa[(size_t)s * TM_MD_CROW + c] = i < n_sel ? tmd_centre(table[(size_t)sel[i] * stride + (size_t)(t0 + s)], mean[sel[i]]) : 0.0;
                    sb[(size_t)s * TM_MD_CROW + c] = j < n_sel ? tmd_centre(table[(size_t)sel[j] * stride + (size_t)(t0 + s)], mean[sel[j]]) : 0.0;
                }
            for (int ci = 0; ci < TM_MD_CT; ci++)
                for (int cj = 0; cj < TM_MD_CT; cj++)
                    for (int s = 0; s < m; s++)
                        acc[(size_t)ci * TM_MD_CT + cj] = tmd_cov_acc(acc[(size_t)ci * TM_MD_CT + cj], sa[(size_t)s * TM_MD_CROW + ci], sb[(size_t)s * TM_MD_CROW + cj]);
        }
        for (int ci = 0; ci < TM_MD_CT; ci++)
            for (int cj = 0; cj < TM_MD_CT; cj++) {
                const int i = bi * TM_MD_CT + ci, j = bj * TM_MD_CT + cj;
                if (!tmd_cov_owns(i, j, n_sel)) continue;
                S[(size_t)i * n_sel + j] = acc[(size_t)ci * TM_MD_CT + cj];
                S[(size_t)j * n_sel + i] = acc[(size_t)ci * TM_MD_CT + cj];
            }
    }
}
#endif

// ---- launch arguments (tamcmc_modediag.hip) ----
struct TmMdArgs {
    const double *table;          // [n_cols][max_samples]
    const double *mean;           // [n_cols]: the table's Welford means (its state)
    double *acc;                  // [L + 1][n_cols]
    double *fin;                  // [TM_MD_NFIN][n_cols]
    int32_t *cut;                 // [n_cols]
    long long n, max_samples;     // accepted rows, 4 <= n <= max_samples
    int32_t n_cols, L;            // L odd, 1 <= L <= min(TM_MD_MAX_LAG, n - 1)
    double tau_floor;             // 1 / log10(n), formed on the host
};
struct TmMdCovArgs {
    const double *table, *mean;
    const int32_t *sel;           // [n_sel] columns, device memory
    double *S;                    // [n_sel][n_sel]
    long long n, max_samples;     // 2 <= n <= max_samples
    int32_t n_cols, n_sel;        // 1 <= n_sel <= TM_MD_MAX_COLS
};

int tm_launch_modediag_lag(const TmMdArgs &a, void *stream);       // each returns a hipError_t
int tm_launch_modediag_finish(const TmMdArgs &a, void *stream);
int tm_launch_modediag_cov(const TmMdCovArgs &a, void *stream);
