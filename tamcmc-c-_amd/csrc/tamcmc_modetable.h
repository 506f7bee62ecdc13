// tamcmc_modetable.h -- the posterior mode table (tamcmc_modetable_* in include/tamcmc_accel.h): per stored sample the
// derived quantities of every multiplet and of the chain -- what tamcmc_derive.h makes of a params row, the same
// derivation the setup and backward kernels run -- and their statistics over the chain: count, mean, standard deviation,
// minimum, maximum and exact quantiles.
//
// Everything below is plain C++17: the kernels (tamcmc_modetable.hip), the host side of the C ABI
// (tamcmc_modetable_api.cpp) and the stand-alone check (tests/cpp/modetable_core_check.cpp, built with g++) call the same
// functions.
//
// Columns, a pure function of the context's TmLayout:
//   chain level, first:        inclination (degrees; 0 where the model has none), eta, a3, asymmetry
//   per multiplet j, in the chain's table order (tm_mult_nl of tamcmc_derive.h), l = its degree:
//       freq  width  height  amplitude  splitting  window_lo  window_hi  nu_m (m = -l ... l)  h_m (m = -l ... l)
//   height = sum_m h_m added in the order m = -l ... l;  amplitude = sqrt((pi height) width), the reference's convention
//   H = A^2 / (pi Gamma);  splitting is exactly 0.0 for l = 0;  [window_lo, window_hi) is the truncation window in bins.
//   n_cols = 4 + sum_j (7 + 2 (2 l_j + 1)).
//
// Running state per column: Welford mean and sum of squared deviations, minimum, maximum (the recurrences of
// tamcmc_summary.hip), one thread per column walking the accepted samples in push order -- no result bit depends on how
// the samples are cut into pushes and blocks.
//
// Quantiles: the accepted rows are kept column-major, table[col * max_samples + k] being column col of the k-th accepted
// sample.  A radix selection on the order-preserving keys of tamcmc_quantile.h, TM_MT_QBITS bits per pass: every sample
// whose offset D = key(v) - key(min) shares the quantile's prefix is counted in a cell of a 2^d histogram (tmq_match), the
// cell that holds the rank extends the prefix (tmq_narrow); with no bit left the prefix is D of the order statistic
// itself.  tm_mt_select below is that selection for one column and one rank, serially; the kernel runs the same steps with
// a workgroup per column, the histogram in LDS, all of a call's ranks in one sweep over the column per pass.
// (-0 and +0 are one key: a zero is returned as +0.)
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "tamcmc_dev.h"
#include "tamcmc_quantile.h"

enum {                            // TAMCMC_MODETABLE_* of tamcmc_accel.h
    TM_MT_INCLINATION = 0, TM_MT_ETA, TM_MT_A3, TM_MT_ASYMMETRY,
    TM_MT_FREQ, TM_MT_WIDTH, TM_MT_HEIGHT, TM_MT_AMPLITUDE, TM_MT_SPLITTING, TM_MT_WINDOW_LO, TM_MT_WINDOW_HI,
    TM_MT_NU_M, TM_MT_H_M,
    TM_MT_NKINDS
};
#define TM_MT_CHAIN_COLS 4        // chain-level columns
#define TM_MT_MULT_FIXED 7        // columns of a multiplet before its per-m columns
#define TM_MT_THREADS 64          // derive kernel: one wave per sample, one lane per multiplet (a loop past 64)
#define TM_MT_FOLD_THREADS 64     // fold kernel: one thread per column
#define TM_MT_FOLD_UNROLL 8       // row loads in flight per thread
#define TM_MT_QTHREADS 256        // quantile kernel: one workgroup per column
#define TM_MT_QBITS 8             // bits per pass of the selection: 256 cells of 32 bits per rank in LDS
#define TM_MT_BLOCK 4096          // samples per block at most
#define TM_MT_BLOCK_BYTES ((size_t)1 << 26)   // ... lowered so that a block's derived rows take at most 64 MiB

enum { TM_MT_MEAN = 0, TM_MT_M2, TM_MT_MIN, TM_MT_MAX, TM_MT_NSTATE };   // state[TM_MT_NSTATE][n_cols]

struct TmMtCol {                  // tamcmc_modetable_col
    int32_t kind, mult, order, l, m, param_index;
};

// (n, l) of multiplet j: tm_mult_nl of tamcmc_derive.h (device code there), restated for host and device
TM_HD inline void tm_mt_mult_nl(const TmLayout &L, int j, int *n, int *l)
{
    if (L.family == TM_FAM_GLOBAL) {
        *n = j / (L.lmax + 1);
        *l = j % (L.lmax + 1);
    } else {
        int ll = 0, jj = j;
        while (ll < 3 && jj >= L.Nfl[ll]) { jj -= L.Nfl[ll]; ll++; }
        *n = jj; *l = ll;
    }
}

TM_HD inline int tm_mt_mult_cols(int l) { return TM_MT_MULT_FIXED + 2 * (2 * l + 1); }

// first column of multiplet j, 0 <= j <= n_mult (j = n_mult: the number of columns)
TM_HD inline int tm_mt_mult_first(const TmLayout &L, int j)
{
    int c = TM_MT_CHAIN_COLS;
    if (L.family == TM_FAM_GLOBAL) {
        const int n = j / (L.lmax + 1), l = j % (L.lmax + 1);
        int per = 0, before = 0;
        for (int ll = 0; ll <= L.lmax; ll++) {
            if (ll < l) before += tm_mt_mult_cols(ll);
            per += tm_mt_mult_cols(ll);
        }
        return c + n * per + before;
    }
    int jj = j;
    for (int ll = 0; ll < 4; ll++) {
        if (ll == 3 || jj < L.Nfl[ll]) { c += jj * tm_mt_mult_cols(ll); break; }
        c += L.Nfl[ll] * tm_mt_mult_cols(ll);
        jj -= L.Nfl[ll];
    }
    return c;
}

TM_HD inline int tm_mt_ncols(const TmLayout &L) { return tm_mt_mult_first(L, L.n_mult); }

// The layout: every column's description into out[0 ... n_cols - 1] (out may be NULL); returns n_cols.
inline int tm_mt_layout(const TmLayout &L, TmMtCol *out)
{
    const int n_cols = tm_mt_ncols(L);
    if (!out) return n_cols;
    for (int k = 0; k < TM_MT_CHAIN_COLS; k++) out[k] = TmMtCol{TM_MT_INCLINATION + k, -1, -1, -1, 0, -1};
    for (int j = 0; j < L.n_mult; j++) {
        int n, l;
        tm_mt_mult_nl(L, j, &n, &l);
        TmMtCol *o = out + tm_mt_mult_first(L, j);
        for (int k = 0; k < TM_MT_MULT_FIXED; k++) o[k] = TmMtCol{TM_MT_FREQ + k, j, n, l, 0, -1};
        o[0].param_index = L.off_f[l] + n;                       // TmMultFull::idx_f
        const int nc = 2 * l + 1;
        for (int k = 0; k < nc; k++) {
            o[TM_MT_MULT_FIXED + k] = TmMtCol{TM_MT_NU_M, j, n, l, k - l, -1};
            o[TM_MT_MULT_FIXED + nc + k] = TmMtCol{TM_MT_H_M, j, n, l, k - l, -1};
        }
    }
    return n_cols;
}

// samples per block of a table with n_cols columns
inline int tm_mt_block(int n_cols)
{
    const size_t fit = TM_MT_BLOCK_BYTES / ((size_t)n_cols * sizeof(double));
    return fit >= TM_MT_BLOCK ? TM_MT_BLOCK : (fit < 1 ? 1 : (int)fit);
}

// device bytes of an object (the header comment of tamcmc_modetable_create states them)
inline size_t tm_mt_table_bytes(long long max_samples, int n_cols) { return (size_t)max_samples * (size_t)n_cols * sizeof(double); }
inline size_t tm_mt_block_bytes(int B, int Nparams, int n_cols) { return (size_t)B * ((size_t)(Nparams + n_cols) * sizeof(double) + 2 * sizeof(int32_t)); }
inline size_t tm_mt_state_bytes(int n_cols) { return (size_t)(2 * TM_MT_NSTATE + TM_Q_MAXQ) * (size_t)n_cols * sizeof(double) + TM_Q_MAXQ * sizeof(uint64_t); }

// One Welford / envelope step of a column: v is its n-th accepted value (n >= 1)
TM_HD inline void tm_mt_fold_one(double &mean, double &M2, double &mn, double &mx, const long long n, const double v)
{
    const double d = v - mean;
    mean += d / (double)n;
    M2 += d * (v - mean);
    if (n == 1) { mn = v; mx = v; }
    else { mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
}

// The order statistic of rank k (0-based) of col[0], col[stride], ..., n of them, none a NaN, whose minimum and maximum
// are vmin and vmax: the selection the quantile kernel runs, serially.
inline double tm_mt_select(const double *col, size_t stride, long long n, double vmin, double vmax, uint64_t k, int bits = TM_MT_QBITS)
{
    const uint64_t kmin = tmq_key(vmin), R = tmq_key(vmax) - kmin;
    uint64_t prefix = 0, below = 0;
    uint32_t hist[1 << TM_MT_QBITS] = {};
    for (int u = tmq_bit_length(R); u > 0;) {
        const int d = tmq_digits(u, bits);
        for (long long i = 0; i < n; i++) {
            unsigned cell;
            if (tmq_match(tmq_key(col[(size_t)i * stride]) - kmin, prefix, u, d, &cell)) hist[cell]++;
        }
        tmq_narrow(&prefix, &below, k, hist, 1, d);
        u -= d;
    }
    return tmq_unkey(kmin + prefix);
}

// ---- launch arguments (tamcmc_modetable.hip) ----
struct TmMtDeriveArgs {
    TmLayout L;
    const double *params;         // [B][L.Nparams]
    double *rows;                 // [B][n_cols]
    int32_t *status;              // [B] TAMCMC_CHAIN_*
    int32_t B, n_cols;
};

struct TmMtFoldArgs {
    const double *rows;           // [B][n_cols] of the derive kernel
    const int32_t *accept;        // [B] non-zero: the sample enters the statistics
    double *state;                // [TM_MT_NSTATE][n_cols]
    double *table;                // [n_cols][max_samples], or NULL
    long long n_before;           // accepted samples before this block
    long long max_samples;
    int32_t B, n_cols;
};

struct TmMtQuantArgs {
    const double *table;          // [n_cols][max_samples]
    const double *state;          // the fold's: minimum and maximum of every column
    const uint64_t *ranks;        // [Nq], device memory
    double *out;                  // [Nq][n_cols]
    long long n, max_samples;     // accepted samples, 1 <= n <= max_samples
    int32_t n_cols, Nq;
};

int tm_launch_modetable_derive(const TmMtDeriveArgs &a, size_t lds_bytes, void *stream);    // return a hipError_t
int tm_launch_modetable_fold(const TmMtFoldArgs &a, void *stream);
int tm_launch_modetable_quantiles(const TmMtQuantArgs &a, void *stream);
