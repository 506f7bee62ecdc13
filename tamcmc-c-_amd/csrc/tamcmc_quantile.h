// tamcmc_quantile.h -- exact per-bin quantiles of a stored chain (tamcmc_summary_quantiles_* in include/tamcmc_accel.h):
// a radix selection on order-preserving integer keys, one thread per bin, a few bits per pass over the chain.
//
// The per-bin arithmetic below is plain C++17: the kernels (tamcmc_quantile.hip), the host side of the C ABI and the
// stand-alone check (tests/cpp/quantile_core_check.cpp, built with g++) all call these same functions.
//
//   key      v + 0.0 (so that -0 and +0 are one value), its 64 bits u:  key = (u >> 63) ? ~u : u | 2^63.  Strictly
//            monotone over all doubles that are not NaN, +-inf and denormals included.
//   offset   D = key(v) - key(min_M) in uint64 (exact, monotone: two values either side of a power of two cost no extra
//            pass), R = key(max_M) - key(min_M), u0 = bit_length(R) = the bin's unresolved bits (0: all samples equal).
//   state    per bin: u, the number of bits still unresolved; per (quantile, bin): prefix = (D of the order statistic)
//            >> u, and below = the number of samples whose D >> u is smaller than prefix.
//   a pass   every sample with D >> u == prefix is counted in cell (D >> (u - d)) & (2^d - 1), d = min(bits, u)
//   narrow   the cell that holds rank k - below becomes the next d bits of the prefix, below grows by the cells under it,
//            u -= d.  With u = 0 the prefix is D of the order statistic itself.
// No shift in here is ever by 64 or more.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TMQ_FN __host__ __device__ inline
#else
#define TMQ_FN inline
#endif

#define TM_Q_MAXQ 8               // quantiles per selection (TAMCMC_SUMMARY_MAX_QUANTILES)
#define TM_Q_MAXBITS 6            // bits per pass at most: 64 cells
#define TM_Q_DEFAULT_BITS 6
#define TM_Q_THREADS 64           // histogram kernel: one wave per workgroup, one bin per thread
#define TM_Q_UNROLL 8             // row loads in flight per thread
#define TM_Q_RUN 65535            // samples between two flushes of the 16-bit LDS counters: a counter cannot wrap
#define TM_Q_NARROW_THREADS 256   // narrow / init kernels

TMQ_FN uint64_t tmq_key(double v)
{
    v = v + 0.0;
    uint64_t u;
    memcpy(&u, &v, sizeof(u));
    return (u >> 63) ? ~u : (u | ((uint64_t)1 << 63));
}

TMQ_FN double tmq_unkey(uint64_t k)
{
    const uint64_t u = (k >> 63) ? (k & ~((uint64_t)1 << 63)) : ~k;
    double v;
    memcpy(&v, &u, sizeof(v));
    return v;
}

TMQ_FN int tmq_bit_length(uint64_t r)
{
    return r ? 64 - __builtin_clzll((unsigned long long)r) : 0;
}

// digits resolved by the next pass of a bin with u unresolved bits
TMQ_FN int tmq_digits(int u, int bits) { return u < bits ? u : bits; }

// Does a sample at offset D belong to the bracket (prefix, u), u >= 1?  If so *cell is its cell of the 2^d histogram.
TMQ_FN bool tmq_match(uint64_t D, uint64_t prefix, int u, int d, unsigned *cell)
{
    const uint64_t hi = u >= 64 ? (uint64_t)0 : (D >> u);
    *cell = (unsigned)((D >> (u - d)) & (((uint64_t)1 << d) - 1));
    return hi == prefix;
}

// Narrows (prefix, below) of one (quantile, bin) by its histogram hist[c * stride], c < 2^d, towards rank k; clears the
// cells it read.  A rank the cells do not hold (the pass did not see the fold pass's samples) ends in the top cell.
template <class Count>
TMQ_FN void tmq_narrow(uint64_t *prefix, uint64_t *below, uint64_t k, Count *hist, size_t stride, int d)
{
    const unsigned ncell = 1u << d;
    const uint64_t want = k - *below;
    uint64_t cum = 0, under = 0;
    unsigned digit = ncell - 1;
    bool found = false;
    for (unsigned c = 0; c < ncell; c++) {
        const uint64_t n = (uint64_t)hist[(size_t)c * stride];
        hist[(size_t)c * stride] = 0;
        if (!found && want < cum + n) { found = true; digit = c; under = cum; }
        cum += n;
    }
    *below += under;
    *prefix = (*prefix << d) | (uint64_t)digit;
}

// The bracket of (prefix, u) as offsets: [lo, hi], hi clipped to R.
TMQ_FN void tmq_bracket(uint64_t prefix, int u, uint64_t R, uint64_t *lo, uint64_t *hi)
{
    if (u >= 64) { *lo = 0; *hi = R; return; }
    *lo = prefix << u;
    const uint64_t h = *lo + ((((uint64_t)1 << u) - 1));
    *hi = h > R ? R : h;
}

// rank of quantile q among n samples: the smallest sample whose empirical CDF reaches q (numpy's inverted_cdf)
inline int64_t tmq_rank(double q, int64_t n)
{
    int64_t k = (int64_t)ceil(q * (double)n) - 1;
    if (k < 0) k = 0;
    if (k > n - 1) k = n - 1;
    return k;
}

// ---- launch arguments (tamcmc_quantile.hip) ----
struct TmQuantArgs {
    const double *rows;           // [B][Nx] model rows of the block (stage 1)
    const int32_t *status;        // [B]
    const double *fold_state;     // [TM_SUM_NSTATE][Nx] of the fold pass (init reads min_M, max_M)
    uint64_t *kmin, *R;           // [Nx] key(min_M), key(max_M) - key(min_M)
    uint32_t *u;                  // [Nx] unresolved bits
    uint64_t *prefix, *below;     // [Nq][Nx]
    const uint64_t *ranks;        // [Nq], device memory
    uint32_t *hist;               // [Nq][2^bits][Nx]
    const long long *cnt_in;      // {accepted, rejected} of this pass before the block / after it (as TmSummaryArgs)
    long long *cnt_out;
    uint32_t *flag;               // set to 1 by any thread that meets a sample outside the envelope
    int32_t Nx, B, Nq, bits;
};

int tm_launch_quantile_init(const TmQuantArgs &a, void *stream);      // return a hipError_t
int tm_launch_quantile_hist(const TmQuantArgs &a, void *stream);
int tm_launch_quantile_narrow(const TmQuantArgs &a, void *stream);
