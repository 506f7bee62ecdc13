// tamcmc_summary_walk.h -- what the stage-2 kernels of a posterior summary share: the pointwise log-likelihood and the
// residual of one (sample, bin), the walk of one bin over a block's model rows, the grid size of a one-thread-per-bin launch.
//
//   l         chi(2,2p)    l = -p (y / M + log M)                      likelihoods.cpp:17-29, per bin
//             chi_square   l = -(y - M)^2 / sigma^2                    likelihoods.cpp:31-39 (the reference's convention: no 1/2)
//   residual  chi(2,2p)    y / M
//             chi_square   (y - M) / sigma, sigma given as sqrt(1 / sigma^2)
// Both are free of FMA contraction whatever the including file's own setting is (the pragma sits inside the function
// bodies): a bin's results must not depend on which kernel formed its l.
//
//   walk      one thread owns one bin and walks the samples [b0, b1) of a block ONE AT A TIME IN PUSH ORDER: UNROLL row
//             loads (64-bit row offsets) are requested before the first is used; a sample whose status is not 0
//             (TAMCMC_CHAIN_OK) is skipped and counted -- its row is loaded and dropped; past b1 nothing is loaded.  The
//             status words come from device memory (a wave-uniform test); every thread counts the same samples.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TMS_FN __host__ __device__ inline
#define TMS_NO_FMA _Pragma("clang fp contract(off)")
#else
#define TMS_FN inline
#define TMS_NO_FMA                // g++ builds of this header pass -ffp-contract=off
#endif

TMS_FN double tms_like(const bool chi_square, const double y, const double M, const double isig2, const double p)
{
    TMS_NO_FMA
    if (chi_square) { const double dd = y - M; return -((dd * dd) * isig2); }
    return -p * (y / M + log(M));
}

// isig = sqrt(isig2): a kernel that walks many samples of one bin forms it once per bin
TMS_FN double tms_resid(const bool chi_square, const double y, const double M, const double isig)
{
    TMS_NO_FMA
    return chi_square ? (y - M) * isig : y / M;
}

inline unsigned tms_blocks(const long long Nx, const int threads) { return (unsigned)((Nx + threads - 1) / threads); }   // one thread per bin

// samples per block where the caller leaves it open (block_chains = 0): 64, lowered so that a block's rows -- B x Nx doubles --
// take at most 64 MiB; a grid whose single row is longer than that still gets 1
#define TMS_DEFAULT_BLOCK 64
#define TMS_DEFAULT_BLOCK_BYTES ((size_t)64 << 20)
inline int tms_default_block(const long long Nx)
{
    const size_t fit = TMS_DEFAULT_BLOCK_BYTES / ((size_t)Nx * sizeof(double));
    return fit >= TMS_DEFAULT_BLOCK ? TMS_DEFAULT_BLOCK : (fit >= 1 ? (int)fit : 1);
}

#if defined(__HIPCC__)
// What l of a bin needs besides M, from launch arguments with y, isig2 (NULL unless chi_square), likelihood_case, like_p
struct TmsBinLike {
    double y, isig2, p;
    bool chi_square;
    template <class A>
    __device__ __forceinline__ TmsBinLike(const A &a, const int bin)
        : y(a.y[bin]), isig2(a.likelihood_case != 0 ? a.isig2[bin] : 0.0), p(a.like_p), chi_square(a.likelihood_case != 0) {}
    __device__ __forceinline__ double l(const double M) const { return tms_like(chi_square, y, M, isig2, p); }
};

struct TmsCount { long long n, rej; };       // {accepted, rejected}

// rows: the bin's element of the block's first row, rows nx doubles apart; status: the block's.  For every accepted
// sample of [b0, b1), in push order, accept(v, n) is called with the model value and the number of accepted samples
// including this one.  Returns the counts after b1.  (Both counters are the walker's own locals: counters that the caller
// owns and the callable advances end up in scratch.)
template <int UNROLL, class F>
__device__ __forceinline__ TmsCount tms_walk(const double *__restrict__ rows, const int32_t *status, const int b0, const int b1,
                                             const size_t nx, const TmsCount in, F &&accept)
{
    long long n = in.n, rej = in.rej;
    for (int s0 = b0; s0 < b1; s0 += UNROLL) {
        double v[UNROLL];
#pragma unroll
        for (int k = 0; k < UNROLL; k++)
            v[k] = (s0 + k < b1) ? rows[(size_t)(s0 + k) * nx] : 1.0;
#pragma unroll
        for (int k = 0; k < UNROLL; k++) {
            if (s0 + k >= b1) break;
            if (status[s0 + k] != 0) { rej++; continue; }
            n++;
            accept(v[k], n);
        }
    }
    return TmsCount{n, rej};
}
#endif
