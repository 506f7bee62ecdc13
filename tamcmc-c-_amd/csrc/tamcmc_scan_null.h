// tamcmc_scan_null.h -- Monte-Carlo null of the sliding-window scan (tamcmc_scan_null_* in include/tamcmc_accel.h): the law of
// the scan's extremes over all positions of every width under a correctly specified model, simulated once, and the lines and
// p-values read off it by counting.  The scan's default line log(0.01 W / Nx) is Bonferroni over Nx / W independent windows
// per width: neither the overlap of neighbouring positions nor the several widths enter it.
//
// If the model is right, y_i / M_i is Gamma(p, 1 / p) for chi(2,2p) and r_i is N(0, 1/2) for chi_square, independent of the
// model: the null depends on (likelihood, p, Nx, widths) alone and on no context or chain.
//
//   generator    Philox4x32-10, key = (seed low, seed high), counter = (bin, pair index t, replicate low, replicate high):
//                the variate of (bin, replicate) is a function of these alone, so a workgroup generates its tile AND the halo
//                its widest window reaches into, without talking to its neighbour, and nothing of size R x Nx ever exists.
//                                                                                                     tmn_philox, tmn_uniform
//   variate      chi(2,2p): q = (e_0 + ... + e_{p-1}) / (double)p, e_k = -log(u_k), u_k the (k & 1)-th uniform of call t = k >> 1,
//                added in ascending k.  chi_square: q = sqrt(-log(u_even)) cospi(2 u_odd) of call t = 0: variance 1/2, the
//                likelihood taken at its word as in the predictive check.                                        tmn_variate
//   sums         S = tmw_sum(q + j, W_k) for every position j of every width k: the scan sums kernel's walk, one ascending sum
//                per position taken off at every width.  Not stored: per (replicate, width) the maximum with its first
//                position and the minimum with its first position.                                    tmn_takes, tmn_combine
//   statistic    on the host with the scan's own tail functions: which = 0 (excess) min_log = log Q at S_max, which = 1
//                (deficit) log P at S_min.  The tails are monotone in S: this is the minimum over positions of what the scan
//                computes for a chain of one sample.
//   calibration  integer counting over the R replicates so far, per side (TmNullCalib below).
//
// The generator, the variate, the combine rule and the calibration are plain C++17, callable from g++
// (tests/cpp/scan_null_core_check.cpp); tamcmc_scan_null.hip includes this header under `#pragma clang fp contract(off)`.
#pragma once
#include <algorithm>
#include <vector>

#include "tamcmc_scan.h"

#define TM_NULL_THREADS 256
#define TM_NULL_WAVES (TM_NULL_THREADS / 64)
#define TM_NULL_MAX_REPLICATES ((long long)1 << 24)     // TAMCMC_SCAN_NULL_MAX_REPLICATES
// LDS of the extremes kernel: the tile's variates with their halo as in the scan sums kernel (2559 doubles, placed on 16
// bytes), and per wave, width and side one (value, position in the tile) -- 20 480 + 4 x 8 x 2 x 12 = 21 248 bytes
#define TM_NULL_LDS_BYTES ((TM_SCAN_LDS_DOUBLES * 8 + 15) / 16 * 16 + TM_NULL_WAVES * TM_SCAN_MAX_WIDTHS * 2 * 12)
#define TM_NULL_PARTIAL_BYTES ((long long)64 << 20)     // partials of one chunk of replicates, at most
#define TM_NULL_CHUNK_MAX 4096

// ---- generator ----

TMP_FN void tmn_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
    for (int round = 0; round < 10; round++) {
        const uint64_t a = (uint64_t)0xD2511F53u * c0, b = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(b >> 32) ^ c1 ^ k0, n2 = (uint32_t)(a >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)b; c3 = (uint32_t)a; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 52 bits of two words, centred in their cell: exact, and strictly inside (0, 1)
TMP_FN double tmn_uniform(const uint32_t wa, const uint32_t wb)
{
    return ((double)(((uint64_t)wa << 20) | (uint64_t)(wb >> 12)) + 0.5) * 0x1p-52;
}

// the two uniforms of call t of (bin, replicate)
TMP_FN void tmn_uniforms(const uint64_t seed, const uint64_t rep, const uint32_t bin, const uint32_t t, double *u_even, double *u_odd)
{
    uint32_t w[4];
    tmn_philox(bin, t, (uint32_t)rep, (uint32_t)(rep >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
    *u_even = tmn_uniform(w[0], w[1]);
    *u_odd = tmn_uniform(w[2], w[3]);
}

TMP_FN double tmn_cospi(const double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return cospi(x);
#else
    return cos(3.14159265358979323846 * x);       // the host never generates what the library hands out
#endif
}

// the variate of (bin, replicate): rep is the global replicate, first_replicate + r
TMP_FN double tmn_variate(const bool gauss, const int p, const uint64_t seed, const uint64_t rep, const uint32_t bin)
{
    double ue, uo;
    if (gauss) {
        tmn_uniforms(seed, rep, bin, 0u, &ue, &uo);
        return sqrt(-log(ue)) * tmn_cospi(2.0 * uo);
    }
    tmn_uniforms(seed, rep, bin, 0u, &ue, &uo);
    double z = -log(ue);
    if (p > 1) z += -log(uo);
    for (int k = 2; k < p; k += 2) {
        tmn_uniforms(seed, rep, bin, (uint32_t)(k >> 1), &ue, &uo);
        z += -log(ue);
        if (k + 1 < p) z += -log(uo);
    }
    return z / (double)p;
}

// ---- extremes ----

// does (v, pos) take the place of (best, best_pos): the larger (smaller) sum, and of equal sums the lower position.  A
// position below 0 marks "no window here" (its value is -inf for a maximum, +inf for a minimum) and never takes a place.
TMP_FN bool tmn_takes(const bool want_max, const double v, const long long pos, const double best, const long long best_pos)
{
    if (pos < 0) return false;
    if (best_pos < 0) return true;
    return (want_max ? v > best : v < best) || (v == best && pos < best_pos);
}

// the partials of one (replicate, width, side) over the tiles, `stride` apart, in tile order
TMP_FN void tmn_combine(const bool want_max, const int tiles, const size_t stride, const double *val, const long long *pos,
                        double *out_val, long long *out_pos)
{
    double best = want_max ? -(double)INFINITY : (double)INFINITY;
    long long at = -1;
    for (int t = 0; t < tiles; t++)
        if (tmn_takes(want_max, val[(size_t)t * stride], pos[(size_t)t * stride], best, at)) { best = val[(size_t)t * stride]; at = pos[(size_t)t * stride]; }
    *out_val = best;
    *out_pos = at;
}

// ---- host-only arithmetic ----

inline long long tmn_tiles(const long long Nx, const int W0) { return (tmsc_positions(Nx, W0) + TM_SCAN_TILE - 1) / TM_SCAN_TILE; }

// replicates per chunk: the partials of a chunk are 2 K tiles (value, position) pairs per replicate
inline long long tmn_chunk(const long long tiles, const int K)
{
    const long long per = 2LL * K * tiles * 16;
    long long c = TM_NULL_PARTIAL_BYTES / per;
    const long long grid = ((long long)1 << 30) / (tiles * TM_NULL_THREADS);     // at most 2^30 threads a launch
    c = c < grid ? c : grid;
    c = c < TM_NULL_CHUNK_MAX ? c : TM_NULL_CHUNK_MAX;
    return c < 1 ? 1 : c;
}

// min_log of one (width, side) from the extreme sum
inline double tmn_min_log(const bool gauss, const TmWinShape &sh, const int p, const int which, const double S)
{
    double lP, lQ;
    if (gauss) tmw_gauss(sh, S, &lP, &lQ);
    else tmw_chi(sh, p, S, &lP, &lQ);
    return which == 0 ? lQ : lP;
}

// Calibration of one side: m[k] = the R values of min_log of width k.  All of it is counting:
//   cnt[r][k] = #{r' : m[r'][k] <= m[r][k]},  vmin[r] = min_k cnt[r][k]
//   p_width(v) = (1 + n_v) / (R + 1) with n_v = #{r : m[r][k] <= v};  p_joint(v) = (1 + #{r : vmin[r] <= n_v}) / (R + 1)
//   line at level alpha, j = floor(alpha (R + 1)), 1 <= j <= R: per width the j-th smallest m[.][k]; jointly the c-th smallest
//   m[.][k], c = the j-th smallest vmin.  Without ties ceil(j / K) <= c <= j, and always joint line <= per-width line.
struct TmNullCalib {
    long long R = 0;
    int K = 0;
    std::vector<double> sorted[TM_SCAN_MAX_WIDTHS];       // m[.][k], ascending
    std::vector<long long> vmin;                          // ascending

    void build(const int K_, const long long R_, const std::vector<double> *m)
    {
        K = K_; R = R_;
        for (int k = 0; k < K; k++) {
            sorted[k].assign(m[k].begin(), m[k].begin() + R);
            std::sort(sorted[k].begin(), sorted[k].end());
        }
        vmin.assign((size_t)R, 0);
        for (long long r = 0; r < R; r++) {
            long long v = R;
            for (int k = 0; k < K; k++) {
                const long long c = count_le(k, m[k][(size_t)r]);
                v = c < v ? c : v;
            }
            vmin[(size_t)r] = v;
        }
        std::sort(vmin.begin(), vmin.end());
    }
    long long count_le(const int k, const double v) const
    {
        return (long long)(std::upper_bound(sorted[k].begin(), sorted[k].end(), v) - sorted[k].begin());
    }
    long long vmin_le(const long long n) const { return (long long)(std::upper_bound(vmin.begin(), vmin.end(), n) - vmin.begin()); }
    // j = floor(alpha (R + 1)), or 0 where that is no rank 1 ... R (a NaN alpha included)
    long long rank(const double alpha) const
    {
        const double j = floor(alpha * (double)(R + 1));
        return j >= 1.0 && j <= (double)R ? (long long)j : 0;
    }
    // the rank c of the joint line among m[.][k] (j itself for the per-width line)
    long long line_rank(const long long j, const bool joint) const { return joint ? vmin[(size_t)(j - 1)] : j; }
    double line(const int k, const long long j, const bool joint) const { return sorted[k][(size_t)(line_rank(j, joint) - 1)]; }
    void pvalue(const int k, const double v, double *p_width, double *p_joint) const
    {
        const long long n = count_le(k, v);
        *p_width = (double)(1 + n) / (double)(R + 1);
        *p_joint = (double)(1 + vmin_le(n)) / (double)(R + 1);
    }
};

// ---- launch arguments (tamcmc_scan_null.hip) ----
struct TmNullArgs {
    double *part_val;             // [C][tiles][K][2] partial extremes of a chunk: side 0 the maximum, side 1 the minimum
    long long *part_pos;          // [C][tiles][K][2] their first positions, -1: no window of this width starts in the tile
    double *ext_val;              // [C][K][2] the extremes of the chunk's replicates
    long long *ext_pos;           // [C][K][2]
    unsigned long long seed;
    unsigned long long rep0;      // global replicate of the chunk's first
    long long Nx;
    int32_t W[TM_SCAN_MAX_WIDTHS];
    int32_t K, tiles;
    int32_t n;                    // replicates of the chunk, <= C
    int32_t gauss, p;
};

// the extremes kernel and the combine kernel on `stream`; returns a hipError_t
int tm_launch_scan_null(const TmNullArgs &a, void *stream);
// the variates of global replicate `rep` into d_q[Nx], by the extremes kernel's generating function
int tm_launch_scan_null_variates(const TmNullArgs &a, unsigned long long rep, double *d_q, void *stream);
