// tamcmc_compare.h -- the comparison of K fits of one spectrum from their pointwise log predictive values (tamcmc_compare_* in
// include/tamcmc_accel_compare.h, which holds the definitions of record).  Shared by the kernels (tamcmc_compare.hip), the host
// side (tamcmc_compare_api.cpp), the one-thread host timing (tools/compare_host_time.cpp) and the stand-alone check
// (tests/cpp/compare_core_check.cpp, plain g++):
//
//   variate      e = -log(u), u the (g & 1)-th uniform of tmn_uniforms(seed, g >> 1, i, 0) of tamcmc_scan_null.h: the two
//                replicates 2 m and 2 m + 1 share one Philox call                                  tmc_variates2, tmc_variate
//   inclusion    a unit is included iff elpd[k][i] is finite for every k                                       tmc_included
//   pair totals  on the host, in unit order, in long double                                                  tmc_pair_totals
//   bootstrap    per replicate A = sum e_i and B_k = sum e_i D_k,i over the included units, z_k = ((double)N' B_k) / A.  Order
//                of the sums: thread t of a tile owns the units j0 + t + 256 u, u = 0 ... 7 ascending; the 64 lanes of a wave
//                by the butterfly v += shfl_xor(v, d), d = 32 ... 1 (the same bits in every lane: + commutes); the four waves
//                in wave order; the tiles of TM_CMP_TILE units in tile order                                       tmc_z
//   chunk        replicates whose partial sums (tiles x K doubles each) fit scratch_bytes                          tmc_chunk
//   counting     prob, the rank of interval, softmax, pseudo-BMA+                tmc_prob, tmc_rank, tmc_softmax, tmc_bma_plus
//   stacking     P_k = exp(s (elpd_k - max_k' elpd_k')), den = w_0 P_0 + ... + w_{K-1} P_{K-1} in ascending k, the sums of
//                P_k / den and of log(den) in the order thread (units j0 + t + 256 u, u = 0 ... 15), lanes, waves, tiles of
//                TM_CMP_STACK_TILE units; then the EM update and the gap                          tmc_P, tmc_den, tmc_em_step
// tamcmc_compare.hip includes this header under `#pragma clang fp contract(off)`.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "tamcmc_scan_null.h"

#define TM_CMP_MAX_FITS 8                   // TAMCMC_COMPARE_MAX_FITS
#define TM_CMP_MAX_REPLICATES ((long long)1 << 24)     // TAMCMC_COMPARE_MAX_REPLICATES
#define TM_CMP_THREADS 256
#define TM_CMP_WAVES (TM_CMP_THREADS / 64)
#define TM_CMP_UPT 8                        // units a thread of the bootstrap kernel keeps in registers
#define TM_CMP_TILE (TM_CMP_THREADS * TM_CMP_UPT)      // TAMCMC_COMPARE_TILE
#define TM_CMP_PAIRS 8                      // pairs of replicates a workgroup works through with its D in registers
#define TM_CMP_STACK_UPT 16
#define TM_CMP_STACK_TILE (TM_CMP_THREADS * TM_CMP_STACK_UPT)     // TAMCMC_COMPARE_STACK_TILE
#define TM_CMP_STACK_COLS (TM_CMP_MAX_FITS + 1)         // the K sums of P_k / den, then the sum of log(den)
#define TM_CMP_SCRATCH ((long long)64 << 20)            // scratch_bytes = 0 of the bootstrap
#define TM_CMP_STACK_SCRATCH ((long long)1 << 30)       // scratch_bytes = 0 of the stacking
#define TM_CMP_CHUNK_MAX 65536
#define TM_CMP_K_HIGH 0.7
// LDS of the bootstrap kernel: per wave and replicate of the pair A and B_1 ... B_{K-1}
#define TM_CMP_LDS_BYTES (TM_CMP_WAVES * 2 * TM_CMP_MAX_FITS * 8)
// LDS of the stacking sums kernel: per wave the TM_CMP_STACK_COLS sums
#define TM_CMP_STACK_LDS_BYTES (TM_CMP_WAVES * TM_CMP_STACK_COLS * 8)

// ---- variate ----

// the variates of (unit i, global replicates 2 pair and 2 pair + 1)
TMP_FN void tmc_variates2(const uint64_t seed, const uint64_t pair, const uint32_t i, double *e_even, double *e_odd)
{
    double ue, uo;
    tmn_uniforms(seed, pair, i, 0u, &ue, &uo);
    *e_even = -log(ue);
    *e_odd = -log(uo);
}

TMP_FN double tmc_variate(const uint64_t seed, const uint64_t g, const uint32_t i)
{
    double e0, e1;
    tmc_variates2(seed, g >> 1, i, &e0, &e1);
    return (g & 1) ? e1 : e0;
}

// ---- inclusion ----

TMP_FN bool tmc_finite(const double v) { return v - v == 0.0; }       // false for NaN and +-inf

// elpd[k * N + i]
TMP_FN bool tmc_included(const int K, const double *elpd, const long long N, const long long i)
{
    bool ok = true;
    for (int k = 0; k < K; k++) ok = ok && tmc_finite(elpd[(size_t)k * (size_t)N + (size_t)i]);
    return ok;
}

// ---- stacking ----

TMP_FN double tmc_P(const double s, const double v, const double vmax) { return exp(s * (v - vmax)); }

// P_0 ... P_{K-1} of an included unit
TMP_FN void tmc_P_unit(const int K, const double *elpd, const long long N, const long long i, const double s, double *P)
{
    double vmax = elpd[i];
    for (int k = 1; k < K; k++) { const double v = elpd[(size_t)k * (size_t)N + (size_t)i]; vmax = v > vmax ? v : vmax; }
    for (int k = 0; k < K; k++) P[k] = tmc_P(s, elpd[(size_t)k * (size_t)N + (size_t)i], vmax);
}

TMP_FN double tmc_den(const int K, const double *w, const double *P)
{
    double den = w[0] * P[0];
    for (int k = 1; k < K; k++) den += w[k] * P[k];
    return den;
}

// the state of a stacking fit, on the device between the iterations
struct TmCmpStack {
    double w[TM_CMP_MAX_FITS], g[TM_CMP_MAX_FITS];
    double gap, f;
    long long iterations;
    int32_t converged, frozen;
};

TMP_FN void tmc_em_init(const int K, TmCmpStack *st)
{
    for (int k = 0; k < TM_CMP_MAX_FITS; k++) { st->w[k] = k < K ? 1.0 / (double)K : 0.0; st->g[k] = 0.0; }
    st->gap = 0.0; st->f = 0.0; st->iterations = 0; st->converged = 0; st->frozen = 0;
}

// one iteration from its sums: sum[k] = sum_i P_ki / den_i, sumlog = sum_i log(den_i), both at st->w
TMP_FN void tmc_em_step(const int K, const long long Np, const double *sum, const double sumlog, const double tol, const long long max_iter,
                        TmCmpStack *st)
{
    if (st->frozen) return;
    double gmax = sum[0] / (double)Np;
    for (int k = 0; k < K; k++) {
        const double g = sum[k] / (double)Np;
        st->g[k] = g;
        gmax = g > gmax ? g : gmax;
    }
    st->gap = gmax - 1.0;
    st->f = sumlog / (double)Np;
    st->iterations++;
    if (st->gap <= tol) { st->converged = 1; st->frozen = 1; }
    else if (st->iterations >= max_iter) st->frozen = 1;
    else
        for (int k = 0; k < K; k++) st->w[k] = st->w[k] * st->g[k];
}

// ---- bootstrap ----

TMP_FN double tmc_z(const long long Np, const double A, const double B) { return ((double)Np * B) / A; }

inline long long tmc_tiles(const long long N) { return (N + TM_CMP_TILE - 1) / TM_CMP_TILE; }
inline long long tmc_stack_tiles(const long long N) { return (N + TM_CMP_STACK_TILE - 1) / TM_CMP_STACK_TILE; }

// replicates per chunk: the partial sums of a replicate are tiles x K doubles, its z K - 1 doubles
inline long long tmc_chunk(const long long scratch_bytes, const long long tiles, const int K)
{
    const long long per = tiles * K * 8 + (K - 1) * 8;
    long long c = (scratch_bytes > 0 ? scratch_bytes : TM_CMP_SCRATCH) / per;
    long long groups = ((long long)1 << 30) / (tiles * TM_CMP_THREADS);          // at most 2^30 threads a launch
    groups = groups < 1 ? 1 : groups;
    const long long grid = 2 * TM_CMP_PAIRS * groups - 2;                         // (its slots fit `groups` workgroups)
    c = c < grid ? c : grid;
    c = c < TM_CMP_CHUNK_MAX ? c : TM_CMP_CHUNK_MAX;
    return c < 1 ? 1 : c;
}
// pairs of replicates (slots of the partials) that n replicates from global replicate g0 touch
TMP_FN long long tmc_slots(const unsigned long long g0, const long long n) { return (long long)(((g0 + (unsigned long long)n - 1) >> 1) - (g0 >> 1)) + 1; }
// slots the partials of a chunk of c replicates need at most
inline long long tmc_slots_max(const long long c) { return c / 2 + 1; }

// ---- host-only arithmetic ----

struct TmCmpTotals {
    long long n_included, n_excluded, n_better, n_worse, n_k_high;
    double elpd_diff, se_diff, diff_k_high;
};

// the pair (a, b); khat NULL: n_k_high = -1, diff_k_high = NaN
inline TmCmpTotals tmc_pair_totals(const int K, const long long N, const double *elpd, const double *khat, const int a, const int b)
{
    TmCmpTotals t{};
    const double *ea = elpd + (size_t)a * (size_t)N, *eb = elpd + (size_t)b * (size_t)N;
    long double sum = 0.0L, sum_high = 0.0L;
    for (long long i = 0; i < N; i++) {
        if (!tmc_included(K, elpd, N, i)) { t.n_excluded++; continue; }
        t.n_included++;
        const double d = ea[i] - eb[i];
        sum += (long double)d;
        if (d > 0.0) t.n_better++;
        if (d < 0.0) t.n_worse++;
        if (khat) {
            const double ka = khat[(size_t)a * (size_t)N + (size_t)i], kb = khat[(size_t)b * (size_t)N + (size_t)i];
            if (ka > TM_CMP_K_HIGH || kb > TM_CMP_K_HIGH) { t.n_k_high++; sum_high += (long double)d; }     // (a NaN compares false)
        }
    }
    const double nan = std::nan("");
    if (!khat) t.n_k_high = -1;
    if (t.n_included == 0) { t.elpd_diff = t.se_diff = t.diff_k_high = nan; return t; }
    t.elpd_diff = (double)sum;
    t.diff_k_high = khat ? (double)sum_high : nan;
    if (t.n_included < 2) { t.se_diff = nan; return t; }
    const long double mean = sum / (long double)t.n_included;
    long double ss = 0.0L;
    for (long long i = 0; i < N; i++) {
        if (!tmc_included(K, elpd, N, i)) continue;
        const long double c = (long double)(ea[i] - eb[i]) - mean;
        ss += c * c;
    }
    t.se_diff = (double)sqrtl((long double)t.n_included / (long double)(t.n_included - 1) * ss);
    return t;
}

// rank of quantile q among R values: ceil(q R) - 1 clamped (tmq_rank of tamcmc_quantile.h)
inline long long tmc_rank(const double q, const long long R)
{
    long long k = (long long)ceil(q * (double)R) - 1;
    if (k < 0) k = 0;
    if (k > R - 1) k = R - 1;
    return k;
}

// z[r * (K - 1) + k - 1] for k >= 1, 0 for k = 0
inline double tmc_z_at(const double *z, const int K, const long long r, const int k) { return k == 0 ? 0.0 : z[(size_t)r * (size_t)(K - 1) + (size_t)(k - 1)]; }

inline void tmc_prob(const double *z, const int K, const long long R, const int a, const int b, long long *n_greater, long long *n_equal)
{
    long long gt = 0, eq = 0;
    for (long long r = 0; r < R; r++) {
        const double za = tmc_z_at(z, K, r, a), zb = tmc_z_at(z, K, r, b);
        if (za > zb) gt++;
        if (za == zb) eq++;
    }
    *n_greater = gt; *n_equal = eq;
}

inline double tmc_interval(const double *z, const int K, const long long R, const int a, const int b, const double q)
{
    std::vector<double> d((size_t)R);
    for (long long r = 0; r < R; r++) d[(size_t)r] = tmc_z_at(z, K, r, a) - tmc_z_at(z, K, r, b);
    const long long k = tmc_rank(q, R);
    std::nth_element(d.begin(), d.begin() + k, d.end());
    return d[(size_t)k];
}

// w_k = exp(x_k - max x) / sum_j exp(x_j - max x), the sum in ascending j
inline void tmc_softmax(const int K, const double *x, double *w)
{
    double m = x[0];
    for (int k = 1; k < K; k++) m = x[k] > m ? x[k] : m;
    double sum = 0.0;
    for (int k = 0; k < K; k++) { w[k] = exp(x[k] - m); sum += w[k]; }
    for (int k = 0; k < K; k++) w[k] = w[k] / sum;
}

// pseudo-BMA+: the mean over r, in r order, of the softmax over k of s z_rk
inline void tmc_bma_plus(const double *z, const int K, const long long R, const double s, double *w)
{
    double acc[TM_CMP_MAX_FITS] = {0.0}, x[TM_CMP_MAX_FITS], v[TM_CMP_MAX_FITS];
    for (long long r = 0; r < R; r++) {
        for (int k = 0; k < K; k++) x[k] = s * tmc_z_at(z, K, r, k);
        tmc_softmax(K, x, v);
        for (int k = 0; k < K; k++) acc[k] += v[k];
    }
    for (int k = 0; k < K; k++) w[k] = acc[k] / (double)R;
}

// ---- launch arguments (tamcmc_compare.hip) ----
struct TmCmpArgs {
    const double *elpd;           // [K][N] on the device
    double *part;                 // [slots][2][tiles][K]: A in column 0, B_k in column k, of replicates 2 (g0 / 2 + slot) + half
    double *z;                    // [n][K - 1] of the chunk
    unsigned long long seed;
    unsigned long long g0;        // global replicate of the chunk's first
    long long N, Np;
    int32_t K, tiles;
    int32_t n;                    // replicates of the chunk
    int32_t pad;
};

struct TmCmpStackArgs {
    const double *elpd;           // [K][N]
    double *P;                    // [K][N] or NULL: formed again in every iteration; P[i] < 0 marks an excluded unit
    double *part;                 // [tiles][TM_CMP_STACK_COLS]
    TmCmpStack *state;
    double scale, tol;
    long long N, Np, max_iter;
    int32_t K, tiles;
};

// the sums kernel and the finish kernel of a chunk on `stream`; returns a hipError_t
int tm_launch_compare_bootstrap(const TmCmpArgs &a, void *stream);
// the variates of global replicate g into d_e[N]
int tm_launch_compare_variates(const TmCmpArgs &a, unsigned long long g, double *d_e, void *stream);
// the table of P
int tm_launch_compare_prepare(const TmCmpStackArgs &a, void *stream);
// n iterations: sums kernel and update kernel each
int tm_launch_compare_iterations(const TmCmpStackArgs &a, int n, void *stream);
