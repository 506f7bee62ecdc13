// tamcmc_bandess.h -- effective sample size of the credible-band edges of a stored chain (tamcmc_summary_bandess_* in
// include/tamcmc_accel.h): per bin and threshold the 0 / 1 series b_t = (M_t <= thr), its lag products as integer counts,
// the centred lag products times n^2 as exact 64-bit integers, and Geyer's initial monotone sequence on them (tme_finish of
// tamcmc_ess.h, used as it stands).
//
// The arithmetic below is plain C++17: the kernels (tamcmc_bandess.hip), the host side (tamcmc_summary_api.cpp) and the
// stand-alone check (tests/cpp/bandess_core_check.cpp, built with g++) call these same functions.  Everything up to the
// conversion of E_k to double is integer arithmetic, so nothing depends on the order of additions.
//
//   series   b_t = (M_t <= thr) as the IEEE comparison of doubles                                          tmb_le
//            t = 0 ... n - 1 counts ACCEPTED samples in push order
//   storage  one bit per sample in 64-bit words, sample t in bit t mod 64 of word t / 64:
//              ring[RW]   word w in slot w mod RW, RW = ceil(L / 64) + 2: the chunk under way and the L bits before it span
//                         at most ceil(L / 64) + 2 words                                                  tmb_ring_words
//              head[HW]   words 0 ... HW - 1 as they were written, HW = ceil(L / 64): the first L bits      tmb_head_words
//            a pass is cut into chunks of at most TM_ESS_CHUNK pushed samples; a chunk's c <= 64 accepted bits are
//            appended at position t0 (one or two words of either array)                                   tmb_store_bits
//   counts   C_k = sum_{t=k}^{n-1} b_t b_{t-k}, k = 0 ... L: per chunk C_k += popcount(new & window_k), new = the chunk's bits
//            (bit i: sample t0 + i), window_k = the bits of samples t0 - k + i, a funnel shift over adjacent ring words;
//            samples before t = 0 are 0.  One thread owns TM_BANDESS_G consecutive lags                    tmb_lag_group
//            N = C_0;  H_k = the first k bits' count (head), T_k = the last k bits' count (ring): masked popcounts
//   centred  E_k = n^2 C_k - n N (2N - H_k - T_k) + (n - k) N^2 = n^2 sum_{t=k}^{n-1} (b_t - N/n)(b_{t-k} - N/n), in int64_t:
//            n < 2^20 keeps every term below 2^61 and |E_k| < 2^62                                          tmb_E, tmb_centred
//   finish   A_k = (double)E_k, then tme_finish(A, L, (double)n, 1 / log10(n))
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "tamcmc_ess.h"

#define TMB_FN TME_FN

#define TM_BANDESS_MAX_K 8              // TAMCMC_SUMMARY_MAX_QUANTILES
#define TM_BANDESS_MAX_N (1LL << 20)    // n_used must stay below this
#define TM_BANDESS_G 16                 // consecutive lags owned by one thread
#define TM_BANDESS_BINS 64              // lag kernel: a workgroup is TM_BANDESS_BINS bins x TM_BANDESS_GROUPS lag groups
#define TM_BANDESS_GROUPS 4
#define TM_BANDESS_THREADS 256          // pack and finish kernels: one thread per bin

TMB_FN int tmb_head_words(const int L) { return (L + 63) / 64; }
TMB_FN int tmb_ring_words(const int L) { return (L + 63) / 64 + 2; }

TMB_FN uint64_t tmb_le(const double v, const double thr) { return v <= thr ? 1u : 0u; }

// the low c bits, c = 0 ... 64
TMB_FN uint64_t tmb_low(const int c) { return c >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << c) - 1); }

// bits s ... s + 63 of the 128-bit value hi:lo, s = 0 ... 63
TMB_FN uint64_t tmb_funnel(const uint64_t lo, const uint64_t hi, const int s) { return s ? (lo >> s) | (hi << (64 - s)) : lo; }

// word w of the series as the ring holds it (ring: the bin's slot 0, slots `stride` words apart); words before the
// series are 0.  A word past the last one written holds stale bits: every caller masks them away.
TMB_FN uint64_t tmb_word(const uint64_t *ring, const size_t stride, const int RW, const long long w)
{
    return w < 0 ? 0 : ring[(size_t)((int)w % RW) * stride];                 // (w < 2^14: n < 2^20)
}

// the bits of samples p ... p + 63, p >= 0
TMB_FN uint64_t tmb_extract(const uint64_t *ring, const size_t stride, const int RW, const long long p)
{
    const long long w = p >> 6;
    return tmb_funnel(tmb_word(ring, stride, RW, w), tmb_word(ring, stride, RW, w + 1), (int)(p & 63));
}

// Appends the chunk's c accepted bits (nb: bit i is sample t0 + i, nothing above bit c - 1; 1 <= c <= 64) to the ring and,
// while they fall among its HW words, to the head.  A word is begun by the chunk whose first bit is its bit 0, which
// replaces whatever the slot held; the word a chunk runs over into is written whole.
TMB_FN void tmb_store_bits(uint64_t *ring, uint64_t *head, const size_t stride, const int RW, const int HW, const long long t0,
                           const int c, const uint64_t nb)
{
    const int w = (int)(t0 >> 6), o = (int)(t0 & 63);
    const size_t slot = (size_t)(w % RW) * stride;
    const uint64_t first = o ? (ring[slot] & tmb_low(o)) | (nb << o) : nb;
    ring[slot] = first;
    if (w < HW) head[(size_t)w * stride] = first;
    if (o + c > 64) {
        const uint64_t second = nb >> (64 - o);
        ring[(size_t)((w + 1) % RW) * stride] = second;
        if (w + 1 < HW) head[(size_t)(w + 1) * stride] = second;
    }
}

// One bin, one threshold and one group of lags k0 ... min(k0 + TM_BANDESS_G - 1, L) over the accepted samples t0 ... t1 - 1,
// whose bits are in the ring together with the L bits before t0.  C: the counter of lag k0, lags `cstride` counters apart.
// 0 <= t0 < t1 <= t0 + 64.  The windows of the group's lags start at samples t0 - k0 - (ng - 1) ... t0 - k0: with the chunk's
// 64 bits they lie within three adjacent words, loaded once.
TMB_FN void tmb_lag_group(const uint64_t *ring, const size_t stride, const int RW, const long long t0, const long long t1,
                          const int k0, const int L, uint32_t *C, const size_t cstride)
{
    constexpr int G = TM_BANDESS_G;
    const int ng = L + 1 - k0 < G ? L + 1 - k0 : G;
    const uint64_t nb = tmb_extract(ring, stride, RW, t0) & tmb_low((int)(t1 - t0));
    const long long pb = t0 - k0 - (ng - 1);
    const long long wb = pb >= 0 ? pb >> 6 : -((-pb + 63) >> 6);              // floor(pb / 64)
    const uint64_t a0 = tmb_word(ring, stride, RW, wb), a1 = tmb_word(ring, stride, RW, wb + 1), a2 = tmb_word(ring, stride, RW, wb + 2);
#pragma unroll
    for (int j = 0; j < G; j++) {
        if (j >= ng) break;
        const int sh = (int)(t0 - (k0 + j) - 64 * wb);                       // 0 ... 63 + G - 1
        const uint64_t win = sh < 64 ? tmb_funnel(a0, a1, sh) : tmb_funnel(a1, a2, sh - 64);
        C[(size_t)j * cstride] += (uint32_t)__builtin_popcountll(nb & win);
    }
}

// E_k; every term and the result stay within int64_t for n < 2^20 (0 <= C, H, T <= N <= n)
TMB_FN long long tmb_E(const long long n, const long long k, const long long N, const long long C, const long long H, const long long T)
{
    return n * n * C - n * N * (2 * N - H - T) + (n - k) * N * N;
}

// E_0 ... E_L of one bin and threshold after a complete pass of n samples, converted to Out (long long, or double: one
// rounding) into out[k * ostride].  H_k and T_k are masked popcounts: the whole words below (above) the one lag k ends in,
// plus that word's bits below sample k (from sample n - k on; the last word holds nothing past sample n - 1).
template <class Out>
TMB_FN void tmb_centred(const uint64_t *ring, const uint64_t *head, const size_t stride, const int RW, const long long n, const int L,
                        const uint32_t *C, const size_t cstride, Out *out, const size_t ostride)
{
    const long long N = C[0];
    long long Hbase = 0, Tbase = 0, hw_i = -1, tw_i = -1;
    uint64_t hw = 0, tw = 0;
    out[0] = (Out)tmb_E(n, 0, N, N, 0, 0);
    for (int k = 1; k <= L; k++) {
        const long long hi = (k - 1) >> 6, q = n - k, ti = q >> 6;          // L <= n - 1: q >= 1
        if (hi != hw_i) { Hbase += __builtin_popcountll(hw); hw = head[(size_t)hi * stride]; hw_i = hi; }
        if (ti != tw_i) { Tbase += __builtin_popcountll(tw); tw = tmb_word(ring, stride, RW, ti); tw_i = ti; }
        const long long H = Hbase + __builtin_popcountll(hw & tmb_low((int)(k - 64 * hi)));
        const long long T = Tbase + __builtin_popcountll(tw >> (q & 63));
        out[(size_t)k * ostride] = (Out)tmb_E(n, k, N, C[(size_t)k * cstride], H, T);
    }
}

#if defined(TMB_HOST_FEED)
// One bin and one threshold on the host, fed in pieces: the chunking, the packing, the ring, the head and the lag groups of
// the device path (tests/cpp/bandess_core_check.cpp).
#include <vector>
struct TmbHostSeries {
    int L, RW, HW;
    double thr;
    long long t = 0, rejected = 0;
    std::vector<uint64_t> ring, head;
    std::vector<uint32_t> C;
    TmbHostSeries(const int L_, const double thr_)
        : L(L_), RW(tmb_ring_words(L_)), HW(tmb_head_words(L_)), thr(thr_), ring((size_t)RW, ~(uint64_t)0), head((size_t)HW, 0),
          C((size_t)L_ + 1, 0) {}                                           // (the ring starts full of stale bits)
    // m pushed samples; ok == NULL: all accepted
    void push(const double *v, const unsigned char *ok, long long m)
    {
        while (m > 0) {
            const long long b = m < TM_ESS_CHUNK ? m : TM_ESS_CHUNK;
            uint64_t nb = 0;
            int c = 0;
            for (long long i = 0; i < b; i++) {
                if (ok && !ok[i]) { rejected++; continue; }
                nb |= tmb_le(v[i], thr) << c;
                c++;
            }
            if (c > 0) {
                tmb_store_bits(ring.data(), head.data(), 1, RW, HW, t, c, nb);
                for (int k0 = 0; k0 <= L; k0 += TM_BANDESS_G) tmb_lag_group(ring.data(), 1, RW, t, t + c, k0, L, C.data() + k0, 1);
            }
            t += c; v += b; m -= b;
            if (ok) ok += b;
        }
    }
    // after the last push: E_k as integers, A_k as doubles
    void centred(long long *E) const { tmb_centred(ring.data(), head.data(), 1, RW, t, L, C.data(), 1, E, 1); }
    void centred(double *A) const { tmb_centred(ring.data(), head.data(), 1, RW, t, L, C.data(), 1, A, 1); }
};
#endif

struct TmBandArgs {
    const double *rows;           // [B][Nx] model rows of the chunk
    const int32_t *status;        // [B] of the chunk's samples, device memory
    const double *thr;            // [K][Nx] thresholds
    uint64_t *ring;               // [K][RW][Nx]
    uint64_t *head;               // [K][HW][Nx]
    uint32_t *C;                  // [K][L + 1][Nx]
    void *work;                   // [L + 1][Nx] of 8 bytes: A_k (double) or E_k (int64) of the threshold being finished
    double *tau, *ess;            // [K][Nx] each (finish)
    int32_t *cut;                 // [K][Nx]
    const long long *cnt_in;      // {accepted, rejected} before the chunk / after it, as TmSummaryArgs
    long long *cnt_out;
    long long n;                  // the fold pass's accepted samples
    int32_t Nx, B;                // B <= TM_ESS_CHUNK samples in this chunk
    int32_t L, RW, HW, K;
    int32_t j, want_E;            // finish: the threshold; 1: write E_k into work as int64 and stop there
    double tau_floor;             // 1 / log10(n), formed on the host
};

// tamcmc_bandess.hip; each returns a hipError_t
int tm_launch_bandess_chunk(const TmBandArgs &a, void *stream);       // pack kernel, then lag kernel
int tm_launch_bandess_finish(const TmBandArgs &a, void *stream);      // one threshold (a.j)
