// tamcmc_eval_body.h -- device code of the eval kernel (helpers + the per-workgroup body), shared by the two launch
// shapes: tamcmc_eval_kernel (one workgroup per (chain, tile), records prepared by tamcmc_setup_kernel) and
// tamcmc_fused_kernel (short grids with one tile per chain: setup and evaluation in one launch).
// See tamcmc_eval.hip for the description of the algorithm.
#ifndef TAMCMC_EVAL_BODY_H
#define TAMCMC_EVAL_BODY_H
#include <hip/hip_runtime.h>
#include "tamcmc_dev.h"

#define TM_WAVES (TM_THREADS / 64)

// The gradient kernels' cross-wave sums.  Every wave owns TM_ROWS rows of TM_GSLOTS doubles in LDS that only it writes:
// row 0 the likelihood partial (S1, Pm, Pe), rows 1 and 2 the noise sums of the (at most two) cells a tile meets, rows
// 3 .. 3 + TM_ROW_K - 1 the butterfly results of up to TM_ROW_K consecutive active multiplets.  The workgroup adds the
// four waves' rows ONCE per chunk of TM_ROW_K multiplets (tm_eval_body, "flush"), behind the tile's only barrier in the
// common case.  4 waves x 9 rows x 192 B = 6912 B beside the 32 KiB of weights: 39 680 B = 31 LDS granules of 1280 B,
// so four workgroups stay resident on a CU's 160 KiB (one more row per wave would still fit, with nothing to spare).
#define TM_ROW_K 6
#define TM_ROWS (3 + TM_ROW_K)
static_assert(TM_ROWS * TM_GSLOTS <= TM_THREADS, "the flush takes one (row, slot) per thread");
// -DTM_TILE_BARRIERS=1: timing-only A/B build that keeps the rows and the flush but waits at every site where the
// workgroup used to synchronise inside the tile (profiles/README.md, "rowsums/")
#ifndef TM_TILE_BARRIERS
#define TM_TILE_BARRIERS 0
#endif
// pass 2 with look-ahead: the grid's partial last unit behind the pipelined loop (tm_grad_mult); -DTM_TAIL_APART=0/1 for A/B runs
#ifndef TM_TAIL_APART
#define TM_TAIL_APART 1
#endif
#if TM_TILE_BARRIERS
#define TM_TILE_SYNC() __syncthreads()
#else
#define TM_TILE_SYNC() do { } while (0)
#endif

// A multiplet record addressed through the CONSTANT address space: with a wave-uniform address the compiler
// fetches it with scalar loads (s_load_dwordx8/x16) into SGPRs, which VALU instructions take directly as one
// operand -- no LDS read, no VGPRs for the record.  The table was written by the previous kernel (setup), so
// it is invariant for this launch.
typedef const __attribute__((address_space(4))) TmMult *TmMultK;
typedef const __attribute__((address_space(4))) TmCellRec *TmCellRecK;
typedef const __attribute__((address_space(4))) TmTileHdr *TmTileHdrK;
typedef const __attribute__((address_space(4))) TmNoise *TmNoiseK;
typedef const __attribute__((address_space(4))) int32_t *TmIdxK;
typedef const __attribute__((address_space(4))) TmActive *TmActiveK;

// One entry of a tile's active list as ONE 16-byte scalar load (s_load_dwordx4): {idx, imin, imax, shape}.
typedef int TmEntry __attribute__((ext_vector_type(4)));
__device__ __forceinline__ TmEntry tm_load_entry(TmActiveK p)
{
    return *reinterpret_cast<const __attribute__((address_space(4))) TmEntry *>(p);
}

// 1/x for finite, normal, positive x: v_rcp_f64 + two Newton steps (no scaling / fix-up needed
// because every denominator here is bounded away from the subnormal and overflow ranges).
__device__ __forceinline__ double tm_rcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    return r;
}

// The same with one Newton step: 2.2e-15 relative (tools/rcp_accuracy.hip).  Used by pass 2 of the gradient kernel only
// -- the gradient is new functionality checked against finite differences (2e-5), and its sums carry cancellation far
// above that level; everything that enters logL keeps the two-step form.
__device__ __forceinline__ double tm_rcp1(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    const double e = __builtin_fma(-x, r, 1.0);
    return __builtin_fma(r, e, r);
}

// ---- lane exchanges without LDS traffic -----------------------------------------------------------
// __shfl_xor compiles to ds_bpermute_b32 (two per double, through the LDS crossbar); the reductions of the gradient
// pass issue ~50 of them per multiplet and wave and were bound by that path (profiles/README.md).  gfx950 has
// v_permlane32_swap / v_permlane16_swap for the two wide steps, and DPP covers masks 1..8 (semantics checked on the
// hardware with tools/xor_exchange_probe.hip).
template <int MASK>
__device__ __forceinline__ unsigned tm_xor_dw(unsigned v, int lane)
{
    if constexpr (MASK == 1) return __builtin_amdgcn_update_dpp(0u, v, 0xB1, 0xf, 0xf, false);        // quad_perm [1,0,3,2]
    else if constexpr (MASK == 2) return __builtin_amdgcn_update_dpp(0u, v, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
    else if constexpr (MASK == 4) {
        const unsigned r = __builtin_amdgcn_update_dpp(0u, v, 0x104, 0xf, 0x5, false);                // row_shl:4 -> banks 0, 2
        return __builtin_amdgcn_update_dpp(r, v, 0x114, 0xf, 0xa, false);                             // row_shr:4 -> banks 1, 3
    } else if constexpr (MASK == 8) return __builtin_amdgcn_update_dpp(0u, v, 0x128, 0xf, 0xf, false); // row_ror:8
    else if constexpr (MASK == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
        return (lane & 16) ? r[0] : r[1];
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return (lane & 32) ? r[0] : r[1];
    }
}

template <int MASK>
__device__ __forceinline__ double tm_xor(double v, int lane)   // the value lane ^ MASK holds
{
    const unsigned long long b = __double_as_longlong(v);
    const unsigned lo = tm_xor_dw<MASK>((unsigned)b, lane), hi = tm_xor_dw<MASK>((unsigned)(b >> 32), lane);
    return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

// One butterfly step on a PAIR of values with the two-register swaps: returns, in lanes with the MASK bit clear,
// a[lane] + a[lane ^ MASK], and in lanes with the bit set, b[lane ^ MASK] + b[lane]  (MASK = 16 or 32 only).
template <int MASK>
__device__ __forceinline__ double tm_swap_add(double a, double b)
{
    static_assert(MASK == 16 || MASK == 32, "two-register swaps exist for 16 and 32 lanes");
    const unsigned long long ba = __double_as_longlong(a), bb = __double_as_longlong(b);
    unsigned r0l, r1l, r0h, r1h;
    if constexpr (MASK == 32) {
        const auto l = __builtin_amdgcn_permlane32_swap((unsigned)ba, (unsigned)bb, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap((unsigned)(ba >> 32), (unsigned)(bb >> 32), false, false);
        r0l = l[0]; r1l = l[1]; r0h = h[0]; r1h = h[1];
    } else {
        const auto l = __builtin_amdgcn_permlane16_swap((unsigned)ba, (unsigned)bb, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap((unsigned)(ba >> 32), (unsigned)(bb >> 32), false, false);
        r0l = l[0]; r1l = l[1]; r0h = h[0]; r1h = h[1];
    }
    const double r0 = __longlong_as_double(((unsigned long long)r0h << 32) | r0l);
    const double r1 = __longlong_as_double(((unsigned long long)r1h << 32) | r1l);
    return r0 + r1;
}

__device__ __forceinline__ double tm_wave_sum(double v)   // lane 0 ends with the same tree as the shfl_down form
{
    const int lane = threadIdx.x & 63;
    v += tm_xor<32>(v, lane);
    v += tm_xor<16>(v, lane);
    v += tm_xor<8>(v, lane);
    v += tm_xor<4>(v, lane);
    v += tm_xor<2>(v, lane);
    v += tm_xor<1>(v, lane);
    return v;
}

__device__ __forceinline__ double tm_wave_prod(double v)   // product over the 64 lanes (every lane ends with it)
{
    const int lane = threadIdx.x & 63;
    v *= tm_xor<32>(v, lane);
    v *= tm_xor<16>(v, lane);
    v *= tm_xor<8>(v, lane);
    v *= tm_xor<4>(v, lane);
    v *= tm_xor<2>(v, lane);
    v *= tm_xor<1>(v, lane);
    return v;
}

// sum of log M over a tile, kept as (mantissa product, exponent sum): sum log M = log(mant) + e ln 2.  The product of the
// 64 lanes' running mantissas (each in [0.5, 1): at least 2^-64, no underflow) and then of the 4 waves' replaces a log per
// thread; the logs are taken once per tile by whoever sums the tiles (tm_tile_logsum).
// (tm_tile_logsum: tamcmc_dev.h, shared with the backward kernel)

// Horner evaluation of the cell's background polynomial; the coefficients are SGPR operands (scalar loads)
__device__ __forceinline__ double tm_poly(TmCellRecK tr, double z)
{
    double p = tr->bg[TM_PDEG];
#pragma unroll
    for (int j = TM_PDEG - 1; j >= 0; j--) p = __builtin_fma(p, z, tr->bg[j]);
    return p;
}

// ---- transposing butterfly: sums N values per lane over the 64 lanes of a wave -------------------
// One step with lane mask MASK halves the number of live values: lanes with the bit set keep the upper
// half.  After all steps lane L holds the total of slot tm_bfly_slot<N>(L) (replicated over the lane
// bits that were reduced plainly).  Cost: ~N exchanges instead of 6N.
template <int N, int MASK>
struct TmBfly {
    static constexpr int NE = (N + 1) & ~1;   // padded to even
    static constexpr int H = NE / 2;
    __device__ static __forceinline__ void run(double (&v)[TM_GSLOTS], int lane)
    {
        if constexpr (N == 1) {
            v[0] += tm_xor<MASK>(v[0], lane);
        } else if constexpr (MASK >= 16) {
#pragma unroll
            for (int i = 0; i < H; i++) v[i] = tm_swap_add<MASK>(v[i], (i + H < N) ? v[i + H] : 0.0);
        } else {
            const bool hi = (lane & MASK) != 0;
#pragma unroll
            for (int i = 0; i < H; i++) {
                const double up = (i + H < N) ? v[i + H] : 0.0;
                const double send = hi ? v[i] : up;
                const double keep = hi ? up : v[i];
                v[i] = keep + tm_xor<MASK>(send, lane);
            }
        }
        if constexpr (MASK > 1) TmBfly<(N == 1 ? 1 : H), MASK / 2>::run(v, lane);
    }
    // index (at this level) of the value lane `lane` ends up holding; valid = false if it is padding
    __device__ static __forceinline__ int slot_of(int lane, bool &valid)
    {
        if constexpr (N == 1) {
            return 0;
        } else {
            int sub = 0;
            if constexpr (MASK > 1) sub = TmBfly<H, MASK / 2>::slot_of(lane, valid);
            const int idx = sub + (((lane & MASK) != 0) ? H : 0);
            if (idx >= N) valid = false;
            return idx;
        }
    }
};

// Sum over the m-components of one multiplet at one bin, also returning d_m and every 1/E_m.
template <int NC>
__device__ __forceinline__ double tm_mult_value(double x2, const double (&nu2)[NC], const double (&hq)[NC], double g2,
                                                double (&d)[NC], double (&r)[NC])
{
    double E[NC], P[NC];
#pragma unroll
    for (int m = 0; m < NC; m++) {
        d[m] = x2 - nu2[m];
        E[m] = __builtin_fma(d[m], d[m], g2);
    }
    P[0] = E[0];
#pragma unroll
    for (int m = 1; m < NC; m++) P[m] = P[m - 1] * E[m];
    double inv = tm_rcp1(P[NC - 1]);
    double s = 0.0;
#pragma unroll
    for (int m = NC - 1; m >= 1; m--) {
        r[m] = inv * P[m - 1];
        inv = inv * E[m];
    }
    r[0] = inv;
#pragma unroll
    for (int m = 0; m < NC; m++) s = __builtin_fma(hq[m], r[m], s);
    return s;
}

// Forward only: the same sum as one rational N/Q built term by term (N <- N E_m + h_m Q, Q <- Q E_m: 3 ops per
// component instead of the 4 of batch inversion, whose individual 1/E_m only the gradient needs).
template <int NC>
__device__ __forceinline__ double tm_mult_sum(double x2, const double (&nu2)[NC], const double (&hq)[NC], double g2)
{
    double d = x2 - nu2[0];
    double Q = __builtin_fma(d, d, g2);
    double N = hq[0];
#pragma unroll
    for (int m = 1; m < NC; m++) {
        d = x2 - nu2[m];
        const double E = __builtin_fma(d, d, g2);
        N = __builtin_fma(hq[m], Q, N * E);
        Q = Q * E;
    }
    return N * tm_rcp(Q);
}

// Forward: add multiplet `sm` to acc[] for KG bins.  edge (wave-uniform) = false: the whole group lies inside the
// multiplet's window [imin, imax) and inside the grid, so no bin needs a test; edge = true: bins outside the window
// (bi[k] = -1 marks a bin outside the grid) get nothing -- the reference adds the multiplet inside its window only
// (build_lorentzian.cpp:423-427).  One copy of the arithmetic; the tests sit behind a scalar branch.
template <int NC, int KG, bool ASYM>
__device__ __forceinline__ void tm_accum_mult(TmMultK sm, const double (&x2)[KG], const int (&bi)[KG], double (&acc)[KG], const bool edge)
{
    // (the window itself is read from the record only on the edge path: rare, and the record is in flight anyway)
    double nu2[NC], hq[NC];
#pragma unroll
    for (int m = 0; m < NC; m++) { nu2[m] = sm->nu2[m]; hq[m] = sm->hq[m]; }
    const double g2 = sm->g2;
    const double aAh = ASYM ? 0.5 * sm->aA : 0.0, aB = ASYM ? sm->aB : 1.0, c2 = ASYM ? sm->c2 : 0.0;
    double s[KG];
#pragma unroll
    for (int k = 0; k < KG; k++) {
        s[k] = tm_mult_sum<NC>(x2[k], nu2, hq, g2);
        if (ASYM) {
            const double a = __builtin_fma(x2[k], aAh, aB);
            s[k] = s[k] * __builtin_fma(a, a, c2);
        }
    }
    if (edge) {
        const int imin = sm->imin, imax = sm->imax;
#pragma unroll
        for (int k = 0; k < KG; k++) {
            const bool inside = (bi[k] >= imin) && (bi[k] < imax);
            s[k] = inside ? s[k] : 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < KG; k++) acc[k] += s[k];
}

template <int KG>
__device__ __forceinline__ void tm_accum_dispatch(TmMultK sm, const int shape, const double (&x2)[KG], const int (&bi)[KG], double (&acc)[KG], const bool edge)
{
    // shape = ncomp | has_asym << 8, from the active list (known before the record arrives)
    switch (shape) {
    case 1: tm_accum_mult<1, KG, false>(sm, x2, bi, acc, edge); break;
    case 3: tm_accum_mult<3, KG, false>(sm, x2, bi, acc, edge); break;
    case 5: tm_accum_mult<5, KG, false>(sm, x2, bi, acc, edge); break;
    case 7: tm_accum_mult<7, KG, false>(sm, x2, bi, acc, edge); break;
    case 256 + 1: tm_accum_mult<1, KG, true>(sm, x2, bi, acc, edge); break;
    case 256 + 3: tm_accum_mult<3, KG, true>(sm, x2, bi, acc, edge); break;
    case 256 + 5: tm_accum_mult<5, KG, true>(sm, x2, bi, acc, edge); break;
    default: tm_accum_mult<7, KG, true>(sm, x2, bi, acc, edge); break;
    }
}

// Backward, one unit (2 bins per thread) of one multiplet: add this thread's terms to g[].  With d = 2x - 2nu, r = 1/E,
// wA the weight times the asymmetry factor, L = (NC - 1) / 2, the chain rule needs (tamcmc_backward.hip):
//   g[k]           = sum wA d_k r_k^2                      k = 0 .. NC-1   (d/d nu_k: every component has its own)
//   g[NC + am]     = sum wA (r_{L-am} + r_{L+am})          am = 0 .. L     (d/d height: the components +-m share theirs)
//   g[NC + L + 1]  = sum wA sum_k hq_k r_k^2                               (d/d Gamma^2: one per multiplet)
//   g[V-3 .. V-1]  = sum w S, sum w S a, sum w S a x   (S = un-asymmetrised multiplet sum; only if asym != 0)
// -- NC + L + 2 sums instead of 3 NC: fewer values to reduce over the workgroup per multiplet and tile.
// edge (wave-uniform) = false: the unit lies inside the window and the grid (no test per bin).  Only the fetch of x and
// of the weight differs between the two cases; the arithmetic exists once (two copies updating g[] behind a branch cost
// ~40 registers in copies at the join).
template <int NC> struct TmGradSlots {
    static constexpr int L = (NC - 1) / 2;
    static constexpr int A0 = NC, C = NC + L + 1, ASYM0 = NC + L + 2;
    __device__ static constexpr int count(bool asym) { return asym ? ASYM0 + 3 : ASYM0; }
};
// where the compact slot v of a multiplet with NC components is kept in a gmult row (TM_GSLOTS doubles):
// B_k at k, A_am at 7 + am, C at 11, the asymmetry sums at 21 .. 23
template <int NC> __device__ __forceinline__ int tm_grad_store_slot(int v)
{
    using SL = TmGradSlots<NC>;
    return (v < NC) ? v : (v < SL::C) ? 7 + (v - NC) : (v == SL::C) ? 11 : 21 + (v - SL::ASYM0);
}

// (the arithmetic of one bin: x2 and the weight wk, already zero outside the window, are values here)
template <int NC, bool ASYM>
__device__ __forceinline__ void tm_grad_bin(const double (&nu2)[NC], const double (&hq)[NC], double g2, double aAh, double aB, double c2,
                                            const double x2, const double wk, double (&g)[TM_GSLOTS])
{
    using SL = TmGradSlots<NC>;
    double d[NC], r[NC];
    const double Sv = tm_mult_value<NC>(x2, nu2, hq, g2, d, r);
    double wA = wk;
    if (ASYM) {
        const double a = __builtin_fma(x2, aAh, aB);
        wA = wk * __builtin_fma(a, a, c2);
        const double ws = wk * Sv;
        g[SL::ASYM0 + 0] += ws;
        g[SL::ASYM0 + 1] = __builtin_fma(ws, a, g[SL::ASYM0 + 1]);
        g[SL::ASYM0 + 2] = __builtin_fma(ws * a, 0.5 * x2, g[SL::ASYM0 + 2]);
    }
#pragma unroll
    for (int m = 0; m < NC; m++) {
        const double t1 = wA * r[m];
        const double t2 = t1 * r[m];
        const int am = (m >= SL::L) ? m - SL::L : SL::L - m;
        g[SL::A0 + am] += t1;
        g[m] = __builtin_fma(t2, d[m], g[m]);
        g[SL::C] = __builtin_fma(hq[m], t2, g[SL::C]);
    }
}

// One unit, fetched where it is used (the generic bodies): the wave waits for x and the weights at the head of the unit.
template <int NC, bool ASYM>
__device__ __forceinline__ void tm_grad_unit(const double (&nu2)[NC], const double (&hq)[NC], double g2, double aAh, double aB, double c2,
                                             int imin, int imax, const double *__restrict__ gx, const double *wq, int i0, int Nx,
                                             const bool edge, double (&g)[TM_GSLOTS])
{
#pragma unroll
    for (int k = 0; k < 2; k++) {
        double x2, wk;
        if (edge) {
            const int i = i0 + k * TM_THREADS;
            const bool inside = (i >= imin) && (i < imax) && (i < Nx);
            x2 = gx[i < Nx ? i : Nx - 1];
            wk = inside ? wq[k * TM_THREADS] : 0.0;
        } else {
            x2 = gx[i0 + k * TM_THREADS];
            wk = wq[k * TM_THREADS];
        }
        tm_grad_bin<NC, ASYM>(nu2, hq, g2, aAh, aB, c2, x2, wk, g);
    }
}

// The same unit with x and the weights fetched by the caller one unit ahead (tm_grad_fetch): values, not addresses.
// Only the edge path's select on the weight is left of the fetch; the bins outside the grid hold a weight of zero from
// pass 1 and a clamped x, and `inside` excludes them as above.
template <int NC, bool ASYM>
__device__ __forceinline__ void tm_grad_unit_held(const double (&nu2)[NC], const double (&hq)[NC], double g2, double aAh, double aB, double c2,
                                                  int imin, int imax, const double (&xv)[2], const double (&wv)[2], int lo, int tid, int Nx,
                                                  const bool edge, double (&g)[TM_GSLOTS])
{
    double wk[2] = {wv[0], wv[1]};
    if (edge) {
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int i = lo + tid + k * TM_THREADS;
            const bool inside = (i >= imin) && (i < imax) && (i < Nx);
            wk[k] = inside ? wk[k] : 0.0;
        }
        // (kept ONE branch: as selects on the scalar condition the tests cost 6 VALU per bin in every unit, and even the
        // bin index is made only here)
        asm volatile("" : "+v"(wk[0]), "+v"(wk[1]));
    }
#pragma unroll
    for (int k = 0; k < 2; k++) tm_grad_bin<NC, ASYM>(nu2, hq, g2, aAh, aB, c2, xv[k], wk[k], g);
}

// Request x and the two weights of unit u (units [u0, u1) of the tile, weights in s_w as pass 1 left them) for thread tid.
// Only the grid's last, partial unit needs its bin index clamped: a scalar test.  WHOLE: the caller keeps that unit out of
// its range, and the one form of the loads is left.
template <bool WHOLE>
__device__ __forceinline__ void tm_grad_fetch(const double *__restrict__ gx, const double *s_w, int u, int u0, int Nx, int tid,
                                              double (&xv)[2], double (&wv)[2])
{
    const int lo = u << TM_UNIT_SHIFT;
    if (WHOLE || lo + TM_UNIT_BINS <= Nx) {
        // the unit's own base (scalar arithmetic) + the thread index: no vector instruction per unit for the address
        // (behind an empty asm: otherwise the thread's part of the address is hoisted as a 64-bit pointer per thread and
        // the unit's offset added to it with a vector instruction per unit)
        typedef const __attribute__((address_space(1))) double *TmGlobalD;     // (stays a global_load behind the asm)
        TmGlobalD xb = (TmGlobalD)(gx + lo);
        asm volatile("" : "+s"(xb));
#pragma unroll
        for (int k = 0; k < 2; k++) xv[k] = xb[(unsigned)(tid + k * TM_THREADS)];
    } else {
#pragma unroll
        for (int k = 0; k < 2; k++) { const int i = lo + tid + k * TM_THREADS; xv[k] = gx[i < Nx ? i : Nx - 1]; }
        asm volatile("");     // (keeps the two forms of the loads apart: merged they address through a 64-bit pointer per thread)
    }
    const double *wq = s_w + (u - u0) * TM_UNIT_BINS + tid;
#pragma unroll
    for (int k = 0; k < 2; k++) wv[k] = wq[k * TM_THREADS];
}

// Backward: accumulate this thread's partial sums for multiplet `sm` over the tile's units [u0, u1), reduce over the wave
// and leave the wave totals in s_red_row[slot]: a row of the wave's own (TM_ROWS), so nothing here waits for another wave;
// the slots the shape does not use are left as they are (the flush stores them as zero without reading them).
// AHEAD (the common-case body): only the units that meet the window are walked -- the set the `continue` below selects --
// and x and the weights of the NEXT such unit are requested before the current one is evaluated, so that a wave waits for
// them behind ~30 NC fp64 instructions instead of in front of them.  The look-ahead index is clamped to the last unit of
// the range: the last trip requests its own unit again and discards it, the LDS read stays inside what pass 1 wrote.
// The empty asm behind the first fetch keeps the optimiser from folding the carried values back into loads of a carried
// address at the top of the trip (the loop without look-ahead, at the same register count): it pins the first unit's
// values in registers in front of the loop, where the only wait without work behind it is.
// The loop takes two units per iteration, the two sets of registers swapping roles, so that no value is copied from
// "next" to "current" (four v_mov_b64 per unit otherwise); what a unit costs beside its arithmetic is one vector
// instruction (the LDS address of the weights) -- pass 2 runs at the issue rate, so every instruction saved is time.
template <int NC, bool ASYM, bool AHEAD_>
__device__ __forceinline__ void tm_grad_mult(TmMultK sm, const double *__restrict__ gx, const double *s_w,
                                             int u0, int u1, int Nx, int tid, int lane, double *s_red_row)
{
    // l = 3 (NC = 7) keeps the fetch in place: its 12 / 15 accumulators and 28 temporaries leave no room for a second set
    // of x and weights (the kernel needs 123 VGPRs with look-ahead in the shape without asymmetry alone, 128 and 11
    // spilled to scratch with both; tests/test_eval_hot_path_resources.py holds it to 117)
    constexpr bool AHEAD = AHEAD_ && NC < 7;
    constexpr int V = TmGradSlots<NC>::count(ASYM);
    double g[TM_GSLOTS];
    double nu2[NC], hq[NC];
#pragma unroll
    for (int m = 0; m < NC; m++) { nu2[m] = sm->nu2[m]; hq[m] = sm->hq[m]; }
    const double g2 = sm->g2;
    const int imin = sm->imin, imax = sm->imax;
    const double aAh = ASYM ? 0.5 * sm->aA : 0.0, aB = ASYM ? sm->aB : 1.0, c2 = ASYM ? sm->c2 : 0.0;
#pragma unroll
    for (int s = 0; s < TM_GSLOTS; s++) g[s] = 0.0;
    if constexpr (AHEAD) {
        int ua = imin >> TM_UNIT_SHIFT, ub = (imax + TM_UNIT_BINS - 1) >> TM_UNIT_SHIFT;
        ua = ua > u0 ? ua : u0;
        ub = ub < u1 ? ub : u1;
        // TM_TAIL_APART: the grid's partial last unit -- one tile per chain has it -- is taken out of the pipelined range and
        // evaluated behind the loop with the in-place fetch (it is last in the order of summation either way), so that the
        // loop holds the whole-unit form of the loads alone
        constexpr bool APART = TM_TAIL_APART != 0;
        const int uw = Nx >> TM_UNIT_SHIFT;                       // whole units of the grid
        const bool tail = APART && ub > uw && ua <= uw;           // (then the range ends with unit uw, the partial one)
        if (APART && ub > uw) ub = uw;
        if (ua < ub) {
            double xc[2], wc[2];
            tm_grad_fetch<APART>(gx, s_w, ua, u0, Nx, tid, xc, wc);
            asm volatile("" : "+v"(xc[0]), "+v"(xc[1]), "+v"(wc[0]), "+v"(wc[1]));
            // two units per iteration, the two register sets swapping roles: no hand-over copies
            double xd[2], wd[2];
#pragma unroll 1
            for (int u = ua;;) {
                tm_grad_fetch<APART>(gx, s_w, u + 1 < ub ? u + 1 : u, u0, Nx, tid, xd, wd);
                {
                    const int lo = u << TM_UNIT_SHIFT, hi = lo + TM_UNIT_BINS;
                    tm_grad_unit_held<NC, ASYM>(nu2, hq, g2, aAh, aB, c2, imin, imax, xc, wc, lo, tid, Nx, !(lo >= imin && hi <= imax && hi <= Nx), g);
                }
                if (++u >= ub) break;
                tm_grad_fetch<APART>(gx, s_w, u + 1 < ub ? u + 1 : u, u0, Nx, tid, xc, wc);
                {
                    const int lo = u << TM_UNIT_SHIFT, hi = lo + TM_UNIT_BINS;
                    tm_grad_unit_held<NC, ASYM>(nu2, hq, g2, aAh, aB, c2, imin, imax, xd, wd, lo, tid, Nx, !(lo >= imin && hi <= imax && hi <= Nx), g);
                }
                if (++u >= ub) break;
            }
        }
        if (tail) tm_grad_unit<NC, ASYM>(nu2, hq, g2, aAh, aB, c2, imin, imax, gx, s_w + (uw - u0) * TM_UNIT_BINS + tid, (uw << TM_UNIT_SHIFT) + tid, Nx, true, g);
    } else {
#pragma unroll 1
        for (int u = u0; u < u1; u++) {
            // units that do not meet the window are skipped, units inside it need no test per bin (wave-uniform)
            const int lo = u << TM_UNIT_SHIFT, hi = lo + TM_UNIT_BINS;
            if (hi <= imin || lo >= imax) continue;
            const double *wq = s_w + (u - u0) * TM_UNIT_BINS + tid;
            tm_grad_unit<NC, ASYM>(nu2, hq, g2, aAh, aB, c2, imin, imax, gx, wq, lo + tid, Nx, !(lo >= imin && hi <= imax && hi <= Nx), g);
        }
    }
#if defined(TM_ABLATE) && (TM_ABLATE & 1)   // timing-only build: no wave reduction of the partials
    if (lane == 0) s_red_row[0] = g[0] + g[1] + g[2];
    return;
#endif
    // AHEAD: the lane index behind an empty asm, so that the butterfly's lane masks and the store slot of each shape are
    // made here, once per multiplet, instead of being hoisted in front of the multiplet loop -- eight shapes' worth of
    // them -- and, with the registers the look-ahead holds, spilled across it (9 VGPRs went to scratch without this)
    if constexpr (AHEAD) asm volatile("" : "+v"(lane));
    TmBfly<V, 32>::run(g, lane);
    // lanes whose plainly-reduced low bits are zero publish; padded slots are skipped
    constexpr int NSPLIT = (V > 16) ? 5 : (V > 8) ? 4 : (V > 4) ? 3 : (V > 2) ? 2 : 1;   // butterfly levels that split
    const int lowmask = (64 >> NSPLIT) - 1;
    bool valid = true;
    const int slot = TmBfly<V, 32>::slot_of(lane, valid);
    if ((lane & lowmask) == 0 && valid) {
        s_red_row[tm_grad_store_slot<NC>(slot)] = g[0];
    }
}

#ifndef TM_LB_FWD
#define TM_LB_FWD 4    // resident waves per SIMD the register allocator must allow (likelihood-only kernel)
#endif
#ifndef TM_LB_GRAD
#define TM_LB_GRAD 4   // same for the gradient kernel: 128 VGPRs (the pair loop is written to fit: see tm_eval_body)
#endif
// Look-ahead of pass 2 in the common-case gradient body (GRAD && !GEN; tm_grad_mult<.., AHEAD>): on by default;
// -DTM_LOOKAHEAD=0 builds the library without it for A/B runs (`make variant-la N=0`; profiles/README.md, "lookahead/").
// The generic bodies (GEN) sit at their register caps and do not take it.
#ifndef TM_LOOKAHEAD
#define TM_LOOKAHEAD 1
#endif
#ifdef TM_TRACE   // developer build: per-workgroup time stamps (tools/block_trace.py)
__device__ unsigned long long *g_tm_trace = nullptr;
#define TM_STAMP(slot) do { if (threadIdx.x == 0 && g_tm_trace) g_tm_trace[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + (slot)] = wall_clock64(); } while (0)
#else
#define TM_STAMP(slot) do { } while (0)
#endif

// a + b as one rounded addition, whatever produced b: kept out of FMA contraction, so that the sum of the weights is the
// same number in every copy of the group (beside a product in the same block the compiler would fuse the two)
#pragma clang fp contract(off)
__device__ __forceinline__ double tm_add_plain(double a, double b) { return a + b; }
#pragma clang fp contract(fast)

template <int N> struct TmInt { static constexpr int value = N; };
template <bool B> struct TmBool { static constexpr bool value = B; };

// What the background of a cell is made of (pass 1 of tm_eval_body): the cell's polynomial (the common case), exp per
// Harvey profile and bin where the polynomial is not valid (TmCellRec::npoly == 0), or white noise alone (nh == 0).
// TM_CK_ANY: not a kind -- the group decides at run time (generic kernels).
enum TmCellKind { TM_CK_POLY = 0, TM_CK_EXP = 1, TM_CK_NONE = 2, TM_CK_ANY = 3 };

// The workgroup's work for (chain, tile): pass 1 (model, likelihood partials, weights), in-launch finalize or pass 2.
// s_w: dynamic LDS for the weights, [TM_TILE_MAXU * TM_UNIT_BINS] doubles (GRAD only).  Called by tamcmc_eval_kernel
// (tamcmc_eval.hip) and by the fused small-grid kernel (tamcmc_fused.hip).
//
// The tile's units [u0, u1) (TmTileHdr, chosen per chain by the setup kernel) are walked in GROUPS of two units (four
// bins per thread share one fetch of a multiplet's record and one window test; four independent rational chains are in
// flight) -- a single unit where the tile ends on an odd unit or a group would straddle two cells.  A group that lies
// inside the grid takes the FULL path: no index clamps, no per-bin validity tests, loads at constant offsets from one
// per-thread pointer; within it a multiplet whose window covers the whole group takes the no-test form of
// tm_accum_mult.  Only the grid's last, partial unit takes the guarded path.
// A group is compiled for ONE kind of cell background (TmCellKind: polynomial, exp fallback, no Harvey profile); the walk
// picks the kind where it enters a cell (a gradient tile meets at most two cells), so the loops of the polynomial cells
// hold that variant alone -- see the walk below for the loops each kind gets.
// GEN = false: the common case compiled on its own -- chi(2,2p) likelihood, no Gaussian term (ids 0, 1), no model rows
// requested; the launcher picks it from the context (TmEvalArgs::generic).  Same arithmetic, fewer live scalars.
// GEN = true keeps the kind of the cell a run-time branch inside the group (TM_CK_ANY): see the walk.
template <bool GRAD, bool GEN = true>
__device__ __forceinline__ void tm_eval_body(const TmEvalArgs &a, const int chain, const int tile, double *s_w)
{
    const int like = GEN ? a.likelihood_case : 0;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    TmNoiseK sn = (TmNoiseK)(a.noise + chain);

#if defined(TM_ABLATE) && (TM_ABLATE & 16)   // timing-only build: empty workgroups (dispatch cost only)
    if (a.Nx > 0) return;
#endif
    __shared__ double s_red[2][TM_WAVES][TM_GSLOTS];   // likelihood-only kernels: the waves' partials ([0] alone is used)
    __shared__ double s_rows[TM_WAVES][TM_ROWS][TM_GSLOTS];   // gradient kernels: the waves' rows (TM_ROWS above)
    // (an instantiation refers to one of the two; the other is not allocated)

    // ---------------- prologue: nothing but scalar loads ----------------
    // Everything a tile needs -- its bounds, its list of active multiplets (table order), the cells' background
    // polynomials, the chain's noise record, the multiplet records themselves -- was prepared by the setup kernel and is
    // wave-uniform: it is fetched with s_load into SGPRs.  No LDS staging, no barrier before the first bin.
    // The chain's spectrum: contexts holding several spectra on one grid (ensembles, tamcmc_ctx_set_spectra) keep them
    // as consecutive blocks of Nx.
    const size_t spec_off = (a.spec != nullptr) ? (size_t)((TmIdxK)a.spec)[chain] * (size_t)a.Nx : 0;
    const double *__restrict__ yp = a.y + spec_off;
    const double *__restrict__ isp = a.isig2 + spec_off;      // dereferenced only when the likelihood is chi_square (then non-NULL)
    const TmMult *__restrict__ gm = a.mult + (size_t)chain * a.n_mult;
    TmTileHdrK th = (TmTileHdrK)(a.thdr + (size_t)chain * a.tiles + tile);
    const int u0 = th->u0;
    int u1 = th->u1;
    if (u1 - u0 > (GRAD ? TM_TILE_MAXU : TM_TILE_MAXU_L)) u1 = u0 + (GRAD ? TM_TILE_MAXU : TM_TILE_MAXU_L);      // the setup kernel never builds such a tile (and flags it if it did)
    const int nact = th->nact;
    TmCellRecK cells = (TmCellRecK)(a.cell + (size_t)chain * a.cells);
    TmActiveK tix = (TmActiveK)(a.tidx + ((size_t)chain * a.tiles + tile) * (a.n_mult > 0 ? a.n_mult : 1));
    const int nh = sn->nh;
    const bool has_gauss = GEN && sn->has_gauss != 0;
    const double N0 = sn->N0;
    const int row = (GEN && a.row_of_chain != nullptr) ? a.row_of_chain[chain] : -1;
    // FULL groups address the grid as (wave-uniform base pointer) + (32-bit per-thread bin index): global loads with a
    // scalar base and one VGPR of offset, instead of one 64-bit pointer per array and thread (Nx < 2^28 is checked at create)
    const double *__restrict__ xb = a.x2;
    const double *__restrict__ lb = a.lx;

#if defined(TM_ABLATE) && (TM_ABLATE & 32)   // timing-only build: prologue (scalar loads) only
    if (nact >= 0 && N0 == N0) { if (tid == 0 && !GRAD) a.part[((size_t)chain * a.tiles + tile) * 4] = (double)(nh + row + u0 + (has_gauss ? 1 : 0)); return; }
#endif
    // ---------------- pass 1: model spectrum and likelihood partial sums ----------------
    double S1 = 0.0;
    double P = 1.0;
    int esum = 0;
    int sgn = 0;                        // OR of the model values' high words: the sign bit tells whether any was negative
    double gn_[GRAD ? TM_GSLOTS : 1];   // GRAD: noise partial sums (3 per Harvey, sum w at slot 3*TM_MAXH, Gaussian at 13..15)
#pragma unroll
    for (int s_ = 0; s_ < (GRAD ? TM_GSLOTS : 1); s_++) gn_[s_] = 0.0;
    const double wscale = GRAD ? a.wt[2 * chain + 1] : 0.0;

    // one group of KG / 2 units starting at unit u, inside cell `tr`, whose background is of kind CK (TmCellKind): a
    // compile-time choice, so that a group holds ONE variant of the background code and of the noise sums (TM_CK_ANY:
    // both behind run-time branches, as the generic kernels keep them).  Bit 3 of kind_c marks a cold copy: no early loads.
    auto group = [&](auto kg_c, auto full_c, auto kind_c, const int u, TmCellRecK tr) __attribute__((always_inline)) {
        constexpr int KG = decltype(kg_c)::value;
        constexpr bool FULL = decltype(full_c)::value;
        constexpr int CK = decltype(kind_c)::value & 7;
        constexpr bool COLD = (decltype(kind_c)::value & 8) != 0;
        constexpr bool RT = CK == TM_CK_ANY;
        const bool HARVEY = RT ? nh > 0 : CK != TM_CK_NONE;     // the chain has Harvey profiles (nh > 0)
        const bool NPOLY = RT ? (nh > 0 && tr->npoly != 0) : CK == TM_CK_POLY;      // ... and this cell's polynomial is valid (TmCellRec::npoly)
        const int lo = u << TM_UNIT_SHIFT, hi = lo + KG * TM_THREADS;
        // cold copies: the profile count behind an empty asm, so that the `h < nh` masks of the fallback are made where
        // they are used instead of being hoisted in front of the cold loop and spilled across it
        int nhx = nh;
        if constexpr (COLD) asm volatile("" : "+s"(nhx));
        double x2[KG], acc[KG];
        int bi[KG];
#pragma unroll
        for (int k = 0; k < KG; k++) {
            const int i = lo + k * TM_THREADS + tid;
            if (FULL) {
                bi[k] = i;
                x2[k] = xb[(unsigned)i];
            } else {
                const bool valid = i < a.Nx;
                bi[k] = valid ? i : -1;
                x2[k] = a.x2[valid ? i : a.Nx - 1];
            }
            acc[k] = 0.0;
        }
        // likelihood-only kernel (registers to spare): log x and y are requested now, so that their latency passes
        // behind the multiplet loop instead of in front of the background / likelihood arithmetic
        constexpr bool EARLY = FULL && !GRAD && !COLD;
        double lxe[EARLY ? KG : 1], ye[EARLY ? KG : 1];
        if constexpr (EARLY) {
#pragma unroll
            for (int k = 0; k < KG; k++) { lxe[k] = HARVEY ? lb[(unsigned)bi[k]] : 0.0; ye[k] = yp[(unsigned)bi[k]]; }
        }
        if constexpr (GRAD) {
            for (int jj = 0; jj < nact; jj++) {
                const int idx = tix[jj].idx, imin = tix[jj].imin, imax = tix[jj].imax, shape = tix[jj].shape;
                if (hi <= imin || lo >= imax) continue;   // wave-uniform skip
                tm_accum_dispatch<KG>((TmMultK)(gm + idx), shape, x2, bi, acc, !(FULL && lo >= imin && hi <= imax));
            }
        } else if (nact > 0) {
            // Likelihood kernel (SGPRs to spare): the list entry of the NEXT multiplet is requested before the current one
            // is evaluated (one 16-byte scalar load, in flight beside the record's), so a wave waits once per multiplet
            // instead of three times in a row (window; index and shape; record) -- waits that a wave with few
            // neighbours on its SIMD cannot hide (the tail of a launch).  (The common-case gradient kernel has the SGPRs for
            // it since the cell-kind split; there it measured 0.5 - 0.9 us slower, in pass 2 no different: profiles/README.md,
            // "lookahead/".)
            TmEntry e = tm_load_entry(tix);
            asm volatile("" :: "s"(e.x));             // a use: the first entry is waited for here, not inside the loop
            for (int jj = 0; jj < nact; jj++) {
                const TmEntry en = tm_load_entry(tix + (jj + 1 < nact ? jj + 1 : jj));
                const int idx = e.x, imin = e.y, imax = e.z, shape = e.w;
                if (!(hi <= imin || lo >= imax))   // wave-uniform skip
                    tm_accum_dispatch<KG>((TmMultK)(gm + idx), shape, x2, bi, acc, !(FULL && lo >= imin && hi <= imax));
                e = en;
            }
        }

        // background, likelihood and (GRAD) weights + noise partial sums, KH bins at a time: the gradient kernel keeps
        // three accumulators per component in pass 2 and sixteen noise sums here, so it takes the four bins of a group
        // in two halves (fewer values live at once: 4 waves per SIMD instead of 3)
        constexpr int KH = GRAD ? 2 : KG;
#pragma unroll
        for (int h0 = 0; h0 < KG; h0 += KH) {
        double hu[TM_MAXH][GRAD ? KH : 1], harg[GRAD ? KH : 1];   // GRAD: u = 1/(1+t) per Harvey and bin (t u = 1 - u), log x per bin
        const bool n0_done = NPOLY;                           // the polynomial's constant term holds N0
        if (HARVEY) {
            double dl[KH];
#pragma unroll
            for (int k = 0; k < KH; k++) {
#if defined(TM_ABLATE) && (TM_ABLATE & 128)   // timing-only build: no log x load (wrong values)
                dl[k] = tr->lxc + 1e-9 * x2[h0 + k];
#else
                dl[k] = EARLY ? lxe[h0 + k] : FULL ? lb[(unsigned)bi[h0 + k]] : a.lx[bi[h0 + k] >= 0 ? bi[h0 + k] : a.Nx - 1];
#endif
                if constexpr (GRAD) harg[k] = dl[k];
            }
            if (NPOLY) {
                const double lxc = tr->lxc;
                // whole background (all profiles + white noise) as ONE polynomial: 8 FMAs per bin.  The gradient path
                // accumulates the moments sum w dl^j instead of per-profile sums (below); the backward kernel turns
                // them into the per-profile sums with each profile's own series coefficients.
#pragma unroll
                for (int k = 0; k < KH; k++) { dl[k] -= lxc; acc[h0 + k] += tm_poly(tr, dl[k]); if constexpr (GRAD) harg[k] = dl[k]; }
            } else {
#pragma unroll
                for (int h = 0; h < TM_MAXH; h++) {
                    if (h < nhx) {
                        const double Hh = sn->H[h], ph = sn->p[h], lth = sn->lt[h];
#pragma unroll
                        for (int k = 0; k < KH; k++) {
                            const double t = exp(ph * (lth + dl[k]));
                            const double uu = 1.0 / (t + 1.0);
                            acc[h0 + k] += Hh * uu;
                            if constexpr (GRAD) hu[h][k] = uu;
                        }
                    }
                }
            }
        }
        if (has_gauss) {
            const double gA = sn->gA, gnu0 = sn->gnu0, gs2 = sn->gs2;
#pragma unroll
            for (int k = 0; k < KH; k++) {
                const double dd = 0.5 * x2[h0 + k] - gnu0;
                acc[h0 + k] = gA * exp((-0.5 * (dd * dd)) / gs2) + acc[h0 + k];
            }
        }
        if (!n0_done) {
#pragma unroll
            for (int k = 0; k < KH; k++) acc[h0 + k] += N0;
        }
        if (row >= 0) {
#pragma unroll
            for (int k = 0; k < KH; k++)
                if (FULL || bi[h0 + k] >= 0) a.model_out[(size_t)row * a.Nx + (size_t)(lo + (h0 + k) * TM_THREADS + tid)] = acc[h0 + k];
        }

        double wreg[GRAD ? KH : 1];
        if (like == 0) {
            // -p * (sum y/M + sum log M), likelihoods.cpp:23-25
#pragma unroll
            for (int k = 0; k < KH; k++) {
                double wv = 0.0;
                if (FULL || bi[h0 + k] >= 0) {
                    // A model value that is NaN, +-inf or 0 turns rM (and so S1) into NaN by itself (v_rcp_f64 + the
                    // Newton steps); a negative one is caught by the sign bits collected in sgn.  Either way logL
                    // becomes NaN, which is what log() of such a value gives the reference.
                    const double M = acc[h0 + k];
                    const double yv = EARLY ? ye[h0 + k] : FULL ? yp[(unsigned)bi[h0 + k]] : yp[bi[h0 + k]];
                    sgn |= __double2hiint(M);
                    const double rM = tm_rcp(M);
                    S1 = __builtin_fma(yv, rM, S1);
                    int e;
                    P *= frexp(M, &e);
                    esum += e;
                    wv = wscale * (yv * rM * rM - rM);   // d(logL/T)/dM_i
                }
                if constexpr (GRAD) wreg[k] = wv;
            }
            {
                int e;
                P = frexp(P, &e);   // keep the running mantissa product in [0.5, 1)
                esum += e;
            }
        } else {
            // -sum (y-M)^2 / sigma^2, likelihoods.cpp:36
#pragma unroll
            for (int k = 0; k < KH; k++) {
                double wv = 0.0;
                if (FULL || bi[h0 + k] >= 0) {
                    const int i = lo + (h0 + k) * TM_THREADS + tid;
                    const double dd = yp[i] - acc[h0 + k];
                    const double is2 = isp[i];
                    S1 = __builtin_fma(dd * dd, is2, S1);
                    wv = wscale * dd * is2;
                }
                if constexpr (GRAD) wreg[k] = wv;
            }
        }
        if constexpr (GRAD) {
            // weights for pass 2 (each thread re-reads only its own entries) and the noise partial sums, reusing u and
            // t*u of these bins (no second pass over the bins)
#pragma unroll
            for (int k = 0; k < KH; k++) {
                const double wk = wreg[k];
                s_w[((u - u0) * 2 + h0 + k) * TM_THREADS + tid] = wk;
                gn_[3 * TM_MAXH] = tm_add_plain(gn_[3 * TM_MAXH], wk);
#if defined(TM_ABLATE) && (TM_ABLATE & 512)   // timing-only build: no weight moments
                if (false) {
#else
                if (NPOLY) {
#endif
                    // moments of the weights about the cell centre: slot j-1 <- sum w dl^j, j = 1..TM_HSER-1
                    // (each power is rounded for the next one, and added fused: w dl^j = fma(dl, w dl^(j-1), sum))
                    double q = wk;
#pragma unroll
                    for (int j = 0; j < TM_HSER - 1; j++) { gn_[j] = __builtin_fma(harg[k], q, gn_[j]); q *= harg[k]; }
                } else if (HARVEY) {
#pragma unroll
                    for (int h = 0; h < TM_MAXH; h++) {
                        if (h < nhx) {
                            const double wu = wk * hu[h][k];
                            const double tu2 = wu * (1.0 - hu[h][k]);   // t u = 1 - u
                            gn_[3 * h] = __builtin_fma(wk, hu[h][k], gn_[3 * h]);
                            gn_[3 * h + 1] = __builtin_fma(wu, 1.0 - hu[h][k], gn_[3 * h + 1]);
                            gn_[3 * h + 2] = __builtin_fma(tu2, sn->lt[h] + harg[k], gn_[3 * h + 2]);
                        }
                    }
                }
                if (has_gauss) {
                    // Gaussian term: sum w e, sum w e d, sum w e d^2 with e = exp(-0.5 d^2/s2), d = x - nu0
                    const double dd = 0.5 * x2[h0 + k] - sn->gnu0;
                    const double we = wk * exp((-0.5 * (dd * dd)) / sn->gs2);
                    gn_[13] += we;
                    gn_[14] = __builtin_fma(we, dd, gn_[14]);
                    gn_[15] = __builtin_fma(we * dd, dd, gn_[15]);
                }
            }
        }
        if constexpr (GRAD) __builtin_amdgcn_sched_barrier(0);   // keep the halves apart: interleaved they need 40 more registers
        }   // halves of the group
    };

    // GRAD: the noise partial sums of the cell just finished -> the wave's row 1 + part; the flush behind pass 2 adds the
    // four waves and stores gnoise[chain][tile][part].  No barrier: the row is this wave's own and is written once.
    auto flush_noise = [&](const int part, auto cold_c) __attribute__((always_inline)) {
        if constexpr (GRAD) {
            // the cold loop's copy: the lane index behind an empty asm, so that its lane masks are made here, once
            // per flush, instead of being hoisted in front of that loop and spilled across it (8 SGPRs)
            int ln = lane;
            if constexpr (decltype(cold_c)::value) asm volatile("" : "+v"(ln));
            static_assert(TM_NSLOTS == 16, "butterfly below assumes 16 noise slots");
            TmBfly<TM_NSLOTS, 32>::run(gn_, ln);
            bool valid = true;
            const int slot = TmBfly<TM_NSLOTS, 32>::slot_of(ln, valid);
            double *red = s_rows[wave][1 + part];
            if ((ln & 3) == 0) red[slot] = gn_[0];
            TM_TILE_SYNC();
            TM_TILE_SYNC();
#pragma unroll
            for (int s_ = 0; s_ < TM_GSLOTS; s_++) gn_[s_] = 0.0;
        }
    };

    {
        // The walk over the tile's units, cell by cell: the part [u, ue) of the tile that lies in one cell has one kind of
        // background (TmCellKind), chosen where the walk enters the cell.  Within it the hot loop is the run of PAIRS (two
        // units: four bins per thread), aligned to even units; cells begin on even units, so a pair never straddles two
        // cells and the groups are those of one walk over the whole tile.  An odd first unit is taken alone before the
        // pair loop; what is left after it -- an odd last unit, and at the end of the grid the partial unit -- alone
        // after it.  A loop holds ONE variant of the group: a second one behind a branch in the same loop costs registers
        // in copies where the two meet (~40 for the pair code; 9 copies of noise sums per bin for the two backgrounds).
        auto walk = [&](auto kind_c, int u, const int ue, TmCellRecK tr) __attribute__((always_inline)) {
            if ((u & 1) && u < ue && ((u + 1) << TM_UNIT_SHIFT) <= a.Nx) { group(TmInt<2>(), TmBool<true>(), kind_c, u, tr); u += 1; }
#pragma unroll 1
            for (; u + 2 <= ue && ((u + 2) << TM_UNIT_SHIFT) <= a.Nx; u += 2) group(TmInt<4>(), TmBool<true>(), kind_c, u, tr);
#pragma unroll 1
            for (; u < ue; u += 1) {
                if (((u + 1) << TM_UNIT_SHIFT) <= a.Nx) group(TmInt<2>(), TmBool<true>(), kind_c, u, tr);
                else                                    group(TmInt<2>(), TmBool<false>(), kind_c, u, tr);
            }
        };
        // the same units one at a time (cold cells): a pair is its two units in turn -- the same sums in the same order,
        // the mantissa product rescaled (exactly: by powers of two) twice as often
        auto walk_single = [&](auto kind_c, int u, const int ue, TmCellRecK tr) __attribute__((always_inline)) {
#pragma unroll 1
            for (; u < ue; u += 1) {
                if (((u + 1) << TM_UNIT_SHIFT) <= a.Nx) group(TmInt<2>(), TmBool<true>(), kind_c, u, tr);
                else                                    group(TmInt<2>(), TmBool<false>(), kind_c, u, tr);
            }
        };
        const int cell0 = u0 >> TM_CELL_SHIFT;
        int ce = cell0;
        int u = u0;
#if defined(TM_ABLATE) && (TM_ABLATE & 256)   // timing-only build: no pass 1
        u = u1;
#endif
        if constexpr (GEN) {
            // The generic kernels sit at their register budgets (128 / 72 VGPRs) with one copy of the three loops and have
            // no room for a second, nor for a loop over the cells around them: they walk the tile in one go and keep the
            // kind a run-time branch inside the group (TM_CK_ANY).
            int cur_cell = cell0;
            auto cell_of = [&](const int uu) __attribute__((always_inline)) {
                const int c = uu >> TM_CELL_SHIFT;
                if (GRAD && c != cur_cell) { flush_noise(0, TmBool<false>()); cur_cell = c; }   // at most once per tile (TM_TILE_MAXU <= TM_CELL_UNITS)
                return cells + c;
            };
            if ((u & 1) && u < u1 && ((u + 1) << TM_UNIT_SHIFT) <= a.Nx) { TmCellRecK tr = cell_of(u); group(TmInt<2>(), TmBool<true>(), TmInt<TM_CK_ANY>(), u, tr); u += 1; }
#pragma unroll 1
            for (; u + 2 <= u1 && ((u + 2) << TM_UNIT_SHIFT) <= a.Nx; u += 2) { TmCellRecK tr = cell_of(u); group(TmInt<4>(), TmBool<true>(), TmInt<TM_CK_ANY>(), u, tr); }
#pragma unroll 1
            for (; u < u1; u += 1) {
                TmCellRecK tr = cell_of(u);
                if (((u + 1) << TM_UNIT_SHIFT) <= a.Nx) group(TmInt<2>(), TmBool<true>(), TmInt<TM_CK_ANY>(), u, tr);
                else                                    group(TmInt<2>(), TmBool<false>(), TmInt<TM_CK_ANY>(), u, tr);
            }
            ce = cur_cell + 1;
        } else {
            // The polynomial cells at the head of the tile -- in the common case all of it -- in a loop of their own,
            // with the three loops of `walk`: neither the exp fallback nor a branch on the kind is in it, none of the
            // fallback's scalars (sn->H/p/lt, the constants of exp) is live in it, and acc[] and the noise sums are
            // updated in place.
#pragma unroll 1
            for (; u < u1; ce++) {
                TmCellRecK tr = cells + ce;
                if (nh <= 0 || tr->npoly == 0) break;
                if (GRAD && ce != cell0) flush_noise(0, TmBool<false>());
                const int cend = (ce + 1) << TM_CELL_SHIFT;
                const int ue = cend < u1 ? cend : u1;
                walk(TmInt<TM_CK_POLY>(), u, ue, tr);
                u = ue;
            }
            // From the first cell of another kind to the end of the tile (cold): every kind, each with its own loop, one
            // unit at a time and without the early loads.  With pair loops as well these copies took the gradient
            // kernel to 128 VGPRs plus 2 spilled and the likelihood kernel to 75.
#pragma unroll 1
            for (; u < u1; ce++) {
                TmCellRecK tr = cells + ce;
                if (GRAD && ce != cell0) flush_noise(0, TmBool<true>());
                const int cend = (ce + 1) << TM_CELL_SHIFT;
                const int ue = cend < u1 ? cend : u1;
                if (nh <= 0)             walk_single(TmInt<8 + TM_CK_NONE>(), u, ue, tr);
                else if (tr->npoly != 0) walk_single(TmInt<8 + TM_CK_POLY>(), u, ue, tr);
                else                     walk_single(TmInt<8 + TM_CK_EXP>(), u, ue, tr);
                u = ue;
            }
        }
        if (GRAD) flush_noise(ce > cell0 + 1 ? 1 : 0, TmBool<false>());   // the part of the tile's last cell
    }
    TM_STAMP(1);
    // tile partials: S1 = sum y/M (or the chi-square sum), and sum log M as (mantissa product, exponent sum)
    double Pm = 1.0, Pe = 0.0;
    if (like == 0) {
        int e;
        Pm = frexp(tm_wave_prod(P), &e);
        Pe = tm_wave_sum((double)esum) + (double)e;
        if (__builtin_amdgcn_ballot_w64(sgn < 0) != 0) Pm = __builtin_nan("");     // a negative model value anywhere: log -> NaN
    }
    S1 = tm_wave_sum(S1);
    if constexpr (!GRAD) {
        if (lane == 0) { s_red[0][wave][0] = S1; s_red[0][wave][1] = Pm; s_red[0][wave][2] = Pe; }
        __syncthreads();
    }
    if constexpr (GRAD) {
        // the wave's row 0, no barrier; the flush behind pass 2 combines the four waves into part[]
        if (lane == 0) { s_rows[wave][0][0] = S1; s_rows[wave][0][1] = Pm; s_rows[wave][0][2] = Pe; }
        TM_TILE_SYNC();
    } else if (wave == 0) {
        // Finalize inside this launch: the workgroup that publishes the LAST tile partial of a chain sums all of them
        // in a fixed order (lane-strided, then a wave tree), so the result does not depend on which workgroup that is.
        // Hand-off without cache-wide fences: the partials are written and read with agent-scope relaxed atomics, which
        // on gfx942 / gfx950 compile to global_store / global_load with sc1 (write-through to, and read from, the
        // device-coherent level past the per-XCD L2s); the publisher drains its stores (s_waitcnt vmcnt(0)) before it
        // takes its ticket (an agent-scope atomic add, executed at that same level), and the last arriver reads only
        // after its ticket returned.  This is NOT the HIP memory model's release / acquire (no fence instructions: those
        // cost 18 us per launch here); it relies on these gfx9 properties, and tests/test_parity_gpu.py
        // (test_launch_order_does_not_change_results, run-to-run bitwise equality) is its guard.
        int last = 0;
        double *pp = a.part + (size_t)chain * a.tiles * 4;
        if (lane == 0) {
            double t1 = 0.0, tm = 1.0, te = 0.0;
#pragma unroll
            for (int wv = 0; wv < TM_WAVES; wv++) { t1 += s_red[0][wv][0]; tm *= s_red[0][wv][1]; te += s_red[0][wv][2]; }
#if defined(TM_ABLATE) && (TM_ABLATE & 4)    // timing-only build: plain stores, no ticket, no finalize
            pp[4 * tile] = t1; pp[4 * tile + 1] = tm; pp[4 * tile + 2] = te;
#else
            if (a.tiles == 1) {
                // the chain's only tile: nothing to hand over.  Same value as the general path below, without its
                // store-drain-ticket-reload round trip
                pp[0] = t1; pp[1] = tm; pp[2] = te;
                const double t2 = (like == 0) ? tm_tile_logsum(tm, te) : 0.0;
                double f = (like == 0) ? -a.like_p * (t1 + t2) : -t1;
                f = f / a.wt[2 * chain];
                int st = a.noise[chain].status;
                if (st != 0) f = __builtin_nan("");
                else if (!(f == f)) st = 1;
                a.logL[chain] = f;
                if (a.status) a.status[chain] = st;
            } else {
            __hip_atomic_store(pp + 4 * tile, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(pp + 4 * tile + 1, tm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(pp + 4 * tile + 2, te, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const int prev = __hip_atomic_fetch_add(a.ticket + chain, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = (prev == a.tiles - 1) ? 1 : 0;
            }
#endif
        }
        last = __shfl(last, 0, 64);
        if (last) {
            double s1 = 0.0, s2 = 0.0;
            for (int t = lane; t < a.tiles; t += 64) {
                s1 += __hip_atomic_load(pp + 4 * t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (like == 0)
                    s2 += tm_tile_logsum(__hip_atomic_load(pp + 4 * t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                                         __hip_atomic_load(pp + 4 * t + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
            s1 = tm_wave_sum(s1);
            s2 = tm_wave_sum(s2);
            if (lane == 0) {
                double f = (like == 0) ? -a.like_p * (s1 + s2) : -s1;
                f = f / a.wt[2 * chain];
                int st = a.noise[chain].status;
                if (st != 0) f = __builtin_nan("");
                else if (!(f == f)) st = 1;
                a.logL[chain] = f;
                if (a.status) a.status[chain] = st;
                __hip_atomic_store(a.ticket + chain, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm
            }
        }
    }

    TM_STAMP(2);
#ifdef TM_TRACE
    if (threadIdx.x == 0 && g_tm_trace) {
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g_tm_trace[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + 3] = ((unsigned long long)xcc << 32) | hw;
    }
#endif
    // ---------------- pass 2: gradient partial sums ----------------
    if constexpr (GRAD) {
        constexpr bool AHEAD = !GEN && TM_LOOKAHEAD != 0;     // tm_grad_mult: x and the weights of the next unit ahead of use
        // No barrier in front of pass 2: a thread reads only its own entries of s_w, and rows 0..2 are not written again.
        // The waves run decoupled through the active list, TM_ROW_K multiplets at a time, each into its own rows; the
        // workgroup meets once per chunk -- in the common case (nact <= TM_ROW_K) once per tile -- at the flush below.
        TM_TILE_SYNC();
#if defined(TM_ABLATE) && (TM_ABLATE & 2)   // timing-only build: no multiplet pass 2 at all
        const int nrun = 0;
#else
        const int nrun = nact;
#endif
#pragma unroll 1
        for (int base = 0;; base += TM_ROW_K) {
            const int nrow = nrun - base < TM_ROW_K ? nrun - base : TM_ROW_K;      // multiplets of this chunk
            const bool last = base + TM_ROW_K >= nrun;
#pragma unroll 1
            for (int j = 0; j < nrow; j++) {
                const int jj = base + j;
                const int idx = tix[jj].idx, shape = tix[jj].shape;
                TmMultK sm = (TmMultK)(gm + idx);
                double *red = s_rows[wave][3 + j];
                switch (shape) {
                case 1: tm_grad_mult<1, false, AHEAD>(sm, a.x2, s_w, u0, u1, a.Nx, tid, lane, red); break;
                case 3: tm_grad_mult<3, false, AHEAD>(sm, a.x2, s_w, u0, u1, a.Nx, tid, lane, red); break;
                case 5: tm_grad_mult<5, false, AHEAD>(sm, a.x2, s_w, u0, u1, a.Nx, tid, lane, red); break;
                case 7: tm_grad_mult<7, false, AHEAD>(sm, a.x2, s_w, u0, u1, a.Nx, tid, lane, red); break;
                case 256 + 1: tm_grad_mult<1, true, AHEAD>(sm, a.x2, s_w, u0, u1, a.Nx, tid, lane, red); break;
                case 256 + 3: tm_grad_mult<3, true, AHEAD>(sm, a.x2, s_w, u0, u1, a.Nx, tid, lane, red); break;
                case 256 + 5: tm_grad_mult<5, true, AHEAD>(sm, a.x2, s_w, u0, u1, a.Nx, tid, lane, red); break;
                default: tm_grad_mult<7, true, AHEAD>(sm, a.x2, s_w, u0, u1, a.Nx, tid, lane, red); break;
                }
                TM_TILE_SYNC();
            }
            // The flush: thread t takes row t / TM_GSLOTS, slot t % TM_GSLOTS, adds the four waves in the order 0, 1, 2, 3 and
            // stores the total: here the chunk's gmult rows.  A slot the multiplet's shape does not write
            // (tm_grad_store_slot) is stored as zero and never read from LDS, so nothing has to clear a row before it is reused.
#if !(defined(TM_ABLATE) && (TM_ABLATE & 64))   // (bit 64, timing-only build: no flush barrier)
            __syncthreads();
#endif
            const int r = tid / TM_GSLOTS, s = tid - r * TM_GSLOTS;
            if (r >= 3 && r - 3 < nrow) {
                const int idx = tix[base + r - 3].idx, shape = tix[base + r - 3].shape;
                const int nc = shape & 255;
                double t = 0.0;
                if (s < nc || (s >= 7 && s <= 7 + ((nc - 1) >> 1)) || s == 11 || (s >= 21 && shape >= 256)) {      // B_k, A_am, C, asymmetry sums
#pragma unroll
                    for (int wv = 0; wv < TM_WAVES; wv++) t += s_rows[wv][r][s];
                }
                a.gmult[(((size_t)chain * a.tiles + tile) * a.n_mult + idx) * TM_GSLOTS + s] = t;
            }
            if (last) break;
            __syncthreads();   // the rows are free again: only tiles with nact > TM_ROW_K come here
        }
        // Behind the last chunk's barrier rows 0..2 of every wave are complete as well: the likelihood triple (a product for
        // the mantissas) -> part[], summed by the backward kernel, and the noise sums of the cells the tile met -> gnoise.
        // Kept behind the chunk loop, not in it: inside, the generic kernel spilled ten more SGPRs.
        {
            const int r = tid / TM_GSLOTS, s = tid - r * TM_GSLOTS;
            const size_t ct = (size_t)chain * a.tiles + tile;
            if (r == 0) {
                if (s < 3) {
                    double t = (s == 1) ? 1.0 : 0.0;
#pragma unroll
                    for (int wv = 0; wv < TM_WAVES; wv++) { const double v = s_rows[wv][0][s]; t = (s == 1) ? t * v : t + v; }
                    a.part[ct * 4 + s] = t;
                }
            } else if (r < 3 && s < TM_NSLOTS && (r == 1 || ((u1 - 1) >> TM_CELL_SHIFT) > (u0 >> TM_CELL_SHIFT))) {
                // part 1 exists where the tile's last unit lies in another cell than its first (a tile meets at most two)
                double t = 0.0;
#pragma unroll
                for (int wv = 0; wv < TM_WAVES; wv++) t += s_rows[wv][r][s];
                a.gnoise[(ct * 2 + (r - 1)) * TM_NSLOTS + s] = t;
            }
        }
        TM_STAMP(2);   // gradient kernel: slot 2 = end of pass 2
    }
}

#endif
