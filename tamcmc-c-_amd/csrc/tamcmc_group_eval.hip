// tamcmc_group_eval.hip -- the likelihood launch of a fit group (tamcmc_group.h): a 1-D grid over sum_k Nchains_k x
// tiles_k workgroups, member-major.  Workgroup -> member by a scalar search over the prefix of workgroup counts, then
// (chain, tile) by exactly the rules tamcmc_eval_kernel applies to that member's own 2-D grid (order_mode / order[] /
// prio), then tm_eval_body with the member's TmEvalArgs.  Compiled with the flags of tamcmc_eval.o, so a chain's
// partial sums, finalize and logL are those of its context's own launch bit for bit.  Generic members (chi_square,
// ids 0 / 1) go to the GEN = true instance in a launch of their own, as the solo launcher picks that body for them.
#include <hip/hip_runtime.h>
#include "tamcmc_dev.h"
#include "tamcmc_eval_body.h"
#include "tamcmc_group.h"

template <bool GEN>
__global__ __launch_bounds__(TM_THREADS, TM_LB_FWD) void tamcmc_group_eval_kernel(const TmEvalArgs *desc, const int32_t *pre,
                                                                                 const int32_t *nch, int n)
{
    typedef const __attribute__((address_space(4))) int32_t *K;
    const int k = tm_group_member(pre, n, (int)blockIdx.x);
    const unsigned w = (unsigned)((int)blockIdx.x - ((K)pre)[k]);      // workgroup within the member's launch
    const unsigned nc = (unsigned)((K)nch)[k];
    const TmEvalArgs &a = tm_group_desc(desc, k);
    // the member's 2-D grid, linearised as the hardware numbers it: (tiles, Nchains) for order_mode 0, else (Nchains, tiles)
    int chain, tile, rank;
    if (a.order_mode == 0) {
        const unsigned t = (unsigned)a.tiles;
        chain = (int)(w / t);
        const int slot = (int)(w - (unsigned)chain * t);
        const unsigned rn = (unsigned)((a.tiles - 1) & 7) * (unsigned)(chain & 0xffff);
        const unsigned rq = (unsigned)(((unsigned long long)rn * a.tile_magic) >> 40);
        tile = slot + (int)(rn - rq * (unsigned)a.tiles);
        if (tile >= a.tiles) tile -= a.tiles;
        rank = slot;
    } else {
        rank = (int)(w / nc);
        chain = (int)(w - (unsigned)rank * nc);
        tile = (a.order_mode == 2) ? a.order[(size_t)chain * a.tiles + rank] : rank;
    }
    // (the divisions above are expanded into vector instructions: without these the compiler would treat chain and tile
    // as per-lane values and fetch the records through vector loads instead of scalar ones)
    chain = __builtin_amdgcn_readfirstlane(chain);
    tile = __builtin_amdgcn_readfirstlane(tile);
    rank = __builtin_amdgcn_readfirstlane(rank);
    if (a.order_mode != 0 && a.prio == 1) {
        const int r4 = (4 * rank) / a.tiles;
        if (r4 == 0) __builtin_amdgcn_s_setprio(3); else if (r4 == 1) __builtin_amdgcn_s_setprio(2); else if (r4 == 2) __builtin_amdgcn_s_setprio(1);
    }
    extern __shared__ double s_dyn[];
    tm_eval_body<false, GEN>(a, chain, tile, s_dyn);
}

int tm_launch_group_eval(const TmEvalArgs *d_desc, const int32_t *d_pre, const int32_t *d_nch, int n, int total, bool generic,
                         void *stream_)
{
    if (n < 1 || total < 1) return (int)hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    if (generic) hipLaunchKernelGGL((tamcmc_group_eval_kernel<true>), dim3(total), dim3(TM_THREADS), 8, stream, d_desc, d_pre, d_nch, n);
    else         hipLaunchKernelGGL((tamcmc_group_eval_kernel<false>), dim3(total), dim3(TM_THREADS), 8, stream, d_desc, d_pre, d_nch, n);
    return (int)hipGetLastError();
}
