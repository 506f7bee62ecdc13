// tamcmc_group.h -- fit groups (tamcmc_group_* in include/tamcmc_accel.h): the chains of several contexts -- different
// grids, model ids, parameter layouts -- evaluated by ONE launch per kernel kind instead of one launch per context.
//
// The solo kernels map a workgroup to (chain, tile) of one context; the grouped kernels (tamcmc_group_setup.hip,
// tamcmc_group_eval.hip, tamcmc_group_fused.hip) map it to (member, chain, tile) and then call the same bodies with that
// member's arguments.  The member comes from a scalar binary search over a prefix table of workgroup counts; its
// arguments come from a descriptor table in device memory, read through the constant address space (scalar loads into
// SGPRs, as kernel arguments are).  A chain thus runs the same code on the same data with the same tile geometry as when
// its context is evaluated alone, and gets the same bits.
//
// Device table of a call (one allocation, written by one host-to-device copy when it changes):
//   [n_setup + 1] int32 prefix of chains, [n_setup] TmGroupSetup           non-fused members, setup launch
//   [n_fused + 1] int32 prefix of chains, [n_fused] TmGroupFused           one-tile members, setup + eval in one launch
//   [n_spec + 1]  int32 prefix of workgroups, [n_spec] chains, [n_spec] TmEvalArgs   specialised likelihood members
//   [n_gen + 1]   int32 prefix of workgroups, [n_gen] chains, [n_gen] TmEvalArgs      generic members (chi_square, ids 0 / 1)
// (each array at a 256-byte boundary; the launches run in this order)
#pragma once
#include "tamcmc_dev.h"

#ifndef TM_SETUP_THREADS
#define TM_SETUP_THREADS 512      // as tamcmc_setup.hip
#endif
#define TM_GROUP_MAX_MEMBERS 1024 // members of one group at most (TAMCMC_GROUP_MAX_MEMBERS, tamcmc_group_create)

// Arguments of tamcmc_setup_kernel for one member (likelihood path: no gradient records).
struct TmGroupSetup {
    TmLayout L;
    const double *params, *Tcoefs;
    double *wt;
    const double *lx;
    TmMult *mult;
    TmNoise *noise;
    TmCellRec *cell;
    TmTileHdr *thdr;
    TmActive *tidx;
    int32_t *order;               // NULL unless the member's eval launch ranks its tiles (order_mode 2)
    TmCostModel cm;
    int32_t units, cells, tiles, eq;   // eq: the balancer flag (tm_setup_balances)
    int32_t p_doubles, pad;
};

// Arguments of tamcmc_fused_kernel for one member.
struct TmGroupFused {
    TmLayout L;
    TmFusedArgs f;
    TmEvalArgs a;
};

static_assert(sizeof(TmGroupSetup) % 8 == 0 && sizeof(TmGroupFused) % 8 == 0 && sizeof(TmEvalArgs) % 8 == 0,
              "descriptors are loaded as 8-byte words");

#if defined(__HIPCC__)
// Largest k < n with pre[k] <= b (pre[0] = 0 <= b < pre[n]): the member that owns workgroup b.  Scalar: b is uniform.
__device__ __forceinline__ int tm_group_member(const int32_t *pre, int n, int b)
{
    typedef const __attribute__((address_space(4))) int32_t *K;
    const K p = (K)pre;
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// A member's descriptor as the bodies take it (by reference): a generic pointer cast from the constant address space.
// Address-space inference turns every field access back into a constant-address-space load at its point of use -- a
// scalar load, issued where the body needs the field, as for a kernel argument -- instead of one copy of the whole
// record up front (which would not fit in the SGPRs next to the bodies' own scalars).
template <typename T>
__device__ __forceinline__ const T &tm_group_desc(const T *tab, int k)
{
    typedef const __attribute__((address_space(4))) T *K;
    return *(const T *)((K)tab + k);
}
#endif

#ifdef __cplusplus
extern "C++" {
// launchers (tamcmc_group_*.hip); n members with pre[n] workgroups, lds = dynamic LDS bytes (the largest member's need)
int tm_launch_group_setup(const TmGroupSetup *d_desc, const int32_t *d_pre, int n, int total, size_t lds, void *stream);
int tm_launch_group_eval(const TmEvalArgs *d_desc, const int32_t *d_pre, const int32_t *d_nch, int n, int total, bool generic,
                         void *stream);
int tm_launch_group_fused(const TmGroupFused *d_desc, const int32_t *d_pre, int n, int total, size_t lds, void *stream);
}
#endif
