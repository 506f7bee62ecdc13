// tamcmc_group_fused.hip -- the one-tile members of a fit group (tamcmc_group.h) in ONE launch: workgroup b runs the
// prologue and the evaluation of one chain of the member that owns it, exactly as tamcmc_fused_kernel does for a context
// alone (the slices of a local fit: 8 members x 10 chains are one launch of 80 workgroups instead of 8 launches).
// Visibility protocol of tamcmc_fused.hip, unchanged: the records written by the prologue are fenced, the workgroup
// meets at a barrier, the scalar cache is invalidated, and the record pointers reach the eval body through an opaque
// move, so that no constant-address-space load of a record is scheduled ahead of the barrier.
#include <hip/hip_runtime.h>
#include "tamcmc_dev.h"
#include "tamcmc_setup_body.h"
#include "tamcmc_eval_body.h"
#include "tamcmc_group.h"

__global__ __launch_bounds__(TM_THREADS) void tamcmc_group_fused_kernel(const TmGroupFused *desc, const int32_t *pre, int n)
{
    extern __shared__ double s_dyn[];   // [f.p_doubles] this chain's params row, then the eval body's slot
    const int k = tm_group_member(pre, n, (int)blockIdx.x);
    const int chain = (int)blockIdx.x - ((const __attribute__((address_space(4))) int32_t *)pre)[k];
    const TmGroupFused &d = tm_group_desc(desc, k);
    const TmEvalArgs &a = d.a;
    const int units = (a.Nx + TM_UNIT_BINS - 1) >> TM_UNIT_SHIFT;
    TmCostModel cm{0, 0, 0, TM_TILE_MAXU};
    tm_setup_body<TM_THREADS>(d.L, chain, d.f.params, d.f.Tcoefs, const_cast<double *>(a.wt), a.lx, units, a.cells, 1, 0, cm,
                              const_cast<TmMult *>(a.mult), const_cast<TmNoise *>(a.noise), const_cast<TmCellRec *>(a.cell),
                              const_cast<TmTileHdr *>(a.thdr), const_cast<TmActive *>(a.tidx), nullptr, nullptr, nullptr,
                              nullptr, s_dyn, nullptr);
    __threadfence();
    __syncthreads();
    asm volatile("s_dcache_inv\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
    TmEvalArgs b = a;
    asm volatile("" : "+s"(b.mult), "+s"(b.noise), "+s"(b.cell), "+s"(b.thdr), "+s"(b.tidx), "+s"(b.wt) : : "memory");
    tm_eval_body<false>(b, chain, 0, s_dyn + d.f.p_doubles);
}

int tm_launch_group_fused(const TmGroupFused *d_desc, const int32_t *d_pre, int n, int total, size_t lds, void *stream)
{
    if (n < 1 || total < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_group_fused_kernel, dim3(total), dim3(TM_THREADS), lds, (hipStream_t)stream, d_desc, d_pre, n);
    return (int)hipGetLastError();
}
