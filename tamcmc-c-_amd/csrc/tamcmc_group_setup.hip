// tamcmc_group_setup.hip -- the per-chain prologue of a fit group (tamcmc_group.h): one workgroup per chain over every
// member that takes the two-launch path, each running tm_setup_body with its member's layout and buffers.  Compiled with
// the flags of tamcmc_setup.o (-ffp-contract=off): a chain's records are those of its context's own setup launch.
#include <hip/hip_runtime.h>
#include "tamcmc_dev.h"
#include "tamcmc_setup_body.h"
#include "tamcmc_group.h"

__global__ __launch_bounds__(TM_SETUP_THREADS) void tamcmc_group_setup_kernel(const TmGroupSetup *desc, const int32_t *pre, int n)
{
    extern __shared__ double s_p[];   // as tamcmc_setup_kernel: the params row, then the unit-cost prefix
    const int k = tm_group_member(pre, n, (int)blockIdx.x);
    const int chain = (int)blockIdx.x - ((const __attribute__((address_space(4))) int32_t *)pre)[k];
    const TmGroupSetup &d = tm_group_desc(desc, k);
    int *s_pre = (d.eq != 0) ? reinterpret_cast<int *>(s_p + d.p_doubles) : nullptr;
    tm_setup_body<TM_SETUP_THREADS>(d.L, chain, d.params, d.Tcoefs, d.wt, d.lx, d.units, d.cells, d.tiles, d.eq, d.cm, d.mult,
                                    d.noise, d.cell, d.thdr, d.tidx, nullptr, nullptr, nullptr, d.order, s_p, s_pre);
}

int tm_launch_group_setup(const TmGroupSetup *d_desc, const int32_t *d_pre, int n, int total, size_t lds, void *stream)
{
    if (n < 1 || total < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tamcmc_group_setup_kernel, dim3(total), dim3(TM_SETUP_THREADS), lds, (hipStream_t)stream, d_desc, d_pre, n);
    return (int)hipGetLastError();
}
