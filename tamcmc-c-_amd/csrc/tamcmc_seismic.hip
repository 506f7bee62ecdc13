// tamcmc_seismic.hip -- the kernel of the mode table's seismic indices (tamcmc_seismic.h).
//
//   indices    one wave per sample, behind the derive kernel on the same rows.  The sample's base columns go into LDS (the
//              gathers of a column's terms are irregular; the row is read from memory once, coalesced); lane j evaluates
//              index column j (j + 64, ... for plans with more than 64) with tm_seis_eval, the function the CPU check
//              runs, and writes it behind the base columns.  A column is one lane's serial loop however many terms it has:
//              the order of addition is part of the result, so nothing is reduced across lanes.  The plan -- per-column
//              term ranges, sources, weights, coefficients, offsets -- is read from device memory; every wave reads the
//              same few kilobytes.  Compiled without floating-point contraction: + - * / only, the bits of the host.
//              Status: a sample whose status is OK and that has a NaN index column gets TAMCMC_CHAIN_NAN (the table's
//              rule "any of its columns is a NaN"); +-inf is a value.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)
#include "tamcmc_seismic.h"

__global__ __launch_bounds__(TM_SEIS_THREADS) void tamcmc_seismic_kernel(const TmSeisArgs a)
{
    extern __shared__ double s_x[];          // this sample's base columns
    __shared__ int s_nan;
    const int lane = threadIdx.x, sample = blockIdx.x;
    if (sample >= a.B) return;
    double *row = a.rows + (size_t)sample * (size_t)a.n_cols;
    for (int e = lane; e < a.n_base_cols; e += TM_SEIS_THREADS) s_x[e] = row[e];
    if (lane == 0) s_nan = 0;
    __syncthreads();
    bool nan = false;
    for (int c = lane; c < a.n_index; c += TM_SEIS_THREADS) {
        const int t0 = a.first[c], t2 = a.first[c + 1], t1 = t0 + a.n_num[c];
        const double v = tm_seis_eval(s_x, a.src, a.wsrc, a.coef, t0, t1, t2, a.offset[c]);
        row[a.n_base_cols + c] = v;
        nan = nan || !(v == v);
    }
    if (nan) atomicOr(&s_nan, 1);
    __syncthreads();
    if (lane == 0 && s_nan != 0 && a.status[sample] == 0) a.status[sample] = 1;      // 1 = TAMCMC_CHAIN_NAN
}

int tm_launch_seismic(const TmSeisArgs &a, void *stream)
{
    const size_t lds = ((size_t)a.n_base_cols + 1) * sizeof(double);
    hipLaunchKernelGGL(tamcmc_seismic_kernel, dim3(a.B), dim3(TM_SEIS_THREADS), lds, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
