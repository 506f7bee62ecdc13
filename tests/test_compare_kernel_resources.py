"""Resources of the kernels of the comparison of fits (tamcmc_compare.hip), cross-compiled for gfx950 (make
resource-usage-compare): exactly seven kernels -- bootstrap, finish, variates, prepare, the two stacking sums kernels (P from
the table, P formed from elpd) and update -- none of which uses scratch or spills a register (a thread's D of eight units and
seven fits and its running sums are indexed by unrolled loops and stay in registers), and LDS only for the waves' partial
sums: TM_CMP_LDS_BYTES and TM_CMP_STACK_LDS_BYTES of tamcmc_compare.h to the byte, and one double per column in update."""
import os
import re

from support import CSRC, kernel_usage, needs_hipcc

KERNELS = ("tamcmc_compare_bootstrap_kernel", "tamcmc_compare_finish_kernel", "tamcmc_compare_variates_kernel",
           "tamcmc_compare_prepare_kernel", "tamcmc_compare_stack_sums_kernelILb1E", "tamcmc_compare_stack_sums_kernelILb0E",
           "tamcmc_compare_stack_update_kernel")


def stated_lds():
    hdr = open(os.path.join(CSRC, "tamcmc_compare.h")).read()
    threads = int(re.search(r"#define TM_CMP_THREADS (\d+)", hdr).group(1))
    fits = int(re.search(r"#define TM_CMP_MAX_FITS (\d+)", hdr).group(1))
    assert "#define TM_CMP_WAVES (TM_CMP_THREADS / 64)" in hdr and "#define TM_CMP_STACK_COLS (TM_CMP_MAX_FITS + 1)" in hdr
    assert "#define TM_CMP_LDS_BYTES (TM_CMP_WAVES * 2 * TM_CMP_MAX_FITS * 8)" in hdr
    assert "#define TM_CMP_STACK_LDS_BYTES (TM_CMP_WAVES * TM_CMP_STACK_COLS * 8)" in hdr
    waves = threads // 64
    return waves * 2 * fits * 8, waves * (fits + 1) * 8, (fits + 1) * 8


@needs_hipcc
def test_compare_kernel_resources():
    usage = kernel_usage("resource-usage-compare")           # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == len(KERNELS) and all(any(k in name for name in usage) for k in KERNELS), sorted(usage)
    boot, sums, update = stated_lds()
    assert (boot, sums, update) == (512, 288, 72)
    for name, v in usage.items():
        assert v[:3] == (0, 0, 0), (name, v)
        want = boot if KERNELS[0] in name else sums if "stack_sums" in name else update if KERNELS[6] in name else 0
        assert v[3] == want, (name, v)
