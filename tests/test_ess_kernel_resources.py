"""Resources of the ESS mode's kernels (tamcmc_ess.hip), cross-compiled for gfx950 (make resource-usage-ess): exactly three
kernels -- centre, lag, finish -- none of which uses scratch or spills a register (the lag kernel's sixteen accumulators,
its window of past values and the sixteen samples in flight stay in registers), and no LDS: nothing is sized by the block
of samples."""
from support import kernel_usage, needs_hipcc

KERNELS = ("tamcmc_ess_centre_kernel", "tamcmc_ess_lag_kernel", "tamcmc_ess_finish_kernel")


@needs_hipcc
def test_ess_kernel_resources():
    usage = kernel_usage("resource-usage-ess")              # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == len(KERNELS) and all(any(k in name for name in usage) for k in KERNELS), sorted(usage)
    for name, v in usage.items():
        assert v[:3] == (0, 0, 0), (name, v)
        assert v[3] == 0, (name, v)                                          # the layout in use has no LDS at all
