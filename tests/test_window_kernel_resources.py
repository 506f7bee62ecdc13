"""Resources of the windowed predictive check's kernels (tamcmc_window.hip), cross-compiled for gfx950 (make
resource-usage-window): exactly three kernels -- sums, tails, fold -- none of which uses scratch or spills a register (the
510-step loop of the tails at shape 512 and the launch arguments' three shapes stay in registers), and LDS only in the
sums kernel, at most 64 KiB per workgroup so that at least two workgroups fit a compute unit's 160 KiB."""
from support import kernel_usage, needs_hipcc

KERNELS = ("tamcmc_summary_window_sums_kernel", "tamcmc_summary_window_tails_kernel", "tamcmc_summary_window_fold_kernel")


@needs_hipcc
def test_window_kernel_resources():
    usage = kernel_usage("resource-usage-window")           # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == len(KERNELS) and all(any(k in name for name in usage) for k in KERNELS), sorted(usage)
    for name, v in usage.items():
        assert v[:3] == (0, 0, 0), (name, v)
        assert (0 < v[3] <= 65536) if KERNELS[0] in name else v[3] == 0, (name, v)
