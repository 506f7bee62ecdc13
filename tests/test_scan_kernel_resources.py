"""Resources of the sliding-window scan's kernels (tamcmc_scan.hip), cross-compiled for gfx950 (make resource-usage-scan):
exactly three kernels -- sums, tails, fold -- none of which uses scratch or spills a register (the launch arguments' eight
widths, offsets and shapes are picked by uniform selects and stay in registers), and LDS only in the sums kernel, which
stages a tile's residuals and its halo: at most 64 KiB per workgroup so that at least two workgroups fit a compute unit's
160 KiB."""
from support import kernel_usage, needs_hipcc

KERNELS = ("tamcmc_summary_scan_sums_kernel", "tamcmc_summary_scan_tails_kernel", "tamcmc_summary_scan_fold_kernel")


@needs_hipcc
def test_scan_kernel_resources():
    usage = kernel_usage("resource-usage-scan")             # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == len(KERNELS) and all(any(k in name for name in usage) for k in KERNELS), sorted(usage)
    for name, v in usage.items():
        assert v[:3] == (0, 0, 0), (name, v)
        assert (0 < v[3] <= 65536) if KERNELS[0] in name else v[3] == 0, (name, v)
