"""Resources of the LOO-PIT kernels (tamcmc_loopit.hip), cross-compiled for gfx950 (make resource-usage-loopit): exactly two
kernels; neither uses scratch or spills a register; the PIT kernel uses no LDS at all, and the prepare kernel's LDS (the
bin's sorted values, the tail's log weights, the profile's theta / l) stays within 64 KiB per workgroup."""
from support import kernel_usage, needs_hipcc


@needs_hipcc
def test_loopit_kernel_resources():
    usage = kernel_usage("resource-usage-loopit")           # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == 2, sorted(usage)
    prep = [v for k, v in usage.items() if "tamcmc_loopit_prepare_kernel" in k]
    pit = [v for k, v in usage.items() if "tamcmc_loopit_kernel" in k]
    assert len(prep) == 1 and len(pit) == 1, sorted(usage)
    for k, (scratch, sspill, vspill, lds) in usage.items():
        assert scratch == 0 and sspill == 0 and vspill == 0, (k, scratch, sspill, vspill)
    assert pit[0][3] == 0, pit
    assert 2048 * 8 <= prep[0][3] <= 64 * 1024, prep
