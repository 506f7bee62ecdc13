"""Resources of the PSIS-LOO kernels (tamcmc_loo.hip), cross-compiled for gfx950 (make resource-usage-loo): neither kernel
uses scratch or spills a register; the tail kernel uses no LDS at all, and the finalize kernel's LDS (the bin's sorted
values, the tail's t_j, the profile's theta / l) stays within 64 KiB per workgroup."""
from support import kernel_usage, needs_hipcc


@needs_hipcc
def test_loo_kernel_resources():
    usage = kernel_usage("resource-usage-loo")              # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == 2, sorted(usage)
    tail = [v for k, v in usage.items() if "tamcmc_loo_tail_kernel" in k]
    fin = [v for k, v in usage.items() if "tamcmc_loo_finalize_kernel" in k]
    assert len(tail) == 1 and len(fin) == 1, sorted(usage)
    for k, (scratch, sspill, vspill, lds) in usage.items():
        assert scratch == 0 and sspill == 0 and vspill == 0, (k, scratch, sspill, vspill)
    assert tail[0][3] == 0, tail
    assert 2048 * 8 <= fin[0][3] <= 64 * 1024, fin
