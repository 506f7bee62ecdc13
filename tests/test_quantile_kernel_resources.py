"""Resources of the quantile kernels (tamcmc_quantile.hip), cross-compiled for gfx950 (make resource-usage-quantile): no
kernel uses scratch or spills a VGPR, and the histogram kernel's LDS counters stay within 64 KiB per workgroup in every
instantiation (the largest holds 8 quantiles x 64 cells x 64 threads x 2 bytes = exactly 64 KiB)."""
from support import kernel_usage, needs_hipcc


@needs_hipcc
def test_quantile_kernel_resources():
    usage = {k: (v[0], v[2], v[3]) for k, v in kernel_usage("resource-usage-quantile").items()}      # scratch bytes, spilled VGPRs, LDS bytes
    hist = {k: v for k, v in usage.items() if "tamcmc_quantile_hist_kernel" in k}
    assert len(hist) == 4 and len(usage) == 6, sorted(usage)
    assert any("tamcmc_quantile_narrow_kernel" in k for k in usage) and any("tamcmc_quantile_init_kernel" in k for k in usage)
    for k, (scratch, spill, lds) in usage.items():
        assert scratch == 0 and spill == 0, (k, scratch, spill)
    assert sorted(v[2] for v in hist.values()) == [8192, 16384, 32768, 65536], hist
    for k, v in usage.items():
        if k not in hist:
            assert v[2] == 0, (k, v)
