"""Resources of the band ESS mode's kernels (tamcmc_bandess.hip), cross-compiled for gfx950 (make resource-usage-bandess):
exactly three kernels -- pack, lag, finish -- none of which uses scratch or spills a register (the pack kernel's eight
thresholds and eight words of bits, the lag kernel's three ring words, stay in registers), and no LDS: every counter belongs
to one thread."""
from support import kernel_usage, needs_hipcc

KERNELS = ("tamcmc_bandess_pack_kernel", "tamcmc_bandess_lag_kernel", "tamcmc_bandess_finish_kernel")


@needs_hipcc
def test_bandess_kernel_resources():
    usage = kernel_usage("resource-usage-bandess")          # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == len(KERNELS) and all(any(k in name for name in usage) for k in KERNELS), sorted(usage)
    for name, v in usage.items():
        assert v[:3] == (0, 0, 0), (name, v)
        assert v[3] == 0, (name, v)                                          # no LDS at all
