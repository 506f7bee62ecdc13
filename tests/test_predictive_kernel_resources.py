"""Resources of the posterior predictive kernel (tamcmc_predictive.hip), cross-compiled for gfx950 (make
resource-usage-predictive): exactly one kernel, and like the fold kernel it uses no scratch, spills no register and has no
LDS -- the three per-sample routines (chi_square, p = 1, p > 1) and their loops stay in registers."""
from support import kernel_usage, needs_hipcc


@needs_hipcc
def test_predictive_kernel_resources():
    usage = kernel_usage("resource-usage-predictive")       # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == 1 and "tamcmc_summary_predictive_kernel" in next(iter(usage)), sorted(usage)
    for k, v in usage.items():
        assert v == (0, 0, 0, 0), (k, v)
