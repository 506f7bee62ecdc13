"""The kernel of tamcmc_seismic.hip cross-compiled for gfx950 (make resource-usage-seismic): no scratch, no spilled
register; its static LDS is the one NaN flag (the sample's base columns are dynamic LDS, 8 n_base_cols bytes at launch, which
tamcmc_modetable_indices_enable refuses above TM_SEIS_LDS_MAX)."""
import os
import re

from support import kernel_usage, needs_hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@needs_hipcc
def test_kernel_resources():
    hdr = open(os.path.join(ROOT, "tamcmc-c-_amd", "csrc", "tamcmc_seismic.h")).read()
    assert re.search(r"#define TM_SEIS_LDS_MAX \(60 \* 1024\)", hdr) and re.search(r"#define TM_SEIS_THREADS 64\b", hdr)
    usage = kernel_usage("resource-usage-seismic")              # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == 1 and "tamcmc_seismic_kernel" in next(iter(usage)), sorted(usage)
    for k, (scratch, sspill, vspill, lds) in usage.items():
        print(f"{k}: SGPR spills {sspill}, static LDS {lds} bytes")
        assert scratch == 0 and sspill == 0 and vspill == 0 and lds <= 16, (k, scratch, sspill, vspill, lds)
