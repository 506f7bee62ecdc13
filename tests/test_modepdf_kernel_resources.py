"""The three kernels of tamcmc_modepdf.hip cross-compiled for gfx950 (make resource-usage-modepdf): none uses scratch or
spills a register; the histogram kernel's static LDS is its TM_PDF_MAX_BINS = 4096 uint32 counters with below and above
(at most 16 KiB + 64 bytes), the pair kernel's counters are dynamic LDS (its static LDS at most 64 bytes; 64 KiB + 4 bytes
asked for at the launch of 128 classes an axis, within the 160 KiB a workgroup may have), the HPD kernel holds one (width,
index) per wave."""
import os
import re

from support import kernel_usage, needs_hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@needs_hipcc
def test_kernel_resources():
    hdr = open(os.path.join(ROOT, "tamcmc-c-_amd", "csrc", "tamcmc_modepdf.h")).read()
    bins = int(re.search(r"#define TM_PDF_MAX_BINS (\d+)", hdr).group(1))
    bins2d = int(re.search(r"#define TM_PDF_MAX_BINS2D (\d+)", hdr).group(1))
    assert bins == 4096 and bins2d == 128 and (bins2d * bins2d + 1) * 4 <= 160 * 1024
    usage = kernel_usage("resource-usage-modepdf")             # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == 3, sorted(usage)
    kinds = {k: [s for s in ("hist_kernel", "pair_kernel", "hpd_kernel") if s in k] for k in usage}
    assert sorted(v[0] for v in kinds.values()) == ["hist_kernel", "hpd_kernel", "pair_kernel"], sorted(usage)
    for k, (scratch, sspill, vspill, lds) in usage.items():
        print(f"{kinds[k][0]}: SGPR spills {sspill}, LDS {lds} bytes")
        assert "modepdf" in k
        assert scratch == 0 and vspill == 0 and sspill == 0, (k, scratch, sspill, vspill)
        if "hist_kernel" in k:
            assert bins * 4 <= lds <= 16 * 1024 + 64, (k, lds)
        elif "pair_kernel" in k:
            assert lds <= 64, (k, lds)
        else:
            assert lds <= 64, (k, lds)
