"""Resources of the PSIS-LOO kernels (tamcmc_loo.hip), cross-compiled for gfx950 (make resource-usage-loo): neither kernel
uses scratch or spills a register; the tail kernel uses no LDS at all, and the finalize kernel's LDS (the bin's sorted
values, the tail's t_j, the profile's theta / l) stays within 64 KiB per workgroup."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tamcmc-c-_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_loo_kernel_resources():
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-loo"], capture_output=True, text=True, timeout=600)
    txt = r.stdout + r.stderr
    assert r.returncode == 0, txt[-3000:]
    usage = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?"
                         r"LDS Size \[bytes/block\]: (\d+)", txt, flags=re.S):
        usage[m.group(1)] = tuple(int(m.group(k)) for k in (2, 3, 4, 5))     # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == 2, sorted(usage)
    tail = [v for k, v in usage.items() if "tamcmc_loo_tail_kernel" in k]
    fin = [v for k, v in usage.items() if "tamcmc_loo_finalize_kernel" in k]
    assert len(tail) == 1 and len(fin) == 1, sorted(usage)
    for k, (scratch, sspill, vspill, lds) in usage.items():
        assert scratch == 0 and sspill == 0 and vspill == 0, (k, scratch, sspill, vspill)
    assert tail[0][3] == 0, tail
    assert 2048 * 8 <= fin[0][3] <= 64 * 1024, fin
