"""Resources of the posterior predictive kernel (tamcmc_predictive.hip), cross-compiled for gfx950 (make
resource-usage-predictive): exactly one kernel, and like the fold kernel it uses no scratch, spills no register and has no
LDS -- the three per-sample routines (chi_square, p = 1, p > 1) and their loops stay in registers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tamcmc-c-_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_predictive_kernel_resources():
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-predictive"], capture_output=True, text=True, timeout=600)
    txt = r.stdout + r.stderr
    assert r.returncode == 0, txt[-3000:]
    usage = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?"
                         r"LDS Size \[bytes/block\]: (\d+)", txt, flags=re.S):
        usage[m.group(1)] = tuple(int(m.group(k)) for k in (2, 3, 4, 5))     # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == 1 and "tamcmc_summary_predictive_kernel" in next(iter(usage)), sorted(usage)
    for k, v in usage.items():
        assert v == (0, 0, 0, 0), (k, v)
