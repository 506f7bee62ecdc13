"""Resources of the ESS mode's kernels (tamcmc_ess.hip), cross-compiled for gfx950 (make resource-usage-ess): exactly three
kernels -- centre, lag, finish -- none of which uses scratch or spills a register (the lag kernel's sixteen accumulators,
its window of past values and the sixteen samples in flight stay in registers), and no LDS: nothing is sized by the block
of samples."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tamcmc-c-_amd", "csrc")
KERNELS = ("tamcmc_ess_centre_kernel", "tamcmc_ess_lag_kernel", "tamcmc_ess_finish_kernel")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_ess_kernel_resources():
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-ess"], capture_output=True, text=True, timeout=600)
    txt = r.stdout + r.stderr
    assert r.returncode == 0, txt[-3000:]
    usage = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?"
                         r"LDS Size \[bytes/block\]: (\d+)", txt, flags=re.S):
        usage[m.group(1)] = tuple(int(m.group(k)) for k in (2, 3, 4, 5))     # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == len(KERNELS) and all(any(k in name for name in usage) for k in KERNELS), sorted(usage)
    for name, v in usage.items():
        assert v[:3] == (0, 0, 0), (name, v)
        assert v[3] == 0, (name, v)                                          # the layout in use has no LDS at all
