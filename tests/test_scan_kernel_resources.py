"""Resources of the sliding-window scan's kernels (tamcmc_scan.hip), cross-compiled for gfx950 (make resource-usage-scan):
exactly three kernels -- sums, tails, fold -- none of which uses scratch or spills a register (the launch arguments' eight
widths, offsets and shapes are picked by uniform selects and stay in registers), and LDS only in the sums kernel, which
stages a tile's residuals and its halo: at most 64 KiB per workgroup so that at least two workgroups fit a compute unit's
160 KiB."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tamcmc-c-_amd", "csrc")
KERNELS = ("tamcmc_summary_scan_sums_kernel", "tamcmc_summary_scan_tails_kernel", "tamcmc_summary_scan_fold_kernel")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_scan_kernel_resources():
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-scan"], capture_output=True, text=True, timeout=600)
    txt = r.stdout + r.stderr
    assert r.returncode == 0, txt[-3000:]
    usage = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?"
                         r"LDS Size \[bytes/block\]: (\d+)", txt, flags=re.S):
        usage[m.group(1)] = tuple(int(m.group(k)) for k in (2, 3, 4, 5))     # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == len(KERNELS) and all(any(k in name for name in usage) for k in KERNELS), sorted(usage)
    for name, v in usage.items():
        assert v[:3] == (0, 0, 0), (name, v)
        assert (0 < v[3] <= 65536) if KERNELS[0] in name else v[3] == 0, (name, v)
