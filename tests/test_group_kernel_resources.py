"""Register budgets of the fit-group kernels (tamcmc_group_*.hip), cross-compiled for gfx950 beside their solo
counterparts with the same flags (make resource-usage-group): the grouped likelihood launch stays within the solo
kernel's 72-VGPR step (7 waves / SIMD), and the grouped prologue and fused kernels use no more VGPRs than the solo ones."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tamcmc-c-_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_group_kernel_register_budget():
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-group"], capture_output=True, text=True, timeout=900)
    txt = r.stdout + r.stderr
    assert r.returncode == 0, txt[-3000:]
    usage = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)", txt, flags=re.S):
        usage[m.group(1)] = (int(m.group(2)), int(m.group(4)), int(m.group(3)))       # VGPRs, spilled VGPRs, scratch bytes

    def one(key):
        v = [u for k, u in usage.items() if key in k]
        assert len(v) >= 1, (key, sorted(usage))
        return v

    g_eval = one("tamcmc_group_eval_kernel")
    assert len(g_eval) == 2                                   # specialised and generic body
    for vg, spill, scratch in g_eval:
        assert vg <= 72 and spill == 0 and scratch == 0, g_eval
    (gf,) = one("tamcmc_group_fused_kernel")
    solo_fused = one("tamcmc_fused_kernelILb0")[0]
    assert gf[1] == 0 and gf[2] == 0 and gf[0] <= solo_fused[0], (gf, solo_fused)
    (gs,) = one("tamcmc_group_setup_kernel")
    solo_setup = one("tamcmc_setup_kernel")[0]
    assert gs[1] == 0 and gs[0] <= solo_setup[0], (gs, solo_setup)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_group_kernels_never_touch_scratch(tmp_path):
    """The prologue body makes the compiler reserve a private segment -- 36 bytes per lane in the solo setup kernel, 68 in
    the grouped one (ScratchSize above) -- that neither kernel ever addresses: their code holds no private-memory load or
    store, so the reservation costs no traffic.  The grouped eval and fused kernels reserve none."""
    r = subprocess.run(["make", "-s", "-C", CSRC, "group-asm", f"ASMDIR={tmp_path}"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    private = re.compile(r"^\s*(scratch_(load|store)\w*|buffer_(load|store)\w*)\b", flags=re.M)
    for name in ("tamcmc_setup", "tamcmc_group_setup", "tamcmc_group_eval", "tamcmc_group_fused"):
        asm = (tmp_path / f"{name}.s").read_text()
        assert "_kernel" in asm and not private.findall(asm), (name, private.findall(asm)[:5])
        sizes = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", asm)]
        if name in ("tamcmc_group_eval", "tamcmc_group_fused"):
            assert sizes and max(sizes) == 0, (name, sizes)
