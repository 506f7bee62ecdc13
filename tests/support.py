"""What the test modules share that is not about one feature: the paths of the golden inputs, the oracle, the command-line
tool, the launcher of a fresh process in which torch owns the device first, and the parser of the compiler's
kernel-resource-usage remarks.  Importing this module needs no GPU."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CSRC = os.path.join(ROOT, "tamcmc-c-_amd", "csrc")
G = os.path.join(ROOT, "tests", "golden", "ref_inputs")
CFG = os.path.join(G, "Config_default")
MODEL, DATA = os.path.join(G, "TF_3443483_local-v3.model"), os.path.join(G, "TF_3443483_local-v3.data")
LD = np.longdouble

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                 reason="hipcc not available")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pyorc():
    """The CPU oracle, for module-level helpers that cannot take conftest's `orc` fixture."""
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


def tool():
    exe = os.path.join(ROOT, "bin", "chainsummary_hip")
    if not os.path.exists(exe):        # tests/conftest.py builds only when one of the two older tools is missing
        subprocess.run(["make", "-C", CSRC, "-j4"], check=True)
    return exe


def in_torch_process(module, fn, marker, timeout=300):
    """Runs `module.fn()` in a fresh child process where torch owns the device first (as bench.py); the child must exit 0
    and print `marker`."""
    code = ("import torch, sys; sys.path[:0] = [%r, %r]; import %s as t; t.%s()" % (ROOT, TESTS, module, fn))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and marker in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def kernel_usage(make_target):
    """`make <target>` in csrc compiles for gfx950 with -Rpass-analysis=kernel-resource-usage.  Returns function name ->
    (scratch bytes per lane, spilled SGPRs, spilled VGPRs, LDS bytes per block)."""
    r = subprocess.run(["make", "-s", "-C", CSRC, make_target], capture_output=True, text=True, timeout=600)
    txt = r.stdout + r.stderr
    assert r.returncode == 0, txt[-3000:]
    usage = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?"
                         r"LDS Size \[bytes/block\]: (\d+)", txt, flags=re.S):
        usage[m.group(1)] = tuple(int(m.group(k)) for k in (2, 3, 4, 5))
    return usage
