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


# The reference's .model files that come without a spectrum, and the reader each is written for
REF_MODEL_FILES = [("kplr008379927_kasoc-psd_slc_v2_1000.model", "io_MS_Global"), ("00088.0.model", "io_MS_Global"),
                   ("02194.0.model", "io_MS_Global"), ("kplr008379927_kasoc-psd_slc_v2_1000_local-v2.model", "io_local")]


def chains_around(s, n, seed=3, scale=0.3):
    """n parameter rows: the file's initial guesses, then Gaussian steps of `scale` x the initial proposal errors."""
    rng = np.random.default_rng(seed)
    P = np.tile(s.inputs, (n, 1))
    P[1:, s.index_to_relax] += scale * s.err * rng.standard_normal((n - 1, s.Nvars))
    return P


def load_on_flat_spectrum(name, reader, tmp_path, step=0.02):
    """The Setup of the reference's .model file `name` (first slice) read by `reader`, on a grid of `step` that covers the
    slice with a flat spectrum y = 1 standing in for the data the file comes without."""
    from tamcmc_amd.setup_io import Setup, model_file_slices
    path = os.path.join(G, name)
    lo, hi = model_file_slices(path)[0]
    x = np.arange(lo - 5 * step, hi + 5 * step, step)
    d = os.path.join(str(tmp_path), "flat.data")
    with open(d, "w") as f:
        f.write("# flat\n! frequency power\n* (microHz) (ppm^2/microHz)\n" + "".join("%.8f 1.0\n" % v for v in x))
    s = Setup(CFG)
    s.set("Modeling", "prior_fct_name", reader)
    s.load(path, d, 0)
    return s
