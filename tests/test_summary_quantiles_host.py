"""Quantiles of a stored chain (tamcmc_summary_quantiles_*, include/tamcmc_accel.h), the part that needs no GPU: the symbols
exist with the declared prototypes, a NULL handle is refused before any device is touched, the command-line tool knows the
option, and the per-bin arithmetic of the selection (tamcmc_quantile.h, shared by the kernels) agrees with a sort on the
CPU (tests/cpp/quantile_core_check.cpp, plain g++)."""
import ctypes as C
import os
import subprocess

import numpy as np

from summary_support import prototypes
from support import tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tamcmc_summary_quantiles_begin", "tamcmc_summary_quantiles_step", "tamcmc_summary_quantiles_result",
         "tamcmc_summary_quantiles_end"]


def test_symbols_and_signatures(accel_mod):
    lib = accel_mod.load_library()
    protos, txt = prototypes()
    for n in NAMES:
        assert hasattr(lib, n) and n in accel_mod.capi.EXPORTS, n
    assert protos["tamcmc_summary_quantiles_begin"] == ["tamcmc_summary*", "int32_t", "const double*", "int32_t"]
    assert protos["tamcmc_summary_quantiles_step"] == ["tamcmc_summary*", "int32_t*"]
    assert protos["tamcmc_summary_quantiles_result"] == ["tamcmc_summary*", "int64_t*", "double*", "double*"]
    assert protos["tamcmc_summary_quantiles_end"] == ["tamcmc_summary*"]
    assert "#define TAMCMC_SUMMARY_MAX_QUANTILES 8" in txt and accel_mod.capi.Summary.MAX_QUANTILES == 8
    for m in ("quantiles_begin", "quantiles_step", "quantiles_result", "quantiles_end", "quantiles"):
        assert callable(getattr(accel_mod.Summary, m))


def test_null_handle_is_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    q = np.array([0.16, 0.5, 0.84])
    qp = q.ctypes.data_as(C.POINTER(C.c_double))
    left = C.c_int32(77)
    ranks = np.zeros(3, dtype=np.int64)
    assert lib.tamcmc_summary_quantiles_begin(None, 3, qp, 0) == E
    assert lib.tamcmc_summary_quantiles_begin(None, 0, None, 9) == E
    assert lib.tamcmc_summary_quantiles_step(None, C.byref(left)) == E and left.value == 77
    assert lib.tamcmc_summary_quantiles_step(None, None) == E
    assert lib.tamcmc_summary_quantiles_result(None, ranks.ctypes.data_as(C.POINTER(C.c_int64)), qp, qp) == E
    assert lib.tamcmc_summary_quantiles_result(None, None, None, None) == E
    assert lib.tamcmc_summary_quantiles_end(None) == E


def test_tool_knows_the_option():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--quantiles" in r.stderr and "--qbits" in r.stderr and r.stdout == ""
    for extra in (["--quantiles"], ["--quantiles", "1.5"], ["--quantiles", "0.5,"], ["--quantiles", "0.1,x"],
                  ["--quantiles", "nan"], ["--quantiles", "0.5", "--qbits", "7"],
                  ["--quantiles", "0,.1,.2,.3,.4,.5,.6,.7,.8"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr, extra


def test_core_arithmetic_against_a_sort(tmp_path):
    """The header compiles as plain C++17 under g++; key map, inverse, and whole selections for bits 1 ... 6 and every rank."""
    exe = str(tmp_path / "quantile_core_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "tamcmc-c-_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "quantile_core_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok quantile_core_check") and r.stdout.count("\n") == 1, (r.stdout, r.stderr[-3000:])
