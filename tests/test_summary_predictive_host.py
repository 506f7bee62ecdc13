"""Posterior predictive check of a stored chain (tamcmc_summary_predictive_*, include/tamcmc_accel.h), the part that needs
no GPU: the symbols exist with the declared prototypes and struct layout, a NULL handle is refused before any device is
touched, the command-line tool knows the option, the long-double erfc of the GPU test's reference agrees with mpmath, and
the per-sample arithmetic (tamcmc_predictive.h, shared by the kernel) -- log P and log Q of chi(2,2p) and of the Gaussian,
the guarded log-sum-exp -- agrees on the CPU with a long-double brute force (tests/cpp/predictive_core_check.cpp, plain
g++)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from summary_support import prototypes
from support import tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tamcmc_summary_predictive_enable", "tamcmc_summary_predictive_result", "tamcmc_summary_predictive_kernel_time"]


def test_symbols_and_signatures(accel_mod):
    lib = accel_mod.load_library()
    protos, txt = prototypes()
    for n in NAMES:
        assert hasattr(lib, n) and n in accel_mod.capi.EXPORTS, n
    assert protos["tamcmc_summary_predictive_enable"] == ["tamcmc_summary*"]
    assert protos["tamcmc_summary_predictive_result"] == ["tamcmc_summary*", "tamcmc_summary_predictive_totals*"] + ["double*"] * 4
    assert protos["tamcmc_summary_predictive_kernel_time"] == ["tamcmc_summary*", "double*", "int64_t*"]
    assert "#define TAMCMC_SUMMARY_PREDICTIVE_MAX_P 64" in txt and accel_mod.capi.Summary.PREDICTIVE_MAX_P == 64
    assert "#define TAMCMC_SUMMARY_PIT_CELLS 20" in txt and accel_mod.capi.Summary.PIT_CELLS == 20
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_summary_predictive_totals;", txt)
    assert m and " ".join(m.group(1).split()) == \
        ("int64_t n_used, n_rejected; double ks_D, min_log_sf, min_log_cdf; int64_t bin_min_log_sf, bin_min_log_cdf; "
         "int64_t pit_hist[TAMCMC_SUMMARY_PIT_CELLS];")
    t = accel_mod.capi.SummaryPredictiveTotals
    assert [f[0] for f in t._fields_] == ["n_used", "n_rejected", "ks_D", "min_log_sf", "min_log_cdf", "bin_min_log_sf",
                                         "bin_min_log_cdf", "pit_hist"]
    assert C.sizeof(t) == 7 * 8 + 20 * 8 and t.pit_hist.offset == 56 and t.ks_D.offset == 16 and t.bin_min_log_sf.offset == 40
    for meth in ("predictive_enable", "predictive_result", "predictive_kernel_time"):
        assert callable(getattr(accel_mod.Summary, meth))
    # what the earlier modes expose stays as it is
    assert accel_mod.Summary.ARRAYS == ("mean_M", "var_M", "min_M", "max_M", "mean_l", "var_l", "lppd")
    assert C.sizeof(accel_mod.capi.SummaryTotals) == 40 and C.sizeof(accel_mod.capi.SummaryLooTotals) == 64


def test_null_handle_is_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(8, 7.0)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    t = accel_mod.capi.SummaryPredictiveTotals()
    t.n_used = 77
    assert lib.tamcmc_summary_predictive_enable(None) == E
    assert lib.tamcmc_summary_predictive_result(None, C.byref(t), xp, xp, xp, xp) == E
    assert np.all(x == 7.0) and t.n_used == 77
    assert lib.tamcmc_summary_predictive_result(None, None, None, None, None, None) == E
    n = C.c_int64(5)
    assert lib.tamcmc_summary_predictive_kernel_time(None, xp, C.byref(n)) == E and n.value == 5 and x[0] == 7.0


def test_tool_knows_the_option():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--predictive" in r.stderr and "pit log_cdf log_sf mean_resid" in r.stderr and r.stdout == ""
    r = subprocess.run([exe, "a", "b", "c", "d", "e", "--predictive", "--thin"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr
    r = subprocess.run([exe, "a", "b", "c", "d", "e", "--predictive", "--loo"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Usage" not in r.stderr and "cannot read the default configuration" in r.stderr      # the option is taken


def test_core_arithmetic_against_long_double(tmp_path):
    """The header compiles as plain C++17 under g++: p in {1, 2, 3, 17, 64} over z from 0 and a denormal to 1e300, r from 0 to
    +-1e3, both sides of every branch switch, log(P + Q) = 0, monotony, and the guarded log-sum-exp."""
    exe = str(tmp_path / "predictive_core_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "tamcmc-c-_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "predictive_core_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok predictive_core_check") and r.stdout.count("\n") == 1, (r.stdout, r.stderr[-3000:])


def test_reference_erfc_against_mpmath():
    """log(erfc(r) / 2) of tests/predictive_reference.py, the long-double series / continued fraction the GPU test leans
    on, against mpmath at 50 digits: within 8 long-double ulp of max(1, |value|)."""
    mp = pytest.importorskip("mpmath")
    import predictive_reference as R
    mp.mp.dps = 50
    LD = np.longdouble
    rs = [0.0, 1e-8, 0.3, 0.5, 1.0, 2.0, 2.5, 3.0, 5.0, 10.0, 26.0, 27.0, 40.0, 1e3]
    rs = np.array(sorted(set(rs + [-r for r in rs])), dtype=LD)
    got = R.log_half_erfc(rs)
    worst = 0.0
    for r, g in zip(rs, got):
        want = mp.log(mp.erfc(mp.mpf(float(r))) / 2)
        err = abs(mp.mpf(str(np.format_float_scientific(g, precision=25, unique=False))) - want) / max(1, abs(want))
        worst = max(worst, float(err))
    print("worst relative error of the reference's log(erfc / 2):", worst)
    assert worst <= 8 * float(np.finfo(LD).eps)


def test_reference_gamma_tails():
    """The reference's general sums at p = 1 against the closed form it uses there, and P + Q = 1 for every p: within 8
    long-double ulp of max(1, |value|) (for p > 1: of the largest term of the log-domain sums, 4 p)."""
    import predictive_reference as R
    LD = np.longdouble
    eps = float(np.finfo(LD).eps)
    z = np.concatenate([[0.0, -1.0, 5e-324, 1e-300, 1e-10], np.geomspace(1e-3, 3e3, 400), [1e6, 1e300]]).astype(LD)
    aP, aQ = R.log_gamma_tails(1, z)
    bP, bQ = R.log_gamma_tails(1, z, closed_form=False)
    fin = np.isfinite(aP)
    assert np.array_equal(fin, np.isfinite(bP)) and np.array_equal(aP[~fin], bP[~fin]) and not fin[0] and not fin[1]
    assert float(np.max(np.abs(aP[fin] - bP[fin]) / np.maximum(1, np.abs(aP[fin])))) <= 8 * eps
    assert float(np.max(np.abs(aQ - bQ) / np.maximum(1, np.abs(aQ)))) <= 8 * eps
    for p in (1, 2, 3, 17, 64):
        lP, lQ = R.log_gamma_tails(p, z[2:])
        assert np.all(np.isfinite(lP)) and np.all(np.isfinite(lQ)) and np.all(np.diff(lP) >= -8 * eps * 4 * p) and np.all(np.diff(lQ) <= 8 * eps * 4 * p)
        assert float(np.max(np.abs(np.exp(lP) + np.exp(lQ) - 1))) <= 8 * eps * 4 * p, p
