"""Effective sample size of a stored chain (tamcmc_summary_ess_*, include/tamcmc_accel.h), the part that needs no GPU: the
symbols exist with the declared prototypes and struct layout, a NULL handle and calls outside the mode are refused before
any device is touched, the command-line tool knows the option, the reference the GPU test leans on (tests/ess_reference.py)
agrees with itself on known sequences, and the shared arithmetic (tamcmc_ess.h: the accumulation rule, the ring and carry,
the finish, the R-hat formula) agrees on the CPU with a long-double brute force (tests/cpp/ess_core_check.cpp, plain g++,
built by csrc/Makefile's ess-core-check)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from summary_support import prototypes
from support import tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tamcmc_summary_ess_begin", "tamcmc_summary_ess_result", "tamcmc_summary_ess_acov", "tamcmc_summary_ess_end"]
FIELDS = ["n_used", "n_rejected", "lag", "min_ess_M", "min_ess_l", "max_rhat", "bin_min_ess_M", "bin_min_ess_l", "bin_max_rhat",
          "n_truncated_M", "n_truncated_l", "n_rhat_high"]


def test_symbols_and_signatures(accel_mod):
    lib = accel_mod.load_library()
    protos, txt = prototypes()
    for n in NAMES:
        assert hasattr(lib, n) and n in accel_mod.capi.EXPORTS, n
    assert protos["tamcmc_summary_ess_begin"] == ["tamcmc_summary*", "int32_t", "int32_t*"]
    assert protos["tamcmc_summary_ess_result"] == ["tamcmc_summary*", "tamcmc_summary_ess_totals*"] + ["double*"] * 4 + ["int32_t*"] + \
        ["double*"] * 2 + ["int32_t*"]
    assert protos["tamcmc_summary_ess_acov"] == ["tamcmc_summary*", "int32_t", "double*"]
    assert protos["tamcmc_summary_ess_end"] == ["tamcmc_summary*"]
    assert "#define TAMCMC_SUMMARY_ESS_MAX_LAG 1023" in txt and accel_mod.capi.Summary.ESS_MAX_LAG == 1023
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_summary_ess_totals;", txt)
    assert m and " ".join(m.group(1).split()) == \
        ("int64_t n_used, n_rejected, lag; double min_ess_M, min_ess_l, max_rhat; int64_t bin_min_ess_M, bin_min_ess_l, bin_max_rhat; "
         "int64_t n_truncated_M, n_truncated_l, n_rhat_high;")
    t = accel_mod.capi.SummaryEssTotals
    assert [f[0] for f in t._fields_] == FIELDS
    kinds = dict(t._fields_)
    for k, name in enumerate(FIELDS):                        # every field is eight bytes wide, in the header's order
        assert getattr(t, name).offset == 8 * k, name
        assert kinds[name] is (C.c_double if name in ("min_ess_M", "min_ess_l", "max_rhat") else C.c_int64), name
    assert C.sizeof(t) == 12 * 8
    assert accel_mod.Summary.ESS_ARRAYS == ("ess_M", "tau_M", "mcse_M", "rhat_M", "cut_M", "ess_l", "r_eff", "cut_l")
    assert accel_mod.Summary.ESS_TOTALS == tuple(FIELDS)
    for meth in ("ess_begin", "ess_result", "ess_acov", "ess_end", "ess"):
        assert callable(getattr(accel_mod.Summary, meth))
    # what the other modes expose stays as it is
    assert C.sizeof(accel_mod.capi.SummaryLooTotals) == 8 * 8 and C.sizeof(accel_mod.capi.SummaryTotals) == 5 * 8
    # the header's macro and the kernels' constant agree
    h = open(os.path.join(ROOT, "tamcmc-c-_amd", "csrc", "tamcmc_ess.h")).read()
    assert "#define TM_ESS_MAX_LAG 1023" in h and "#define TM_ESS_DEFAULT_LAG 255" in h


def test_null_handle_is_refused_without_a_device(accel_mod):
    """A NULL object is every entry point's first refusal, and it is also how a call outside the mode ends without a device:
    nothing is written."""
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(8, 7.0)
    c = np.full(8, 7, dtype=np.int32)
    xp, cp = x.ctypes.data_as(C.POINTER(C.c_double)), c.ctypes.data_as(C.POINTER(C.c_int32))
    t = accel_mod.capi.SummaryEssTotals()
    t.n_used = 77
    lag = C.c_int32(-5)
    assert lib.tamcmc_summary_ess_begin(None, 0, C.byref(lag)) == E and lag.value == -5
    assert lib.tamcmc_summary_ess_begin(None, 255, None) == E
    assert lib.tamcmc_summary_ess_result(None, C.byref(t), xp, xp, xp, xp, cp, xp, xp, cp) == E
    assert lib.tamcmc_summary_ess_result(None, None, None, None, None, None, None, None, None, None) == E
    assert lib.tamcmc_summary_ess_acov(None, 0, xp) == E and lib.tamcmc_summary_ess_acov(None, 1, None) == E
    assert lib.tamcmc_summary_ess_end(None) == E
    assert np.all(x == 7.0) and np.all(c == 7) and t.n_used == 77


def test_tool_knows_the_option():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--ess [L]" in r.stderr and ".ess" in r.stderr and "ess_M tau_M mcse_M rhat_M cut_M ess_l r_eff cut_l" in r.stderr
    assert r.stdout == ""
    for bad in (["--ess", "1024"], ["--ess", "7x"], ["--ess", "--ess"], ["--ess", "31", "--ess"], ["--ess", "-3"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr, bad
    for good in (["--ess"], ["--ess", "31"], ["--ess", "--loo"], ["--loo", "--ess", "0", "--block", "7"], ["--ess", "1023"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + good, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" not in r.stderr and "cannot read the default configuration" in r.stderr, good     # the option is taken


def test_core_arithmetic_against_long_double(tmp_path):
    """The header compiles as plain C++17 under g++ and the check passes: AR(1) series at phi = -0.5, 0, 0.8, 0.99, constant
    series, series with +-inf and NaN, pieces of 1, L - 1, L, L + 1 through the carry, the finish, the lag limit, R-hat."""
    exe = str(tmp_path / "ess_core_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tamcmc-c-_amd", "csrc"), "ess-core-check", "ESS_CHECK=" + exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok ess_core_check") and r.stdout.count("\n") == 1, (r.stdout[-3000:], r.stderr[-3000:])


def test_reference_on_known_sequences():
    """tests/ess_reference.py: the lag limit, the finish on hand-made lag products, white noise and AR(1) at their known
    effective sample sizes, and the R-hat of a shifted half."""
    import ess_reference as R
    assert [R.lag_limit(m, n) for m, n in ((0, 70000), (0, 4), (0, 5), (0, 6), (1, 100), (2, 100), (62, 100), (1023, 100), (1023, 101),
                                           (1023, 2000), (1022, 2000))] == [255, 3, 3, 5, 1, 3, 63, 99, 99, 1023, 1023]
    A = np.array([[4.0, 4.0, 4.0, 0.0, np.inf], [2.0, -3.9, 1.0, 1.0, 1.0], [1.0, 1.0, -2.0, 0.0, 0.0], [0.5, 0.5, 0.5, 0.0, 0.0],
                  [np.nan, 0.1, 3.0, 0.0, 0.0], [0.1, 0.1, 3.0, 0.0, 0.0]])
    tau, ess, cut = R.finish(A, 100)
    assert list(cut) == [4, 6, 2, 0, 0]
    assert tau[0] == -1.0 + 2.0 * (1.5 + 0.375) and tau[1] == 0.5 and ess[1] == 200.0 and tau[2] == 1.5
    assert np.isnan(tau[3]) and np.isnan(ess[4])
    n = 4000
    for phi, lo, hi in ((0.0, 0.8, 1.25), (0.8, 0.5, 2.0)):
        _, ess, cut, _ = R.ess_of_sequence(R.ar1(phi, n, 1.0, 1), 63)
        assert lo <= ess / (n * (1 - phi) / (1 + phi)) <= hi and cut < 64, (phi, ess, cut)
    _, ess, cut, _ = R.ess_of_sequence(R.ar1(0.99, n, 1.0, 1), 15)
    assert cut == 16
    _, ess, cut, _ = R.ess_of_sequence(R.ar1(-0.5, n, 1.0, 1), 63)
    assert n < ess <= n * np.log10(n)
    x = R.ar1(0.8, n, 1.0, 1)
    assert float(R.rhat(x[:, None])[0]) < 1.01
    x[n // 2:] += 3.0
    assert float(R.rhat(x[:, None])[0]) > 1.5
    assert np.isnan(R.rhat(np.ones((8, 1)))[0])
