"""LOO-PIT of a stored chain (tamcmc_summary_loo_pit_*, include/tamcmc_accel.h), the part that needs no GPU: the symbols
exist with the declared prototypes and struct layout, a NULL handle is refused before any device is touched, the
command-line tool knows the option, and the shared arithmetic (tamcmc_loopit.h: the tie-mean rule, the clamped search, the
four sums) agrees on the CPU with a long-double brute force (tests/cpp/loopit_core_check.cpp, plain g++, built by
csrc/Makefile's loopit-core-check)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from summary_support import prototypes
from support import tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tamcmc_summary_loo_pit_begin", "tamcmc_summary_loo_pit_result", "tamcmc_summary_loo_pit_kernel_time"]
FIELDS = ["n_used", "n_rejected", "ks_D", "min_log_sf", "min_log_cdf", "min_is_ess", "bin_min_log_sf", "bin_min_log_cdf",
          "bin_min_is_ess", "pit_hist"]


def test_symbols_and_signatures(accel_mod):
    lib = accel_mod.load_library()
    protos, txt = prototypes()
    for n in NAMES:
        assert hasattr(lib, n) and n in accel_mod.capi.EXPORTS, n
    assert protos["tamcmc_summary_loo_pit_begin"] == ["tamcmc_summary*"]
    assert protos["tamcmc_summary_loo_pit_result"] == ["tamcmc_summary*", "tamcmc_summary_loo_pit_totals*"] + ["double*"] * 5
    assert protos["tamcmc_summary_loo_pit_kernel_time"] == ["tamcmc_summary*", "double*", "int64_t*"]
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_summary_loo_pit_totals;", txt)
    assert m and " ".join(m.group(1).split()) == \
        ("int64_t n_used, n_rejected; double ks_D, min_log_sf, min_log_cdf, min_is_ess; "
         "int64_t bin_min_log_sf, bin_min_log_cdf, bin_min_is_ess; int64_t pit_hist[TAMCMC_SUMMARY_PIT_CELLS];")
    t = accel_mod.capi.SummaryLooPitTotals
    assert [f[0] for f in t._fields_] == FIELDS
    kinds = dict(t._fields_)
    for k, name in enumerate(FIELDS):                        # every field starts on the next eight bytes, in the header's order
        assert getattr(t, name).offset == 8 * k, name
        if name != "pit_hist":
            assert kinds[name] is (C.c_double if name in ("ks_D", "min_log_sf", "min_log_cdf", "min_is_ess") else C.c_int64), name
    assert C.sizeof(t) == (9 + 20) * 8
    assert accel_mod.Summary.LOO_PIT_ARRAYS == ("loo_pit", "loo_log_cdf", "loo_log_sf", "is_ess", "log_wsum")
    for meth in ("loo_pit_begin", "loo_pit_result", "loo_pit_kernel_time", "loo"):
        assert callable(getattr(accel_mod.Summary, meth))
    # what LOO mode exposed before stays as it is
    assert protos["tamcmc_summary_loo_result"] == ["tamcmc_summary*", "tamcmc_summary_loo_totals*", "double*", "double*", "double*", "int32_t*"]
    assert C.sizeof(accel_mod.capi.SummaryLooTotals) == 64 and accel_mod.Summary.LOO_ARRAYS == ("elpd_loo", "pareto_k", "cutoff")
    # the kernels' file is its own, and the header's constants are the library's
    h = open(os.path.join(ROOT, "tamcmc-c-_amd", "csrc", "tamcmc_loopit.h")).read()
    assert "#define TM_LOOPIT_UNROLL TM_LOO_UNROLL" in h and "TM_LOOPIT_NSTATE" in h
    assert "tamcmc_loopit" not in open(os.path.join(ROOT, "tamcmc-c-_amd", "csrc", "tamcmc_loo.hip")).read()


def test_null_handle_is_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(8, 7.0)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    t = accel_mod.capi.SummaryLooPitTotals()
    t.n_used = 77
    ms, n = C.c_double(-1.0), C.c_int64(-1)
    assert lib.tamcmc_summary_loo_pit_begin(None) == E
    assert lib.tamcmc_summary_loo_pit_result(None, C.byref(t), xp, xp, xp, xp, xp) == E
    assert lib.tamcmc_summary_loo_pit_result(None, None, None, None, None, None, None) == E
    assert lib.tamcmc_summary_loo_pit_kernel_time(None, C.byref(ms), C.byref(n)) == E
    assert np.all(x == 7.0) and t.n_used == 77 and ms.value == -1.0 and n.value == -1


def test_tool_knows_the_option():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "[--loo-pit]" in r.stderr and ".loopit" in r.stderr and r.stdout == ""
    assert "x loo_pit loo_log_cdf loo_log_sf is_ess pareto_k" in r.stderr
    r = subprocess.run([exe, "a", "b", "c", "d", "e", "--loo-pit", "--thin"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr
    for good in (["--loo-pit"], ["--loo", "--loo-pit"], ["--loo-pit", "--ess", "31", "--block", "7"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + good, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" not in r.stderr and "cannot read the default configuration" in r.stderr, good   # the option is taken


def test_core_arithmetic_against_long_double(tmp_path):
    """The header compiles as plain C++17 under g++ and the check passes: the tie-mean rule on runs of 1, 2, 7, "all equal"
    and a tie with the cutoff; the clamped search on columns of 1, 2, 3, 63, 64, 65, 2047 and 2048 slots (found, not found
    below, between and above, no probe outside the column); the four sums with -inf terms."""
    exe = str(tmp_path / "loopit_core_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tamcmc-c-_amd", "csrc"), "loopit-core-check", "LOOPIT_CHECK=" + exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok loopit_core_check") and r.stdout.count("\n") == 1, (r.stdout[-3000:], r.stderr[-3000:])
