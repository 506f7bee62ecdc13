"""Posterior summaries (tamcmc_summary_*, include/tamcmc_accel.h), the part that needs no GPU: the symbols exist with the
declared signatures, bad arguments are refused before any device is touched, and the command-line tool answers."""
import ctypes as C
import re
import subprocess

import numpy as np

from summary_support import prototypes
from support import tool

NAMES = ["tamcmc_summary_create", "tamcmc_summary_push", "tamcmc_summary_push_device", "tamcmc_summary_result",
         "tamcmc_summary_reset", "tamcmc_summary_destroy"]


def test_symbols_and_signatures(accel_mod):
    lib = accel_mod.load_library()
    protos, txt = prototypes()
    for n in NAMES:
        assert hasattr(lib, n) and n in accel_mod.capi.EXPORTS, n
    assert protos["tamcmc_summary_create"] == ["tamcmc_summary**", "tamcmc_ctx*", "int32_t"]
    assert protos["tamcmc_summary_push"] == ["tamcmc_summary*", "int32_t", "int32_t", "const double*", "double*", "int32_t*"]
    assert protos["tamcmc_summary_push_device"] == ["tamcmc_summary*", "int32_t", "int32_t", "const double*", "double*", "int32_t*"]
    assert protos["tamcmc_summary_result"] == ["tamcmc_summary*", "tamcmc_summary_totals*"] + ["double*"] * 7
    assert protos["tamcmc_summary_reset"] == ["tamcmc_summary*"] and protos["tamcmc_summary_destroy"] == ["tamcmc_summary*"]
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_summary_totals;", txt)
    assert m and " ".join(m.group(1).split()) == "int64_t n_used, n_rejected; double lppd_total, p_waic, waic;"
    t = accel_mod.capi.SummaryTotals
    assert [f[0] for f in t._fields_] == ["n_used", "n_rejected", "lppd_total", "p_waic", "waic"] and C.sizeof(t) == 40
    assert accel_mod.Summary is accel_mod.capi.Summary


def test_bad_arguments_are_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    dp = C.POINTER(C.c_double)
    x = np.ones(8)
    xp = x.ctypes.data_as(dp)
    st = np.zeros(8, dtype=np.int32)
    sp = st.ctypes.data_as(C.POINTER(C.c_int32))
    h = C.c_void_p(0x1234)                    # must come back cleared
    assert lib.tamcmc_summary_create(None, None, 0) == E
    assert lib.tamcmc_summary_create(C.byref(h), None, 0) == E and not h.value
    assert lib.tamcmc_summary_create(C.byref(h), None, -1) == E
    assert lib.tamcmc_summary_push(None, 1, 8, xp, xp, sp) == E
    assert lib.tamcmc_summary_push(None, 0, 8, xp, None, None) == E
    assert lib.tamcmc_summary_push(None, -3, 8, None, None, None) == E
    assert lib.tamcmc_summary_push_device(None, 1, 8, None, None, None) == E
    t = accel_mod.capi.SummaryTotals()
    assert lib.tamcmc_summary_result(None, C.byref(t), xp, xp, xp, xp, xp, xp, xp) == E
    assert lib.tamcmc_summary_result(None, None, None, None, None, None, None, None, None) == E
    assert lib.tamcmc_summary_reset(None) == E
    assert lib.tamcmc_summary_profile(None, 1) == E
    n = C.c_int64()
    assert lib.tamcmc_summary_kernel_time(None, xp, C.byref(n)) == E
    assert lib.tamcmc_summary_destroy(None) == 0          # like tamcmc_ctx_destroy / free


def test_tool_usage_and_version():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr and "--thin" in r.stderr and r.stdout == ""
    r = subprocess.run([exe, "a", "b", "c", "d", "e", "--thin"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr
    r = subprocess.run([exe, "a", "b", "c", "d", "e", "--thin", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr
    r = subprocess.run([exe, "version"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "tamcmc_accel" in r.stdout and "chainsummary_hip" in r.stdout
