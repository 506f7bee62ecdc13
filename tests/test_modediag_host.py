"""The mode table's diagnostics (tamcmc_modediag_*, include/tamcmc_accel.h), the part that needs no GPU: the symbols exist
with the declared prototypes and struct layout, every entry point refuses NULL handles and arguments before any device is
touched and leaves its outputs alone, the command-line tool knows the two options, and the shared arithmetic
(tamcmc_modediag.h: the lag kernel's tile / halo walk and the covariance kernel's strip walk against the plain serial loops,
the correlation finish, the totals) holds on the CPU (tests/cpp/modediag_core_check.cpp, plain g++, built by csrc/Makefile's
modediag-core-check, and once more as a stand-alone binary under the address and undefined-behaviour sanitizers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from support import tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tamcmc-c-_amd", "csrc")
NAMES = ["tamcmc_modediag_ess", "tamcmc_modediag_acov", "tamcmc_modediag_cov", "tamcmc_modediag_corr", "tamcmc_modediag_kernel_time"]


def prototypes():
    txt = open(os.path.join(ROOT, "include", "tamcmc_accel.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(tamcmc_modediag_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            a = re.sub(r"\s*\b[A-Za-z_]\w*$", "", a) if not a.endswith("*") else a      # drop the parameter's name
            types.append(a.replace(" *", "*"))
        out[name] = types
    return out, txt


def test_symbols_and_signatures(accel_mod):
    lib = accel_mod.load_library()
    protos, txt = prototypes()
    assert sorted(protos) == sorted(NAMES)
    for n in NAMES:
        assert hasattr(lib, n) and n in accel_mod.capi.EXPORTS, n
    mt = "tamcmc_modetable*"
    assert protos["tamcmc_modediag_ess"] == [mt, "int32_t", "tamcmc_modediag_totals*"] + ["double*"] * 4 + ["int32_t*"]
    assert protos["tamcmc_modediag_acov"] == [mt, "double*"]
    assert protos["tamcmc_modediag_cov"] == protos["tamcmc_modediag_corr"] == [mt, "int32_t", "const int32_t*", "double*"]
    assert protos["tamcmc_modediag_kernel_time"] == [mt, "double*", "int64_t*"]
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_modediag_totals;", txt)
    assert m and " ".join(m.group(1).split()) == ("int64_t n_used, lag; double min_ess, max_rhat; "
                                                   "int64_t col_min_ess, col_max_rhat, n_truncated, n_constant, n_rhat_high;")
    tot = accel_mod.capi.ModeDiagTotals
    names = ["n_used", "lag", "min_ess", "max_rhat", "col_min_ess", "col_max_rhat", "n_truncated", "n_constant", "n_rhat_high"]
    assert [f[0] for f in tot._fields_] == names and C.sizeof(tot) == 72
    assert [getattr(tot, k).offset for k in names] == list(range(0, 72, 8))
    assert [f[1] for f in tot._fields_] == [C.c_int64] * 2 + [C.c_double] * 2 + [C.c_int64] * 5
    macros = dict(re.findall(r"#define (TAMCMC_MODEDIAG_[A-Z_]+)\s+(\d+)", txt))
    assert macros == {"TAMCMC_MODEDIAG_MAX_LAG": "1023", "TAMCMC_MODEDIAG_MAX_COLS": "1024"}
    assert accel_mod.capi.MODEDIAG_MAX_LAG == 1023 and accel_mod.capi.MODEDIAG_MAX_COLS == 1024
    for meth in ("ess", "acov", "cov", "corr", "diag_kernel_time"):
        assert callable(getattr(accel_mod.ModeTable, meth)), meth
    # the header states the bytes; the kernels' file includes the shared arithmetic under the pragma
    full = open(os.path.join(ROOT, "include", "tamcmc_accel.h")).read()
    assert "8 (L + 4) n_cols + 4 n_cols bytes" in full and "8 n_sel^2 + 4 n_sel bytes" in full
    hip = open(os.path.join(CSRC, "tamcmc_modediag.hip")).read()
    assert hip.index("#pragma clang fp contract(off)") < hip.index('#include "tamcmc_ess.h"') < hip.index('#include "tamcmc_modediag.h"')
    assert "mfma" not in hip.lower().replace("no mfma", "") and "atomic" not in hip.lower().replace("no atomics", "")


def test_null_handle_is_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(8, 7.0)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    i32 = np.full(8, 7, dtype=np.int32)
    ip = i32.ctypes.data_as(C.POINTER(C.c_int32))
    t = accel_mod.capi.ModeDiagTotals()
    t.n_used, t.min_ess = 77, 7.5
    ms, n = C.c_double(-1.0), C.c_int64(-1)
    assert lib.tamcmc_modediag_ess(None, 0, C.byref(t), xp, xp, xp, xp, ip) == E
    assert lib.tamcmc_modediag_ess(None, 0, None, None, None, None, None, None) == E
    assert lib.tamcmc_modediag_ess(None, 5000, C.byref(t), xp, xp, xp, xp, ip) == E
    assert lib.tamcmc_modediag_acov(None, xp) == E and lib.tamcmc_modediag_acov(None, None) == E
    for fn in (lib.tamcmc_modediag_cov, lib.tamcmc_modediag_corr):
        assert fn(None, 2, ip, xp) == E and fn(None, 2, None, xp) == E and fn(None, 0, None, None) == E
    assert lib.tamcmc_modediag_kernel_time(None, C.byref(ms), C.byref(n)) == E
    assert lib.tamcmc_modediag_kernel_time(None, None, None) == E
    assert np.all(x == 7.0) and np.all(i32 == 7) and t.n_used == 77 and t.min_ess == 7.5
    assert ms.value == -1.0 and n.value == -1


def test_tool_knows_the_options():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == ""
    assert "[--modes [q1,q2,...]] [--modes-ess [L]] [--modes-corr]" in r.stderr
    assert "col kind mult order l m param_index ess tau mcse rhat cut" in r.stderr and ".modes.ess" in r.stderr and ".modes.corr" in r.stderr
    assert "col kind mult order l m param_index mean sd min max" in r.stderr
    for bad in (["--modes-ess"], ["--modes-corr"], ["--modes-ess", "15"], ["--modes", "--modes-ess", "1024"], ["--modes", "--modes-ess", "x"],
                ["--modes", "--modes-ess", "15x"], ["--modes", "--modes-ess", "--modes-ess"], ["--modes", "--modes-ess", "3", "--modes-ess", "3"],
                ["--modes", "--modes-corr", "--modes-corr"], ["--modes", "--modes", "--modes-ess"], ["--ess", "--modes-corr"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr, bad
    for good in (["--modes", "--modes-ess"], ["--modes-ess", "--modes"], ["--modes", "--modes-ess", "0"], ["--modes", "--modes-ess", "1023"],
                 ["--modes", "0.16,0.5", "--modes-ess", "15", "--modes-corr"], ["--modes-corr", "--modes", "--thin", "2"],
                 ["--modes-ess", "255", "--modes-corr", "--ess", "--modes", ".5"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + good, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" not in r.stderr and "cannot read the default configuration" in r.stderr, good


def test_core_arithmetic(tmp_path):
    """The header compiles as plain C++17 under g++ and the check passes: the lag kernel's walk fed tile by tile and the
    covariance kernel's strip walk against the plain serial loops, bit for bit (n around every tile edge up to 3 T + 1, L in
    {1, 3, 15, 17, 255, 1023} and n - 1, +-inf and NaN), the correlation finish on hand cases, the totals.  Then once more built
    with -fsanitize=address,undefined and run as a stand-alone binary."""
    for name, flags in (("modediag_core_check", ""), ("modediag_core_check_san", "-fsanitize=address,undefined -fno-sanitize-recover=undefined")):
        exe = str(tmp_path / name)
        r = subprocess.run(["make", "-s", "-C", CSRC, "modediag-core-check", "MODEDIAG_CHECK=" + exe, "CHECKFLAGS=" + flags],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        print(r.stdout)
        assert r.returncode == 0 and r.stdout.startswith("ok modediag_core_check") and r.stdout.count("\n") == 1, (r.stdout[-3000:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
