"""The mode table's rank-normalised diagnostics (tamcmc_moderank_*, include/tamcmc_accel.h), the part that needs no GPU: the
symbols exist with the declared prototypes, struct layout and macros, every entry point refuses a NULL handle before any
device is touched and leaves its outputs alone, the command-line tool knows the option, and the shared arithmetic
(tamcmc_moderank.h: the sort kernel's tile and wide stages against std::sort, the two binary searches against the counts,
z's antisymmetry, monotonicity and accuracy through erfcl, the totals) holds on the CPU (tests/cpp/moderank_core_check.cpp,
plain g++, built by csrc/Makefile's moderank-core-check, and once more as a stand-alone binary under the address and
undefined-behaviour sanitizers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from support import tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tamcmc-c-_amd", "csrc")
NAMES = ["tamcmc_moderank_diag", "tamcmc_moderank_acov", "tamcmc_moderank_series", "tamcmc_moderank_kernel_time"]


def prototypes():
    txt = open(os.path.join(ROOT, "include", "tamcmc_accel.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(tamcmc_moderank_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
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
    assert protos["tamcmc_moderank_diag"] == [mt, "int32_t", "int32_t", "const int32_t*", "int64_t", "tamcmc_moderank_totals*", "double*", "int32_t*"]
    assert protos["tamcmc_moderank_acov"] == [mt, "int32_t", "double*"]
    assert protos["tamcmc_moderank_series"] == [mt, "int32_t", "int64_t*", "int64_t*", "double*", "double*", "double*"]
    assert protos["tamcmc_moderank_kernel_time"] == [mt, "double*", "int64_t*"]
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_moderank_totals;", txt)
    assert m and " ".join(m.group(1).split()) == ("int64_t n_used, lag; double min_ess_bulk, min_ess_tail, max_rhat; "
                                                   "int64_t col_min_ess_bulk, col_min_ess_tail, col_max_rhat, n_truncated, n_constant, n_rhat_high;")
    tot = accel_mod.capi.ModeRankTotals
    names = ["n_used", "lag", "min_ess_bulk", "min_ess_tail", "max_rhat", "col_min_ess_bulk", "col_min_ess_tail", "col_max_rhat", "n_truncated",
             "n_constant", "n_rhat_high"]
    assert [f[0] for f in tot._fields_] == names and C.sizeof(tot) == 88
    assert [getattr(tot, k).offset for k in names] == list(range(0, 88, 8))
    assert [f[1] for f in tot._fields_] == [C.c_int64] * 2 + [C.c_double] * 3 + [C.c_int64] * 6
    macros = dict(re.findall(r"#define (TAMCMC_MODERANK_[A-Z_]+)\s+(\d+)", txt))
    assert macros == {"TAMCMC_MODERANK_NOUT": "8", "TAMCMC_MODERANK_NSERIES": "4"}
    assert accel_mod.capi.MODERANK_NOUT == 8 == len(accel_mod.capi.MODERANK_OUT) and accel_mod.capi.MODERANK_NSERIES == 4 == len(accel_mod.capi.MODERANK_SERIES)
    for meth in ("rank_diag", "rank_acov", "rank_series", "rank_kernel_time"):
        assert callable(getattr(accel_mod.ModeTable, meth)), meth
    # the header states the bytes of a column and that the ESS is the single-chain one; the kernels' file includes the shared
    # arithmetic under the pragma; capi's byte count is the header's
    full = open(os.path.join(ROOT, "include", "tamcmc_accel.h")).read()
    assert "16 P + 32 (n + L + 5) + 44 bytes" in full and "NOT Stan's multi-chain" in full
    assert accel_mod.capi.moderank_col_bytes(1100, 255) == 16 * 2048 + 32 * (1100 + 255 + 5) + 44
    assert accel_mod.capi.moderank_col_bytes(4, 3) == 16 * 4 + 32 * 12 + 44 and accel_mod.capi.moderank_col_bytes(2049, 1) == 16 * 4096 + 32 * 2055 + 44
    hip = open(os.path.join(CSRC, "tamcmc_moderank.hip")).read()
    assert hip.index("#pragma clang fp contract(off)") < hip.index('#include "tamcmc_ess.h"') < hip.index('#include "tamcmc_moderank.h"')
    low = hip.lower()
    assert "mfma" not in low.replace("no\n// mfma", "").replace("no mfma", "") and "atomic" not in low.replace("no atomics", "") and "asm" not in low
    assert "tamcmc_modediag_lag_kernel" not in hip and "tme_finish" not in hip          # the lag and finish kernels are not copied


def test_null_handle_is_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(64, 7.0)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    i32 = np.full(8, 7, dtype=np.int32)
    ip = i32.ctypes.data_as(C.POINTER(C.c_int32))
    i64 = np.full(8, 7, dtype=np.int64)
    lp = i64.ctypes.data_as(C.POINTER(C.c_int64))
    t = accel_mod.capi.ModeRankTotals()
    t.n_used, t.min_ess_bulk = 77, 7.5
    ms, n = C.c_double(-1.0), C.c_int64(-1)
    assert lib.tamcmc_moderank_diag(None, 0, 2, ip, 0, C.byref(t), xp, ip) == E
    assert lib.tamcmc_moderank_diag(None, 0, 2, None, 0, None, None, None) == E
    assert lib.tamcmc_moderank_diag(None, 5000, 2, None, -1, C.byref(t), xp, ip) == E
    assert lib.tamcmc_moderank_acov(None, 0, xp) == E and lib.tamcmc_moderank_acov(None, 9, None) == E
    assert lib.tamcmc_moderank_series(None, 0, lp, lp, xp, xp, xp) == E and lib.tamcmc_moderank_series(None, -1, None, None, None, None, None) == E
    assert lib.tamcmc_moderank_kernel_time(None, C.byref(ms), C.byref(n)) == E
    assert lib.tamcmc_moderank_kernel_time(None, None, None) == E
    assert np.all(x == 7.0) and np.all(i32 == 7) and np.all(i64 == 7) and t.n_used == 77 and t.min_ess_bulk == 7.5
    assert ms.value == -1.0 and n.value == -1


def test_tool_knows_the_option():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == ""
    assert "[--modes-rank [L]]" in r.stderr and ".modes.rank" in r.stderr
    assert "col kind mult order l m param_index ess_bulk ess_tail rhat" in r.stderr
    for bad in (["--modes-rank"], ["--modes-rank", "15"], ["--modes", "--modes-rank", "1024"], ["--modes", "--modes-rank", "x"],
                ["--modes", "--modes-rank", "15x"], ["--modes", "--modes-rank", "--modes-rank"], ["--modes", "--modes-rank", "3", "--modes-rank", "3"],
                ["--modes-ess", "--modes-rank"], ["--ess", "--modes-rank"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr, bad
    for good in (["--modes", "--modes-rank"], ["--modes-rank", "--modes"], ["--modes", "--modes-rank", "0"], ["--modes", "--modes-rank", "1023"],
                 ["--modes", "0.16,0.5", "--modes-rank", "15", "--modes-ess", "--modes-corr"], ["--modes-rank", "255", "--ess", "--modes", ".5"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + good, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" not in r.stderr and "cannot read the default configuration" in r.stderr, good


def test_core_arithmetic(tmp_path):
    """The header compiles as plain C++17 under g++ and the check passes (what it covers: its own header comment).  Then once
    more built with -fsanitize=address,undefined and run as a stand-alone binary."""
    for name, flags in (("moderank_core_check", ""), ("moderank_core_check_san", "-fsanitize=address,undefined -fno-sanitize-recover=undefined")):
        exe = str(tmp_path / name)
        r = subprocess.run(["make", "-s", "-C", CSRC, "moderank-core-check", "MODERANK_CHECK=" + exe, "CHECKFLAGS=" + flags],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        print(r.stdout)
        assert r.returncode == 0 and r.stdout.startswith("ok moderank_core_check") and r.stdout.count("\n") == 1, (r.stdout[-3000:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
