"""The mode table's seismic indices (tamcmc_modetable_indices_*, tamcmc_modetable_index_terms, tamcmc_seismic_kernel_time;
include/tamcmc_accel_seismic.h, which tamcmc_accel.h includes), the part that needs no GPU: the symbols exist with the
declared prototypes, struct layout and kind codes, every entry point refuses a NULL handle before any device is touched and
leaves its outputs alone, the command-line tool knows the option, the header's plan equals the Python restatement's column
for column and coefficient bit for coefficient bit (and the restatement a plan written out by hand), and the shared plan and
arithmetic (tamcmc_seismic.h) hold on the CPU (tests/cpp/seismic_core_check.cpp, plain g++, built by csrc/Makefile's
seismic-core-check, and once more as a stand-alone binary under the address and undefined-behaviour sanitizers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import modetable_reference as MR
import seismic_reference as SR
import workloads as W
from support import tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tamcmc-c-_amd", "csrc")
NAMES = ["tamcmc_modetable_indices_enable", "tamcmc_modetable_indices_info", "tamcmc_modetable_index_terms", "tamcmc_seismic_kernel_time"]


def prototypes():
    txt = open(os.path.join(ROOT, "include", "tamcmc_accel_seismic.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(tamcmc_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
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
    assert sorted(protos) == sorted(NAMES) == sorted(accel_mod.capi.SEISMIC_EXPORTS)
    for n in NAMES:
        assert hasattr(lib, n), n
    mt = "tamcmc_modetable*"
    assert protos["tamcmc_modetable_indices_enable"] == [mt, "int32_t", "const double*", "tamcmc_seismic_info*"]
    assert protos["tamcmc_modetable_indices_info"] == [mt, "tamcmc_seismic_info*"]
    assert protos["tamcmc_modetable_index_terms"] == [mt, "int32_t", "int32_t", "int32_t*", "int32_t*", "int32_t*", "int32_t*", "double*", "double*"]
    assert protos["tamcmc_seismic_kernel_time"] == [mt, "double*", "int64_t*"]
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_seismic_info;", txt)
    assert m and " ".join(m.group(1).split()) == "int64_t n_base_cols, n_index_cols, n_radial, n_unassigned, n_base; double dnu_ref, eps_ref;"
    info = accel_mod.capi.SeismicInfo
    names = ["n_base_cols", "n_index_cols", "n_radial", "n_unassigned", "n_base", "dnu_ref", "eps_ref"]
    assert [f[0] for f in info._fields_] == names and C.sizeof(info) == 56
    assert [getattr(info, k).offset for k in names] == list(range(0, 56, 8))
    assert [f[1] for f in info._fields_] == [C.c_int64] * 5 + [C.c_double] * 2
    # the kind codes follow the table's thirteen, in the order of the Python names and of the reference module
    codes = dict(re.findall(r"#define TAMCMC_MODETABLE_([A-Z0-9_]+)\s+(\d+)", txt))
    assert [k.lower() for k, v in sorted(codes.items(), key=lambda kv: int(kv[1]))] == list(accel_mod.capi.SEISMIC_KINDS) == list(SR.KINDS)
    assert sorted(int(v) for v in codes.values()) == list(range(13, 26))
    assert accel_mod.ModeTable.KINDS == accel_mod.capi.MODETABLE_KINDS + accel_mod.capi.SEISMIC_KINDS == SR.ALL_KINDS
    assert SR.K["dnu_fit"] == 13 and SR.K["r10"] == 25
    for meth in ("enable_indices", "indices_info", "index_terms", "seismic_kernel_time"):
        assert callable(getattr(accel_mod.ModeTable, meth)), meth
    # tamcmc_accel.h brings the declarations in; the kernel's file includes the shared arithmetic under the pragma and has no
    # inline assembly, no atomics on memory and no cross-lane reduction
    assert '#include "tamcmc_accel_seismic.h"' in open(os.path.join(ROOT, "include", "tamcmc_accel.h")).read()
    hip = open(os.path.join(CSRC, "tamcmc_seismic.hip")).read()
    assert hip.index("#pragma clang fp contract(off)") < hip.index('#include "tamcmc_seismic.h"')
    assert "tm_seis_eval(" in hip and "asm" not in hip.lower() and "__shfl" not in hip and "fma(" not in hip
    hdr = open(os.path.join(CSRC, "tamcmc_seismic.h")).read()
    assert "fma(" not in hdr and "TM_HD inline double tm_seis_eval" in hdr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "tamcmc_seismic.o tamcmc_seismic_api.o" in mk and "resource-usage-seismic:" in mk and "seismic-core-check:" in mk


def test_null_handle_is_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(64, 7.0)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    i32 = np.full(8, 7, dtype=np.int32)
    ip = i32.ctypes.data_as(C.POINTER(C.c_int32))
    info = accel_mod.capi.SeismicInfo()
    info.n_base_cols, info.dnu_ref = 77, 7.5
    ms, n = C.c_double(-1.0), C.c_int64(-1)
    assert lib.tamcmc_modetable_indices_enable(None, 8, xp, C.byref(info)) == E
    assert lib.tamcmc_modetable_indices_enable(None, 8, None, None) == E
    assert lib.tamcmc_modetable_indices_info(None, C.byref(info)) == E and lib.tamcmc_modetable_indices_info(None, None) == E
    assert lib.tamcmc_modetable_index_terms(None, 0, 8, ip, ip, ip, ip, xp, xp) == E
    assert lib.tamcmc_modetable_index_terms(None, 300, 0, None, None, None, None, None, None) == E
    assert lib.tamcmc_seismic_kernel_time(None, C.byref(ms), C.byref(n)) == E
    assert lib.tamcmc_seismic_kernel_time(None, None, None) == E
    assert np.all(x == 7.0) and np.all(i32 == 7) and info.n_base_cols == 77 and info.dnu_ref == 7.5
    assert ms.value == -1.0 and n.value == -1


def test_tool_knows_the_option():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == ""
    assert "[--modes-indices]" in r.stderr and ".modes.indices" in r.stderr and ".modes.indices.cov" in r.stderr
    for bad in (["--modes-indices"], ["--modes", "--modes-indices", "--modes-indices"], ["--ess", "--modes-indices"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr, bad
    for good in (["--modes", "--modes-indices"], ["--modes-indices", "--modes", "0.16,0.5,0.84", "--modes-ess"], ["--modes", "--modes-rank", "15", "--modes-indices"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + good, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" not in r.stderr and "cannot read the default configuration" in r.stderr, good


def ladder_row(cols, dnu=100.0, eps=1.2, D0=1.0, n0=10):
    row = np.arange(len(cols), dtype=np.float64) + 0.5
    f = cols["kind"] == MR.K["freq"]
    l, n = cols["l"][f].astype(np.float64), cols["order"][f].astype(np.float64)
    row[f] = dnu * (n0 + n + l / 2.0 + eps) - l * (l + 1.0) * D0
    row[cols["kind"] == MR.K["amplitude"]] = 2.0
    return row


def test_reference_plan_on_a_hand_made_ladder():
    """The restatement by itself: counts, order and refusals on a ladder whose plan can be written down."""
    w = W.layout(2, 3, Nmax=5)
    cols = MR.layout(2, w["plength"])
    row = ladder_row(cols)
    p = SR.plan(cols, row)
    kinds = [SR.ALL_KINDS[k] for k in p["cols"]["kind"]]
    want = (["dnu_fit"] * 4 + ["epsilon", "numax"] + ["dnu_nl"] * 16 + ["d2nu"] * 12 + ["d02"] * 4 + ["d13"] * 4 + ["d01"] * 3 + ["d10"] * 3 +
            ["r02"] * 4 + ["r01"] * 3 + ["r13"] * 3 + ["r10"] * 3)           # (r13 at the top order would need the radial mode above it)
    assert kinds == want
    info = p["info"]
    assert info["n_base"] == 10 and info["n_radial"] == 5 and info["n_unassigned"] == 0 and abs(info["dnu_ref"] - 100.0) < 1e-9 and abs(info["eps_ref"] - 1.2) < 1e-9
    v = SR.evaluate(p["terms"], row[None, :])[0]
    for kind, val in (("dnu_fit", 100.0), ("epsilon", 1.2), ("dnu_nl", 100.0), ("d2nu", 0.0), ("d02", 6.0), ("d13", 10.0), ("d01", 2.0), ("d10", 2.0),
                      ("r02", 0.06), ("r13", 0.1), ("r01", 0.02), ("r10", 0.02), ("numax", 100.0 * (12 + 1.2))):
        got = v[np.array(kinds) == kind]
        assert got.size and np.all(np.abs(got - val) < 1e-9), (kind, got)
    assert list(p["cols"]["order"][np.array(kinds) == "d01"]) == [11, 12, 13] and list(p["cols"]["order"][np.array(kinds) == "d02"]) == [11, 12, 13, 14]
    ld = SR.evaluate(p["terms"], row[None, :], np.longdouble)[0]
    assert np.all(np.abs(ld - v) <= 10 * 2.0 ** -50 * SR.sensitivity(p["terms"], row[None, :])[0])
    f1 = np.flatnonzero((cols["kind"] == MR.K["freq"]) & (cols["l"] == 1))
    for shift, un in ((0.34, 0), (-0.34, 0), (0.36, 1), (-0.36, 1)):
        r = ladder_row(cols, D0=0.0)                # (u of an l = 1 mode is its order exactly)
        r[f1[2]] += shift * 100.0
        assert SR.plan(cols, r)["info"]["n_unassigned"] == un, shift
    r = row.copy()
    r[f1[2]] = r[f1[3]] - 10.0
    assert SR.plan(cols, r)["info"]["n_unassigned"] == 2
    f0 = np.flatnonzero((cols["kind"] == MR.K["freq"]) & (cols["l"] == 0))
    r = row.copy()
    r[f0[3:]] += 100.0
    for bad in (r, ladder_row(MR.layout(2, W.layout(2, 1, Nmax=2)["plength"]))):
        try:
            SR.plan(cols if bad is r else MR.layout(2, W.layout(2, 1, Nmax=2)["plength"]), bad)
        except SR.Refused:
            continue
        raise AssertionError("a refusal is missing")


def test_header_plan_equals_the_restatement(tmp_path):
    """The header's plan (printed by the core check's binary, built from tamcmc_seismic.h) equals the numpy restatement's on
    the same ladder, column for column and coefficient bit for coefficient bit: lmax = 0 ... 3 with 3, 4, 5 radial orders,
    lmax = 3 with 12, lmax = 0 with 70; two radial orders are refused by both."""
    exe = str(tmp_path / "seismic_core_check")
    r = subprocess.run(["make", "-s", "-C", CSRC, "seismic-core-check", "SEISMIC_CHECK=" + exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    fl = float.fromhex
    for lmax, Nmax in [(l, n) for l in range(4) for n in (3, 4, 5)] + [(3, 12), (0, 70)]:
        cols = MR.layout(2, W.layout(2, lmax, Nmax=Nmax)["plength"])
        p = SR.plan(cols, ladder_row(cols))
        r = subprocess.run([exe, "plan", str(Nmax), str(lmax)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (lmax, Nmax, r.stderr)
        lines = [line.split() for line in r.stdout.splitlines()]
        info = p["info"]
        assert lines[0][0] == "info" and [int(t) for t in lines[0][1:5]] == [info["n_index_cols"], info["n_radial"], info["n_unassigned"], info["n_base"]]
        assert fl(lines[0][5]) == info["dnu_ref"] and fl(lines[0][6]) == info["eps_ref"]
        assert len(lines) == 1 + len(p["terms"])
        for tok, c, t in zip(lines[1:], p["cols"], p["terms"]):
            assert [int(v) for v in tok[:5]] == [c["kind"], c["order"], c["l"], t["n_num"], t["n_den"]] and fl(tok[5]) == t["offset"], (lmax, Nmax, tok[:6])
            assert [int(v) for v in tok[6::3]] == list(t["src"]) and [int(v) for v in tok[7::3]] == list(t["wsrc"])
            assert [fl(v) for v in tok[8::3]] == list(t["coef"]), (lmax, Nmax, tok[:6])
    r = subprocess.run([exe, "plan", "2", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "refused\n"


def test_core_arithmetic(tmp_path):
    """The header compiles as plain C++17 under g++ and the check passes (what it covers: its own header comment).  Then once
    more built with -fsanitize=address,undefined and run as a stand-alone binary."""
    for name, flags in (("seismic_core_check", ""), ("seismic_core_check_san", "-fsanitize=address,undefined -fno-sanitize-recover=undefined")):
        exe = str(tmp_path / name)
        r = subprocess.run(["make", "-s", "-C", CSRC, "seismic-core-check", "SEISMIC_CHECK=" + exe, "CHECKFLAGS=" + flags],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        print(r.stdout)
        assert r.returncode == 0 and r.stdout.startswith("ok seismic_core_check") and r.stdout.count("\n") == 1, (r.stdout[-3000:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
