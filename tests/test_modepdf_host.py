"""The mode table's histograms, shortest intervals and pair densities (tamcmc_modepdf_*; include/tamcmc_accel_pdf.h, which
tamcmc_accel.h includes), the part that needs no GPU: the symbols exist with the declared prototypes and constants, every
entry point refuses a NULL handle before any device is touched and leaves its outputs alone, the command-line tool knows the
three options and refuses them without --modes or with a bad value, the numpy restatement agrees with itself on cases that
can be written down, and the shared arithmetic (tamcmc_modepdf.h) holds on the CPU (tests/cpp/modepdf_core_check.cpp, plain
g++, built by csrc/Makefile's modepdf-core-check, and once more as a stand-alone binary under the address and
undefined-behaviour sanitizers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import modepdf_reference as PR
from support import tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tamcmc-c-_amd", "csrc")
NAMES = ["tamcmc_modepdf_hist", "tamcmc_modepdf_hpd", "tamcmc_modepdf_hist2d", "tamcmc_modepdf_kernel_time"]


def prototypes():
    txt = open(os.path.join(ROOT, "include", "tamcmc_accel_pdf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(tamcmc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
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
    assert sorted(protos) == sorted(NAMES) == sorted(accel_mod.capi.PDF_EXPORTS)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n not in accel_mod.capi.EXPORTS
    mt, i32, i64, cd, ci = "tamcmc_modetable*", "int32_t", "int64_t", "const double*", "const int32_t*"
    assert protos["tamcmc_modepdf_hist"] == [mt, i32, i32, ci, cd, cd, "int64_t*", "int64_t*", "int64_t*", "double*", "int32_t*"]
    assert protos["tamcmc_modepdf_hpd"] == [mt, i32, cd, i32, ci, i64, "int64_t*", "int64_t*", "double*", "double*"]
    assert protos["tamcmc_modepdf_hist2d"] == [mt, i32, i32, ci, cd, cd, i32, cd, "int64_t*", "int64_t*", "int64_t*", "int32_t*"]
    assert protos["tamcmc_modepdf_kernel_time"] == [mt, "double*", "int64_t*"]
    consts = dict(re.findall(r"#define TAMCMC_MODEPDF_([A-Z0-9_]+)\s+(\d+)", txt))
    assert int(consts["MAX_BINS"]) == 4096 == accel_mod.capi.MODEPDF_MAX_BINS == PR.MAX_BINS
    assert int(consts["MAX_BINS2D"]) == 128 == accel_mod.capi.MODEPDF_MAX_BINS2D == PR.MAX_BINS2D
    assert int(consts["RANGE"]) == 1 == accel_mod.capi.MODEPDF_RANGE == PR.RANGE
    assert int(consts["MAX_PAIRS"]) == 1024 and int(consts["MAX_MASS"]) == 8
    for meth in ("hist", "hist_edges", "hpd", "hist2d", "pdf_kernel_time"):
        assert callable(getattr(accel_mod.ModeTable, meth)), meth
    # tamcmc_accel.h brings the declarations in and declares none of them itself; the edges are stated as no part of the rule
    acc_h = open(os.path.join(ROOT, "include", "tamcmc_accel.h")).read()
    assert '#include "tamcmc_accel_pdf.h"' in acc_h and "int tamcmc_modepdf_" not in acc_h
    assert "NOT part of the count rule" in open(os.path.join(ROOT, "include", "tamcmc_accel_pdf.h")).read()
    # the kernels' file includes the shared arithmetic under the pragma; no inline assembly, no fma, no atomics on device memory
    hip = open(os.path.join(CSRC, "tamcmc_modepdf.hip")).read()
    assert hip.index("#pragma clang fp contract(off)") < hip.index('#include "tamcmc_modepdf.h"')
    assert "tmp_class(" in hip and "tmp_before(" in hip and "asm" not in hip.lower() and "fma(" not in hip
    hdr = open(os.path.join(CSRC, "tamcmc_modepdf.h")).read()
    assert "fma(" not in hdr and "TMP_FN long long tmp_class" in hdr and "TMP_FN bool tmp_before" in hdr
    for k, v in (("MAX_BINS", 4096), ("MAX_BINS2D", 128), ("RANGE", 1), ("MAX_PAIRS", 1024), ("MAX_MASS", 8)):
        assert re.search(r"#define TM_PDF_%s %d\b" % (k, v), hdr), k
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "tamcmc_modepdf.o tamcmc_modepdf_api.o" in mk and "resource-usage-modepdf:" in mk and "modepdf-core-check:" in mk
    obj = open(os.path.join(CSRC, "tamcmc_modetable_obj.h")).read()
    assert "tamcmc_modepdf_*" in obj and re.search(r"struct TmMtPdf \{\s*TmMtBuf scratch;", obj) and re.search(r"\bTmMtPdf pdf;", obj)
    # every feature's file reaches its own member struct of the object and no other's (a field is reached through its member or
    # through the member's type alone); the table's file reaches the four through their hooks alone
    owners = {"modediag": "diag", "moderank": "rank", "seismic": "seis", "modepdf": "pdf"}
    foreign = r"(->|\.)\s*(%s)\b|\bTmMt(%s)\b"
    for feature, own in owners.items():
        api = open(os.path.join(CSRC, "tamcmc_%s_api.cpp" % feature)).read()
        others = [m for m in owners.values() if m != own]
        if feature == "seismic":                    # indices_enable asks the two whose buffers are sized by n_cols, and nothing else of them
            api = api.replace("mt->diag.sized_by_columns()", "").replace("mt->rank.sized_by_columns()", "")
        assert re.search(r"(->|\.)\s*%s\b" % own, api), feature
        assert not re.search(foreign % ("|".join(others), "|".join(m.capitalize() for m in others)), api), feature
    api = open(os.path.join(CSRC, "tamcmc_modetable_api.cpp")).read()
    named = re.findall(r"(?:->|\.)\s*(?:diag|rank|seis|pdf)\b\s*(\.\s*\w+\s*\(\s*\))?", api)
    assert len(named) == 12 and set(re.sub(r"\s", "", n) for n in named) == {".invalidate()", ".clear()", ".release()"}
    assert not re.search(r"\bTmMt(Diag|Rank|Seis|Pdf)\b", api) and "acov_valid" not in api and "sized_by_columns" not in api


def test_null_handle_is_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(64, 7.0)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    i32 = np.full(8, 7, dtype=np.int32)
    ip = i32.ctypes.data_as(C.POINTER(C.c_int32))
    i64 = np.full(64, 7, dtype=np.int64)
    lp = i64.ctypes.data_as(C.POINTER(C.c_int64))
    ms, n = C.c_double(-1.0), C.c_int64(-1)
    assert lib.tamcmc_modepdf_hist(None, 4, 1, ip, xp, xp, lp, lp, lp, xp, ip) == E
    assert lib.tamcmc_modepdf_hist(None, 4, 1, None, None, None, None, None, None, None, None) == E
    assert lib.tamcmc_modepdf_hpd(None, 1, xp, 1, ip, 0, lp, lp, xp, xp) == E
    assert lib.tamcmc_modepdf_hpd(None, 0, None, 0, None, -1, None, None, None, None) == E
    assert lib.tamcmc_modepdf_hist2d(None, 4, 1, ip, xp, xp, 1, xp, lp, lp, lp, ip) == E
    assert lib.tamcmc_modepdf_hist2d(None, 4, 1, None, None, None, 0, None, None, None, None, None) == E
    assert lib.tamcmc_modepdf_kernel_time(None, C.byref(ms), C.byref(n)) == E
    assert lib.tamcmc_modepdf_kernel_time(None, None, None) == E
    assert np.all(x == 7.0) and np.all(i32 == 7) and np.all(i64 == 7) and ms.value == -1.0 and n.value == -1


def test_tool_knows_the_options():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == ""
    for text in ("[--modes-hist [N]]", "[--modes-hpd m1[,m2,...]]", "[--modes-pairs c1:c2[,c3:c4,...] [N]]", ".modes.hist", ".modes.hpd", ".modes.pairs"):
        assert text in r.stderr, text
    bad = (["--modes-hist"], ["--modes-hpd", "0.68"], ["--modes-pairs", "0:1"],                      # without --modes
           ["--modes", "--modes-hist", "0"], ["--modes", "--modes-hist", "4097"], ["--modes", "--modes-hist", "5x"],
           ["--modes", "--modes-hist", "--modes-hist"],
           ["--modes", "--modes-hpd"], ["--modes", "--modes-hpd", "0"], ["--modes", "--modes-hpd", "1.5"], ["--modes", "--modes-hpd", "0.5,"],
           ["--modes", "--modes-hpd", "nan"], ["--modes", "--modes-hpd", "0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9"],
           ["--modes", "--modes-hpd", "0.5", "--modes-hpd", "0.6"],
           ["--modes", "--modes-pairs"], ["--modes", "--modes-pairs", "0"], ["--modes", "--modes-pairs", "0:"], ["--modes", "--modes-pairs", "0:1,"],
           ["--modes", "--modes-pairs", "-1:2"], ["--modes", "--modes-pairs", "0:1", "0"], ["--modes", "--modes-pairs", "0:1", "129"],
           ["--modes", "--modes-pairs", "0:1", "--modes-pairs", "1:2"])
    for flags in bad:
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + flags, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr, flags
    r = subprocess.run([exe, "a", "b", "c", "d", "e", "--modes-hpd", "0.68"], capture_output=True, text=True, timeout=60)
    assert "--modes-hist, --modes-hpd and --modes-pairs need --modes" in r.stderr
    good = (["--modes", "--modes-hist"], ["--modes-hist", "4096", "--modes"], ["--modes", "--modes-hpd", "0.68,0.95,1"],
            ["--modes", "--modes-pairs", "0:1,5:5,7:2"], ["--modes-pairs", "0:1", "128", "--modes", "0.5", "--modes-hist", "1", "--modes-hpd", "1e-3"],
            ["--modes", "--modes-ess", "--modes-rank", "--modes-hist", "--modes-hpd", "0.68", "--modes-pairs", "3:4", "--modes-indices"])
    for flags in good:
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + flags, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" not in r.stderr and "cannot read the default configuration" in r.stderr, flags


def test_reference_on_hand_made_cases():
    """The restatement by itself, on cases whose answer can be written down."""
    v = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 0.1, -0.0, 2.0, -1.0, np.inf, -np.inf])
    assert list(PR.classes(v, 0.0, 1.0, 4)) == [0, 1, 2, 3, 3, 0, 0, -2, -1, -2, -1]
    assert list(PR.classes(v, 0.5, 0.5, 7)) == [-1, -1, 0, -2, -2, -1, -1, -2, -1, -2, -1]
    h = PR.hist(v[:7, None], 4)
    assert list(h["counts"][0]) == [3, 1, 1, 2] and h["below"][0] == 0 and h["above"][0] == 0 and list(h["range"][0]) == [0.0, 1.0] and h["status"][0] == 0
    h = PR.hist(v[:, None], 4)
    assert h["status"][0] == 1 and h["counts"].sum() == 0 and h["below"][0] == 0 and h["above"][0] == 0
    big = np.array([-1.7e308, 1.7e308])
    assert PR.hist(big[:, None], 3)["status"][0] == 1 and not PR.range_ok(1.0, 0.0) and PR.range_ok(2.0, 2.0)
    assert list(PR.edges(0.0, 1.0, 4)) == [0.0, 0.25, 0.5, 0.75, 1.0] and PR.edges(0.1, 0.7, 7)[-1] == 0.7
    assert [PR.window(m, 10) for m in (0.1, 0.5, 0.68, 0.95, 1.0, 1e-9)] == [1, 5, 7, 10, 10, 1]
    s = np.array([5.0, 1.0, 1.5, 9.0, 1.75, 4.0, -0.0, 0.0])           # sorted: 0 0 1 1.5 1.75 4 5 9
    r = PR.hpd(s[:, None], [0.5, 1.0, 0.125])
    assert list(r["k"]) == [4, 8, 1] and list(r["start"][:, 0]) == [0, 0, 0] and list(r["lo"][:, 0]) == [0.0, 0.0, 0.0] and list(r["hi"][:, 0]) == [1.5, 9.0, 0.0]
    assert not np.signbit(r["lo"][1, 0])
    assert PR.hpd(np.array([0.0, 5.0, 6.0, 6.5, 9.0, 20.0])[:, None], [0.5])["start"][0, 0] == 1         # 6, 1.5, 3, 13.5
    t = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0])                        # every width tied: the first index
    assert PR.hpd(t[:, None], [0.5])["start"][0, 0] == 0
    w = np.array([-np.inf, -np.inf, 1.0, 2.0, np.inf, np.inf])           # k = 2: NaN, inf, 1, inf, NaN
    assert PR.hpd(w[:, None], [0.3])["start"][0, 0] == 2
    assert PR.hpd(np.full((4, 1), np.inf), [0.5])["start"][0, 0] == 0
    assert [PR.level([3, 3, 3, 1], m) for m in (0.3, 0.9, 0.95, 1.0)] == [3, 3, 1, 1] and PR.level([0, 0], 0.5) == 0
    V = np.stack([v[:7], v[:7][::-1]], axis=1)
    j = PR.hist2d(V, [[0, 0], [0, 1]], 4, mass=(0.5, 1.0))
    assert np.array_equal(j["counts"][0], np.diag([3, 1, 1, 2])) and j["counts"][1].sum() == 7 and list(j["level"][:, 0]) == [2, 1]


def test_core_arithmetic(tmp_path):
    """The header compiles as plain C++17 under g++ and the check passes (what it covers: its own header comment).  Then once
    more built with -fsanitize=address,undefined and run as a stand-alone binary."""
    for name, flags in (("modepdf_core_check", ""), ("modepdf_core_check_san", "-fsanitize=address,undefined -fno-sanitize-recover=undefined")):
        exe = str(tmp_path / name)
        r = subprocess.run(["make", "-s", "-C", CSRC, "modepdf-core-check", "MODEPDF_CHECK=" + exe, "CHECKFLAGS=" + flags],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        print(r.stdout)
        assert r.returncode == 0 and r.stdout.startswith("ok modepdf_core_check") and r.stdout.count("\n") == 1, (r.stdout[-3000:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
