"""The posterior mode table (tamcmc_modetable_*, include/tamcmc_accel.h), the part that needs no GPU: the symbols exist with
the declared prototypes and struct layouts, a NULL handle is refused before any device is touched, the command-line tool
knows the option, the shared arithmetic (tamcmc_modetable.h: the column layout, the selection, the fold's recurrences, the
byte counts) holds on the CPU (tests/cpp/modetable_core_check.cpp, plain g++, built by csrc/Makefile's modetable-core-check,
and once more as a stand-alone binary under the address and undefined-behaviour sanitizers), the Python restatement of the
layout agrees with the header's for every case of the layout matrix, and the reconstruction the GPU suite relies on has
teeth."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import layouts
import modetable_reference as MR
import workloads as W
from support import pyorc, tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tamcmc-c-_amd", "csrc")
NAMES = ["tamcmc_modetable_create", "tamcmc_modetable_columns", "tamcmc_modetable_column", "tamcmc_modetable_derive",
         "tamcmc_modetable_push", "tamcmc_modetable_result", "tamcmc_modetable_quantiles", "tamcmc_modetable_reset",
         "tamcmc_modetable_destroy", "tamcmc_modetable_kernel_time"]


def prototypes():
    txt = open(os.path.join(ROOT, "include", "tamcmc_accel.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(tamcmc_modetable_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
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
    assert protos["tamcmc_modetable_create"] == ["tamcmc_modetable**", "tamcmc_ctx*", "int64_t"]
    assert protos["tamcmc_modetable_columns"] == [mt, "int32_t*", "int32_t*"]
    assert protos["tamcmc_modetable_column"] == [mt, "int32_t", "tamcmc_modetable_col*"]
    assert protos["tamcmc_modetable_derive"] == [mt, "int32_t", "int32_t", "const double*", "double*", "int32_t*"]
    assert protos["tamcmc_modetable_push"] == [mt, "int32_t", "int32_t", "const double*", "const int32_t*", "int32_t*"]
    assert protos["tamcmc_modetable_result"] == [mt, "tamcmc_modetable_totals*"] + ["double*"] * 4
    assert protos["tamcmc_modetable_quantiles"] == [mt, "int32_t", "const double*", "int64_t*", "double*"]
    assert protos["tamcmc_modetable_reset"] == [mt] and protos["tamcmc_modetable_destroy"] == [mt]
    assert protos["tamcmc_modetable_kernel_time"] == [mt, "double*", "int64_t*"]
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_modetable_col;", txt)
    assert m and " ".join(m.group(1).split()) == "int32_t kind, mult, order, l, m, param_index;"
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_modetable_totals;", txt)
    assert m and " ".join(m.group(1).split()) == "int64_t n_used, n_rejected, n_cols, n_mult;"
    col, tot = accel_mod.capi.ModeTableCol, accel_mod.capi.ModeTableTotals
    assert [f[0] for f in col._fields_] == ["kind", "mult", "order", "l", "m", "param_index"] and C.sizeof(col) == 24
    assert all(f[1] is C.c_int32 for f in col._fields_) and [getattr(col, f[0]).offset for f in col._fields_] == [0, 4, 8, 12, 16, 20]
    assert [f[0] for f in tot._fields_] == ["n_used", "n_rejected", "n_cols", "n_mult"] and C.sizeof(tot) == 32
    assert all(f[1] is C.c_int64 for f in tot._fields_)
    # the thirteen kind codes, in the order of the Python names and of the reference module
    codes = dict(re.findall(r"#define TAMCMC_MODETABLE_([A-Z0-9_]+)\s+(\d+)", txt))
    assert [k.lower() for k, v in sorted(codes.items(), key=lambda kv: int(kv[1]))] == list(accel_mod.capi.MODETABLE_KINDS) == list(MR.KINDS)
    assert sorted(int(v) for v in codes.values()) == list(range(13))
    assert accel_mod.ModeTable.COL_DTYPE == MR.COL_DTYPE
    for meth in ("columns", "derive", "push", "result", "quantiles", "reset", "close", "kernel_time", "__enter__", "__exit__"):
        assert callable(getattr(accel_mod.ModeTable, meth)), meth
    # the header states the object's bytes; the kernels' file includes the derivation under the pragma and leaves it alone
    assert "8 max_samples n_cols bytes" in open(os.path.join(ROOT, "include", "tamcmc_accel.h")).read()
    hip = open(os.path.join(CSRC, "tamcmc_modetable.hip")).read()
    assert hip.index("#pragma clang fp contract(off)") < hip.index('#include "tamcmc_derive.h"')
    for fn in ("tm_derive_chain_scalars", "tm_derive_chain_tables", "tm_derive_mult", "tm_chain_inc"):
        assert fn + "(" in hip, fn


def test_null_handle_is_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(8, 7.0)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    i32 = np.full(8, 7, dtype=np.int32)
    i64 = np.full(8, 7, dtype=np.int64)
    ip, lp = i32.ctypes.data_as(C.POINTER(C.c_int32)), i64.ctypes.data_as(C.POINTER(C.c_int64))
    t, c = accel_mod.capi.ModeTableTotals(), accel_mod.capi.ModeTableCol()
    t.n_used, c.kind = 77, 77
    h = C.c_void_p(5)
    ms, n = C.c_double(-1.0), C.c_int64(-1)
    assert lib.tamcmc_modetable_create(None, None, 10) == E
    assert lib.tamcmc_modetable_create(C.byref(h), None, 10) == E and h.value is None       # (the handle is cleared)
    assert lib.tamcmc_modetable_columns(None, ip, ip) == E
    assert lib.tamcmc_modetable_column(None, 0, C.byref(c)) == E
    assert lib.tamcmc_modetable_derive(None, 1, 8, xp, xp, ip) == E
    assert lib.tamcmc_modetable_push(None, 1, 8, xp, ip, ip) == E
    assert lib.tamcmc_modetable_push(None, 1, 8, None, None, None) == E
    assert lib.tamcmc_modetable_result(None, C.byref(t), xp, xp, xp, xp) == E
    assert lib.tamcmc_modetable_quantiles(None, 1, xp, lp, xp) == E
    assert lib.tamcmc_modetable_reset(None) == E
    assert lib.tamcmc_modetable_kernel_time(None, C.byref(ms), C.byref(n)) == E
    assert lib.tamcmc_modetable_destroy(None) == 0
    assert np.all(x == 7.0) and np.all(i32 == 7) and np.all(i64 == 7) and t.n_used == 77 and c.kind == 77
    assert ms.value == -1.0 and n.value == -1


def test_handle_classes_share_their_plumbing(accel_mod):
    """The six classes that own a handle take close and the context manager from one base, and the destroy function each
    of them names is one the loaded library has."""
    lib, capi = accel_mod.load_library(), accel_mod.capi
    classes = (capi.Accel, capi.Group, capi.Summary, capi.ScanNull, capi.Compare, capi.ModeTable)
    bases = {cls.__mro__[1] for cls in classes}
    assert len(bases) == 1 and bases != {object}
    base = bases.pop()
    for cls in classes:
        for meth in ("_check", "close", "__del__", "__enter__", "__exit__", "_kernel_time"):
            assert getattr(cls, meth) is getattr(base, meth) and meth not in vars(cls), (cls.__name__, meth)
        assert isinstance(cls._HANDLE, str) and cls._HANDLE.startswith("_"), cls.__name__
        assert cls._DESTROY.startswith("tamcmc_") and cls._DESTROY.endswith("_destroy") and hasattr(lib, cls._DESTROY), cls.__name__
    assert len({cls._DESTROY for cls in classes}) == 6


def test_tool_knows_the_option():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "[--modes [q1,q2,...]]" in r.stderr and ".modes" in r.stderr and r.stdout == ""
    assert "col kind mult order l m param_index mean sd min max" in r.stderr
    for bad in (["--modes", "1.5"], ["--modes", "0.5,"], ["--modes", "0.5x"], ["--modes", "--modes"],
                ["--modes", "0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr, bad
    for good in (["--modes"], ["--modes", "0.16,0.5,0.84"], ["--modes", ".5"], ["--modes", "--thin", "2"], ["--ess", "--modes", "0,1"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + good, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" not in r.stderr and "cannot read the default configuration" in r.stderr, good


def test_core_arithmetic(tmp_path):
    """The header compiles as plain C++17 under g++ and the check passes: the layout against tables written out by hand
    (ids 2, 8, 11, 13), the selection against a sort (ties, +-inf, +-0, one value), the fold, the byte counts.  Then once more
    built with -fsanitize=address,undefined and run as a stand-alone binary."""
    for name, flags in (("modetable_core_check", ""), ("modetable_core_check_san", "-fsanitize=address,undefined -fno-sanitize-recover=undefined")):
        exe = str(tmp_path / name)
        r = subprocess.run(["make", "-s", "-C", CSRC, "modetable-core-check", "MODETABLE_CHECK=" + exe, "CHECKFLAGS=" + flags],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        print(r.stdout)
        assert r.returncode == 0 and r.stdout.startswith("ok modetable_core_check") and r.stdout.count("\n") == 1, (r.stdout[-3000:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]


def test_layout_restatement_of_every_matrix_case(tmp_path):
    """The header's layout function (printed by the core check's binary, built from tamcmc_modetable.h) equals the Python
    restatement for every layout of the matrix; the restatement against the closed form of the column count and its own
    structure.  (The GPU suite compares ModeTable.columns() with the restatement once more.)"""
    exe = str(tmp_path / "modetable_core_check")
    r = subprocess.run(["make", "-s", "-C", CSRC, "modetable-core-check", "MODETABLE_CHECK=" + exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for mid, lmax in layouts.LAYOUTS:
        w = W.layout(mid, lmax)
        cols = MR.layout(mid, w["plength"])
        pl = [int(v) for v in w["plength"]]
        r = subprocess.run([exe, "layout", str(mid)] + [str(v) for v in pl[:6]], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (mid, lmax, r.stderr)
        got = np.array([tuple(int(t) for t in line.split()) for line in r.stdout.splitlines()], dtype=MR.COL_DTYPE)
        assert np.array_equal(got, cols), (mid, lmax)
        mults = MR.multiplets(mid, w["plength"])
        assert len(cols) == 4 + sum(7 + 2 * (2 * l + 1) for (_, l, _) in mults), (mid, lmax)
        assert list(cols["kind"][:4]) == [0, 1, 2, 3] and np.all(cols["mult"][:4] == -1)
        first = MR.first_columns(cols)
        assert len(first) == len(mults) and list(cols["mult"][first]) == list(range(len(mults)))
        for c0, (n, l, idx) in zip(first, mults):
            assert (cols["order"][c0], cols["l"][c0], cols["param_index"][c0]) == (n, l, idx)
            assert list(cols["kind"][c0:c0 + 7]) == list(range(4, 11))
            assert list(cols["m"][c0 + 7:c0 + 7 + 2 * (2 * l + 1)]) == 2 * list(range(-l, l + 1))
        assert np.all(cols["param_index"][cols["kind"] != MR.K["freq"]] == -1)
        # a frequency column points into the frequency block of its degree
        pl = [int(v) for v in w["plength"]]
        f0 = pl[0] + pl[1]
        assert np.all((cols["param_index"][first] >= f0) & (cols["param_index"][first] < f0 + sum(pl[2:6])))
    w = W.layout(2, 2, Nmax=7)
    assert len(MR.layout(2, w["plength"])) == 277                 # the benchmark layout's count


def true_table_id2(w, p):
    """The table row of an id-2 params row from the oracle's exported pieces (models.cpp:528-560 and the `for n` loop)."""
    orc = pyorc()
    pl, x = [int(v) for v in w["plength"]], w["x"]
    b = W.split(w)
    Nmax, lmax, s, wq, q = b["Nmax"], b["lmax"], b["s"], b["w"], b["q"]
    inc = math.atan(p[s + 4] / p[s + 3]) * 180.0 / math.pi
    a1 = p[s + 3] ** 2 + p[s + 4] ** 2
    eta, a3, asym, trunc_c, do_amp = p[s + 1], p[s + 2], p[s + 5], p[q + 1], p[q + 2] != 0.0
    row = [inc, eta, a3, asym]
    f0 = Nmax + lmax
    for (n, l, idx) in MR.multiplets(2, pl):
        f = p[idx]
        G = abs(p[wq + n]) if l == 0 else abs(orc.lin_interpol(p[f0:f0 + Nmax], p[wq:wq + Nmax], f))
        V = 1.0 if l == 0 else abs(p[Nmax + l - 1])
        H = abs(p[n] / (math.pi * G)) * V if do_amp else abs(p[n] * V)
        h = [H * r for r in orc.amplitude_ratio(l, inc)]
        nu = [f if l == 0 else f * (1.0 + eta * MR.q_lm(l, m)) + m * a1 + MR.c_lm(l, m, 0) * a3 for m in range(-l, l + 1)]
        st, lo, hi = orc.truncation_window(x, f, a1, G, l, trunc_c)
        assert st == 0
        height = sum(h)
        row += [f, G, height, math.sqrt(math.pi * height * G), 0.0 if l == 0 else a1, float(lo), float(hi)] + nu + h
    return np.array(row)


def test_the_reference_has_teeth():
    """On the oracle's own row of one id-2 case the true table passes the bound; one nu_m moved by 1e-9 relative fails it, and
    so does one window edge moved by one bin."""
    w = layouts.matrix_case(2, 2, "asym-amp", "fused")
    p = W.perturbed(w, 1)[0]
    M, st = pyorc().model(2, p, w["plength"], w["x"])
    assert st == 0
    cols = MR.layout(2, w["plength"])
    row = true_table_id2(w, p)
    assert row.shape == (len(cols),)
    R, S = MR.reconstruct(2, w["plength"], w["x"], p, row, cols)
    ratio = MR.worst_ratio(R, S, M)
    print(f"true table: worst |R - M| / bound = {ratio:.3g}")
    assert ratio <= 1.0
    c_nu = int(np.flatnonzero((cols["kind"] == MR.K["nu_m"]) & (cols["l"] == 1) & (cols["m"] == 1))[2])
    moved = row.copy()
    moved[c_nu] *= 1.0 + 1e-9
    R, S = MR.reconstruct(2, w["plength"], w["x"], p, moved, cols)
    assert MR.worst_ratio(R, S, M) > 1.0
    for kind, step in (("window_lo", 1.0), ("window_hi", -1.0)):
        c_w = int(np.flatnonzero((cols["kind"] == MR.K[kind]) & (cols["l"] == 2))[1])
        moved = row.copy()
        moved[c_w] += step
        R, S = MR.reconstruct(2, w["plength"], w["x"], p, moved, cols)
        assert MR.worst_ratio(R, S, M) > 1.0, kind
