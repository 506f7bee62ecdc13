"""Leave-one-window-out PSIS-LOO of a stored chain (tamcmc_summary_wloo_*, include/tamcmc_accel.h), the part that needs no
GPU: the symbols exist with the declared prototypes and struct layout, a NULL handle is refused before any device is touched,
the command-line tool knows the option, and the shared arithmetic (tamcmc_wloo.h: the window sum's order, the window
geometry, the byte counts the header documents) holds on the CPU (tests/cpp/wloo_core_check.cpp, plain g++, built by
csrc/Makefile's wloo-core-check, and once more as a stand-alone binary under the address and undefined-behaviour sanitizers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from summary_support import prototypes
from support import kernel_usage, needs_hipcc, tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tamcmc-c-_amd", "csrc")
NAMES = ["tamcmc_summary_wloo_begin", "tamcmc_summary_wloo_result", "tamcmc_summary_wloo_pit_begin", "tamcmc_summary_wloo_pit_result",
         "tamcmc_summary_wloo_pit_kernel_time", "tamcmc_summary_wloo_end"]
FIELDS = ["n_used", "n_rejected", "n_windows", "W", "first", "elpd_lwo", "p_lwo", "k_max", "n_k_high", "n_k_inf"]


def test_symbols_and_signatures(accel_mod):
    lib = accel_mod.load_library()
    protos, txt = prototypes()
    for n in NAMES:
        assert hasattr(lib, n) and n in accel_mod.capi.EXPORTS, n
    assert protos["tamcmc_summary_wloo_begin"] == ["tamcmc_summary*", "int32_t", "int32_t", "int32_t*"]
    assert protos["tamcmc_summary_wloo_result"] == ["tamcmc_summary*", "tamcmc_summary_wloo_totals*", "double*", "double*", "double*", "int32_t*",
                                                    "int64_t*", "int64_t*"]
    assert protos["tamcmc_summary_wloo_pit_begin"] == ["tamcmc_summary*"]
    assert protos["tamcmc_summary_wloo_pit_result"] == ["tamcmc_summary*", "tamcmc_summary_loo_pit_totals*"] + ["double*"] * 5
    assert protos["tamcmc_summary_wloo_pit_kernel_time"] == ["tamcmc_summary*", "double*", "int64_t*"]
    assert protos["tamcmc_summary_wloo_end"] == ["tamcmc_summary*"]
    # the argument order follows the per-bin counterparts
    assert protos["tamcmc_summary_wloo_result"][2:6] == protos["tamcmc_summary_loo_result"][2:]
    assert protos["tamcmc_summary_wloo_pit_result"][1:] == protos["tamcmc_summary_loo_pit_result"][1:]
    assert protos["tamcmc_summary_wloo_begin"][1:] == protos["tamcmc_summary_window_enable"][1:]
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_summary_wloo_totals;", txt)
    assert m and " ".join(m.group(1).split()) == \
        "int64_t n_used, n_rejected, n_windows, W, first; double elpd_lwo, p_lwo, k_max; int64_t n_k_high, n_k_inf;"
    t = accel_mod.capi.SummaryWlooTotals
    assert [f[0] for f in t._fields_] == FIELDS
    kinds = dict(t._fields_)
    for k, name in enumerate(FIELDS):                        # every field starts on the next eight bytes, in the header's order
        assert getattr(t, name).offset == 8 * k, name
        assert kinds[name] is (C.c_double if name in ("elpd_lwo", "p_lwo", "k_max") else C.c_int64), name
    assert C.sizeof(t) == 10 * 8
    S = accel_mod.Summary
    assert S.WLOO_ARRAYS == ("elpd_lwo", "pareto_k", "cutoff") and "elpd_lwo_total" in S.WLOO_TOTALS and "p_lwo" in S.WLOO_TOTALS
    for meth in ("wloo_begin", "wloo_result", "wloo_pit_begin", "wloo_pit_result", "wloo_pit_kernel_time", "wloo_end", "window_loo"):
        assert callable(getattr(S, meth)), meth
    # what LOO mode, LOO-PIT and the windowed check exposed before stays as it is
    assert protos["tamcmc_summary_loo_result"] == ["tamcmc_summary*", "tamcmc_summary_loo_totals*", "double*", "double*", "double*", "int32_t*"]
    assert C.sizeof(accel_mod.capi.SummaryLooTotals) == 64 and C.sizeof(accel_mod.capi.SummaryLooPitTotals) == (9 + 20) * 8
    # the kernels' file is its own: the per-bin and the windowed files do not know it; the header states the mode's bytes
    for other in ("tamcmc_loo.hip", "tamcmc_loopit.hip", "tamcmc_window.hip"):
        assert "wloo" not in open(os.path.join(CSRC, other)).read(), other
    hip = open(os.path.join(CSRC, "tamcmc_wloo.hip")).read()
    assert "#pragma clang fp contract(off)" in hip and "atomic" not in hip.replace("No atomics", "") and "__shfl" not in hip
    doc = open(os.path.join(ROOT, "include", "tamcmc_accel.h")).read()
    assert "52 nw + 32" in doc and "116 nw + 36" in doc and "8 (M + 1) nw" in doc and "16 B nw" in doc


def test_null_handle_is_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(8, 7.0)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    i32 = np.full(8, 7, dtype=np.int32)
    i64 = np.full(8, 7, dtype=np.int64)
    ip, lp = i32.ctypes.data_as(C.POINTER(C.c_int32)), i64.ctypes.data_as(C.POINTER(C.c_int64))
    t, tp = accel_mod.capi.SummaryWlooTotals(), accel_mod.capi.SummaryLooPitTotals()
    t.n_used = tp.n_used = 77
    nw = C.c_int32(-5)
    ms, n = C.c_double(-1.0), C.c_int64(-1)
    assert lib.tamcmc_summary_wloo_begin(None, 20, 0, C.byref(nw)) == E
    assert lib.tamcmc_summary_wloo_begin(None, 20, 7, None) == E
    assert lib.tamcmc_summary_wloo_result(None, C.byref(t), xp, xp, xp, ip, lp, lp) == E
    assert lib.tamcmc_summary_wloo_result(None, None, None, None, None, None, None, None) == E
    assert lib.tamcmc_summary_wloo_pit_begin(None) == E
    assert lib.tamcmc_summary_wloo_pit_result(None, C.byref(tp), xp, xp, xp, xp, xp) == E
    assert lib.tamcmc_summary_wloo_pit_result(None, None, None, None, None, None, None) == E
    assert lib.tamcmc_summary_wloo_pit_kernel_time(None, C.byref(ms), C.byref(n)) == E
    assert lib.tamcmc_summary_wloo_end(None) == E
    assert np.all(x == 7.0) and np.all(i32 == 7) and np.all(i64 == 7) and t.n_used == 77 and tp.n_used == 77
    assert nw.value == -5 and ms.value == -1.0 and n.value == -1


def test_tool_knows_the_option():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "[--loo-window W[,first]]" in r.stderr and ".loowin" in r.stderr and r.stdout == ""
    assert "first_bin last_bin x_first x_last elpd_lwo pareto_k tail_len" in r.stderr
    assert "loo_pit loo_log_cdf loo_log_sf is_ess log_wsum" in r.stderr
    for bad in (["--loo-window"], ["--loo-window", "0"], ["--loo-window", "513"], ["--loo-window", "20,21"], ["--loo-window", "7x"],
                ["--loo-window", "20,0"], ["--loo-window", "20,"], ["--loo-window", "20", "--loo-window", "20"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr, bad
    for good in (["--loo-window", "20"], ["--loo-window", "20,7"], ["--loo-window", "20", "--loo-pit"], ["--loo-pit", "--loo-window", "512,512"],
                 ["--loo-window", "1", "--window", "20", "--block", "7"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + good, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" not in r.stderr and "cannot read the default configuration" in r.stderr, good   # the option is taken


def test_core_arithmetic_against_long_double(tmp_path):
    """The header compiles as plain C++17 under g++ and the check passes: the window sum's order against long double, the
    window geometry for every kind of first and last window, the byte counts the header documents.  Then once more built
    with -fsanitize=address,undefined and run as a stand-alone binary."""
    for name, flags in (("wloo_core_check", ""), ("wloo_core_check_san", "-fsanitize=address,undefined -fno-sanitize-recover=undefined")):
        exe = str(tmp_path / name)
        r = subprocess.run(["make", "-s", "-C", CSRC, "wloo-core-check", "WLOO_CHECK=" + exe, "CHECKFLAGS=" + flags],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        print(r.stdout)
        assert r.returncode == 0 and r.stdout.startswith("ok wloo_core_check") and r.stdout.count("\n") == 1, (r.stdout[-3000:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]


def test_gathered_reference_is_the_reference():
    """The form in which the GPU suites evaluate wloo_reference on chosen windows only (wloo_support.check_reference_at): the
    reference given window 0's bins, the chosen whole middle windows and the last window's bins, with the same W and first,
    returns for those windows the bits of the reference given the whole grid -- 700 bins, 37 rows, float64 and long double; a
    full and a partial first window, a full, a partial and a one-bin last window; the perturbed-x argument too."""
    from window_reference import gathered, partition, windows_holding
    from wloo_reference import wloo_reference
    rng = np.random.default_rng(20263)
    Nx, n = 700, 37
    rows = 1.0 + rng.random((n, Nx))
    y = rows[0] * rng.exponential(size=Nx)
    for Wd, first, top in ((20, 0, 700), (20, 7, 700), (3, 1, 700), (7, 3, 697), (64, 64, 641), (512, 1, 700), (2, 1, 700)):
        f, begin, end = partition(top, Wd, first)
        nw = len(begin)
        chosen = np.unique(np.concatenate([rng.integers(0, nw, size=min(8, nw)), [min(1, nw - 1), max(nw - 2, 0)]]))
        sel, cols, f1 = gathered(chosen, top, Wd, first)
        assert f1 == f and sel[0] == 0 and sel[-1] == nw - 1 and set(chosen) <= set(sel)
        _, b1, e1 = partition(len(cols), Wd, f)
        assert len(b1) == len(sel) and np.array_equal(e1 - b1, (end - begin)[sel])            # the gathered grid's partition is those windows
        assert np.array_equal(cols, np.concatenate([np.arange(begin[i], end[i]) for i in sel]))
        sel2, cols2, _ = windows_holding(begin[chosen], top, Wd, first)                        # by a bin each holds: the same windows
        assert np.array_equal(sel2, sel) and np.array_equal(cols2, cols)
        for dtype in (np.longdouble, np.float64):
            whole = wloo_reference(rows[:, :top], y[:top], Wd, first, dtype=dtype)
            part = wloo_reference(rows[:, cols], y[cols], Wd, f, dtype=dtype)
            assert set(whole) == set(part)
            for k in whole:
                assert part[k].dtype == whole[k].dtype and part[k].shape == (len(sel),), (Wd, first, k)
                assert np.array_equal(part[k], whole[k][sel], equal_nan=True), (Wd, first, dtype, k)
            xb = (np.log(rows) + y / rows).astype(dtype) * dtype(1.0 + 2.0 ** -50)
            whole = wloo_reference(rows[:, :top], y[:top], Wd, first, dtype=dtype, xbins=xb[:, :top])
            part = wloo_reference(rows[:, cols], y[cols], Wd, f, dtype=dtype, xbins=xb[:, cols])
            for k in whole:
                assert np.array_equal(part[k], whole[k][sel], equal_nan=True), (Wd, first, dtype, k, "xbins")


@needs_hipcc
def test_kernel_resources():
    """The five kernels of tamcmc_wloo.hip cross-compiled for gfx950 (make resource-usage-wloo): none uses scratch or spills a
    register; the two sums kernels stage one tile through 34 KiB of LDS, the tail, tails and PIT kernels use none."""
    usage = kernel_usage("resource-usage-wloo")             # scratch bytes, spilled SGPRs, spilled VGPRs, LDS bytes
    assert len(usage) == 5, sorted(usage)
    for k, (scratch, sspill, vspill, lds) in usage.items():
        assert scratch == 0 and sspill == 0 and vspill == 0, (k, scratch, sspill, vspill)
        assert lds == ((4096 + 256) * 8 if "sums_kernel" in k else 0), (k, lds)
    assert sum("sums_kernel" in k for k in usage) == 2
