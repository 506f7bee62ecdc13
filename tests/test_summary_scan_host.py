"""Sliding-window predictive scan of a stored chain (tamcmc_summary_scan_*, include/tamcmc_accel.h), the part that needs no
GPU: the symbols exist with the declared prototypes and struct layouts, a NULL handle is refused before any device is
touched, the command-line tool knows the options, the host arithmetic of tamcmc_scan.h (position counts, chunk size, default
line, region finder, prefix sums) passes its stand-alone check (tests/cpp/scan_core_check.cpp, plain g++), and the reference
the GPU test leans on (tests/scan_reference.py) equals tests/window_reference.py at aligned positions and finds the regions of
hand-written cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from summary_support import prototypes
from support import tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tamcmc_summary_scan_enable", "tamcmc_summary_scan_result", "tamcmc_summary_scan_regions", "tamcmc_summary_scan_kernel_time"]


def test_symbols_and_signatures(accel_mod):
    lib = accel_mod.load_library()
    protos, txt = prototypes()
    for n in NAMES:
        assert hasattr(lib, n) and n in accel_mod.capi.EXPORTS, n
    assert protos["tamcmc_summary_scan_enable"] == ["tamcmc_summary*", "int32_t", "const int32_t*"]
    assert protos["tamcmc_summary_scan_result"] == ["tamcmc_summary*", "int32_t", "tamcmc_summary_scan_totals*"] + ["double*"] * 4
    assert protos["tamcmc_summary_scan_regions"] == ["tamcmc_summary*", "int32_t", "int32_t", "double", "int32_t",
                                                     "tamcmc_summary_scan_region*", "int32_t*"]
    assert protos["tamcmc_summary_scan_kernel_time"] == ["tamcmc_summary*", "double*", "int64_t*"]
    assert "#define TAMCMC_SUMMARY_SCAN_MAX_WIDTHS 8" in txt and accel_mod.capi.Summary.SCAN_MAX_WIDTHS == 8
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_summary_scan_totals;", txt)
    assert m and " ".join(m.group(1).split()) == \
        "int64_t n_used, n_rejected, W, n_positions; double min_log_sf, min_log_cdf; int64_t pos_min_log_sf, pos_min_log_cdf;"
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_summary_scan_region;", txt)
    assert m and " ".join(m.group(1).split()) == \
        "int64_t pos_first, pos_last, bin_first, bin_last, pos_min; double min_log, mean_resid_at_min;"
    for t, fields, doubles in ((accel_mod.capi.SummaryScanTotals, accel_mod.Summary.SCAN_TOTALS, ("min_log_sf", "min_log_cdf")),
                               (accel_mod.capi.SummaryScanRegion, accel_mod.Summary.SCAN_REGION, ("min_log", "mean_resid_at_min"))):
        assert tuple(f[0] for f in t._fields_) == fields
        kinds = dict(t._fields_)
        for k, name in enumerate(fields):                        # every field is eight bytes wide, in the header's order
            assert getattr(t, name).offset == 8 * k, name
            assert kinds[name] is (C.c_double if name in doubles else C.c_int64), name
        assert C.sizeof(t) == 8 * len(fields)
    assert accel_mod.Summary.SCAN_TOTALS == ("n_used", "n_rejected", "W", "n_positions", "min_log_sf", "min_log_cdf", "pos_min_log_sf",
                                             "pos_min_log_cdf")
    assert accel_mod.Summary.SCAN_ARRAYS == ("pit", "log_cdf", "log_sf", "mean_resid")
    for meth in ("scan_enable", "scan_result", "scan_regions", "scan_kernel_time"):
        assert callable(getattr(accel_mod.Summary, meth))
    # what the disjoint check exposes stays as it is
    assert C.sizeof(accel_mod.capi.SummaryWindowTotals) == 80 + 20 * 8
    assert accel_mod.Summary.WINDOW_ARRAYS == ("pit", "log_cdf", "log_sf", "mean_resid")


def test_null_handle_is_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(8, 7.0)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    W = (C.c_int32 * 2)(7, 20)
    assert lib.tamcmc_summary_scan_enable(None, 2, W) == E
    assert lib.tamcmc_summary_scan_enable(None, 2, None) == E
    t = accel_mod.capi.SummaryScanTotals()
    t.n_used = 77
    assert lib.tamcmc_summary_scan_result(None, 0, C.byref(t), xp, xp, xp, xp) == E
    assert np.all(x == 7.0) and t.n_used == 77
    assert lib.tamcmc_summary_scan_result(None, 0, None, None, None, None, None) == E
    r = (accel_mod.capi.SummaryScanRegion * 2)()
    r[0].pos_first = 55
    n = C.c_int32(-5)
    assert lib.tamcmc_summary_scan_regions(None, 0, 0, -3.0, 2, r, C.byref(n)) == E and n.value == -5 and r[0].pos_first == 55
    assert lib.tamcmc_summary_scan_regions(None, 0, 0, float("nan"), 0, None, None) == E
    k = C.c_int64(5)
    assert lib.tamcmc_summary_scan_kernel_time(None, xp, C.byref(k)) == E and k.value == 5 and x[0] == 7.0


def test_tool_knows_the_options():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--scan W0[,W1,...]" in r.stderr and "--scan-below T" in r.stderr and ".scan.regions" in r.stderr and r.stdout == ""
    for bad in (["--scan"], ["--scan", "0"], ["--scan", "513"], ["--scan", "7,7"], ["--scan", "8,7"], ["--scan", "7,"], ["--scan", "x"],
                ["--scan", "1,2,3,4,5,6,7,8,9"], ["--scan", "7", "--scan", "8"], ["--scan", "7", "--scan-below", "0"],
                ["--scan", "7", "--scan-below"], ["--scan", "7", "--scan-below", "x"], ["--scan", "7", "--scan-below", "-3", "--scan-below", "-4"],
                ["--scan-below", "-3"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr, bad
    for good in (["--scan", "7"], ["--scan", "1,2,3,4,5,6,7,512", "--scan-below", "-8.5", "--window", "7,3", "--predictive"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + good, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" not in r.stderr and "cannot read the default configuration" in r.stderr, good    # the option is taken


def test_core_arithmetic(tmp_path):
    """tamcmc_scan.h compiles as plain C++17 under g++ and its host arithmetic passes the stand-alone check."""
    exe = str(tmp_path / "scan_core_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "tamcmc-c-_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "scan_core_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok scan_core_check") and r.stdout.count("\n") == 1, (r.stdout, r.stderr[-3000:])


def test_reference_is_the_window_reference_at_aligned_positions():
    """Position j of width W is window w of window_reference(W, first) wherever that window is full and starts at bin j: the
    same numbers in long double and in float64, for both likelihoods, and every position is reached by some `first`."""
    import scan_reference as R
    import window_reference as WR
    rng = np.random.default_rng(5)
    Nx = 23
    rows, y = rng.uniform(0.5, 2.0, size=(4, Nx)), rng.exponential(size=Nx)
    sigma = rng.uniform(0.5, 2.0, size=Nx)
    for like, p in ((0, 1), (0, 3), (1, 1)):
        for dtype in (np.longdouble, np.float64):
            for W in (1, 2, 5, 23):
                sc = R.scan_reference(rows, y, W, like, p, sigma, dtype)
                assert all(len(sc[k]) == Nx - W + 1 for k in sc)
                seen = set()
                for first in range(1, W + 1):
                    _, begin, end = WR.partition(Nx, W, first)
                    win = WR.window_reference(rows, y, W, first, like, p, sigma, dtype)
                    for w, (b, e) in enumerate(zip(begin, end)):
                        if e - b == W:
                            seen.add(int(b))
                            for k in ("log_cdf", "log_sf", "mean_resid", "pit"):
                                assert sc[k][b] == win[k][w], (like, p, W, first, w, k)
                assert seen == set(range(Nx - W + 1))
    S = R.scan_sums(rows, y, 5, dtype=np.float64)
    for s in range(4):
        for j in range(Nx - 4):
            acc = y[j] / rows[s, j]
            for i in range(j + 1, j + 5):
                acc = acc + y[i] / rows[s, i]
            assert S[s, j] == acc


def test_reference_regions_by_hand():
    import scan_reference as R
    nan = float("nan")
    assert R.regions([], 5, 100, -3.0) == []
    assert R.regions([-1.0, -3.0, nan, 0.0], 5, 100, -3.0) == []                     # -3 is not below -3, a NaN never is
    v = [-1.0, -5.0, -4.0, -5.0, -5.0, -1.0, -9.0]
    mr = [10.0, 11.0, 12.0, 13.0, 14.0, 15.0, 16.0]
    assert R.regions(v, 4, 100, -3.0, mr) == [
        dict(pos_first=1, pos_last=4, bin_first=1, bin_last=7, pos_min=1, min_log=-5.0, mean_resid_at_min=11.0),
        dict(pos_first=6, pos_last=6, bin_first=6, bin_last=9, pos_min=6, min_log=-9.0, mean_resid_at_min=16.0)]
    got = R.regions([-4.0, -6.0, nan, -7.0, -2.0, -3.5], 1, 100, -3.0)               # a run at each end, one split by a NaN
    assert [(r["pos_first"], r["pos_last"], r["pos_min"], r["bin_last"]) for r in got] == [(0, 1, 1, 1), (3, 3, 3, 3), (5, 5, 5, 5)]
    assert [(r["pos_first"], r["pos_last"]) for r in R.regions([-4.0, -6.0, -7.0], 2, 100, -3.0)] == [(0, 2)]     # all below
    # the default line: log(0.01 W / Nx)
    assert R.default_line(20, 700) == float(np.log(0.01 * 20.0 / 700.0)) and abs(R.default_line(20, 700) + 8.1605) < 1e-4
    assert [(r["pos_first"], r["pos_last"]) for r in R.regions([-8.0, -8.2, -8.1, -9.0], 20, 700)] == [(1, 1), (3, 3)]
    t = R.scan_totals([nan, -2.0, -3.0, -3.0], [nan, nan, nan, nan])
    assert t["pos_min_log_cdf"] == 2 and t["min_log_cdf"] == -3.0 and t["pos_min_log_sf"] == -1 and np.isnan(t["min_log_sf"])
