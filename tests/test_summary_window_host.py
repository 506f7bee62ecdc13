"""Windowed predictive check of a stored chain (tamcmc_summary_window_*, include/tamcmc_accel.h), the part that needs no
GPU: the symbols exist with the declared prototypes and struct layout, a NULL handle is refused before any device is
touched, the command-line tool knows the option, the reference the GPU test leans on (tests/window_reference.py) has the
partition of the header and tails that agree with mpmath at shapes up to 512, and the per-(sample, window) arithmetic
(tamcmc_window.h, shared by the kernels) agrees on the CPU with a long-double brute force
(tests/cpp/window_core_check.cpp, plain g++)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from summary_support import prototypes
from support import tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tamcmc_summary_window_enable", "tamcmc_summary_window_result", "tamcmc_summary_window_kernel_time"]
LD = np.longdouble


def test_symbols_and_signatures(accel_mod):
    lib = accel_mod.load_library()
    protos, txt = prototypes()
    for n in NAMES:
        assert hasattr(lib, n) and n in accel_mod.capi.EXPORTS, n
    assert protos["tamcmc_summary_window_enable"] == ["tamcmc_summary*", "int32_t", "int32_t", "int32_t*"]
    assert protos["tamcmc_summary_window_result"] == ["tamcmc_summary*", "tamcmc_summary_window_totals*"] + ["double*"] * 4
    assert protos["tamcmc_summary_window_kernel_time"] == ["tamcmc_summary*", "double*", "int64_t*"]
    assert "#define TAMCMC_SUMMARY_WINDOW_MAX_BINS 512" in txt and accel_mod.capi.Summary.WINDOW_MAX_BINS == 512
    assert "#define TAMCMC_SUMMARY_WINDOW_MAX_SHAPE 512" in txt and accel_mod.capi.Summary.WINDOW_MAX_SHAPE == 512
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_summary_window_totals;", txt)
    assert m and " ".join(m.group(1).split()) == \
        ("int64_t n_used, n_rejected, n_windows, W, first; double ks_D, min_log_sf, min_log_cdf; "
         "int64_t win_min_log_sf, win_min_log_cdf; int64_t pit_hist[TAMCMC_SUMMARY_PIT_CELLS];")
    t = accel_mod.capi.SummaryWindowTotals
    fields = ["n_used", "n_rejected", "n_windows", "W", "first", "ks_D", "min_log_sf", "min_log_cdf", "win_min_log_sf",
              "win_min_log_cdf", "pit_hist"]
    assert [f[0] for f in t._fields_] == fields
    kinds = dict(t._fields_)
    for k, name in enumerate(fields[:-1]):                   # every field is eight bytes wide, in the header's order
        assert getattr(t, name).offset == 8 * k, name
        assert kinds[name] is (C.c_double if name in ("ks_D", "min_log_sf", "min_log_cdf") else C.c_int64), name
    assert t.pit_hist.offset == 80 and C.sizeof(t) == 80 + 20 * 8
    assert accel_mod.Summary.WINDOW_ARRAYS == ("pit", "log_cdf", "log_sf", "mean_resid")
    assert accel_mod.Summary.WINDOW_TOTALS == tuple(fields[:-1])
    for meth in ("window_enable", "window_result", "window_kernel_time"):
        assert callable(getattr(accel_mod.Summary, meth))
    # what the per-bin check exposes stays as it is
    assert C.sizeof(accel_mod.capi.SummaryPredictiveTotals) == 7 * 8 + 20 * 8
    assert accel_mod.Summary.PREDICTIVE_ARRAYS == ("pit", "log_cdf", "log_sf", "mean_resid")


def test_null_handle_is_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(8, 7.0)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    t = accel_mod.capi.SummaryWindowTotals()
    t.n_used = 77
    nw = C.c_int32(-5)
    assert lib.tamcmc_summary_window_enable(None, 20, 0, C.byref(nw)) == E and nw.value == -5
    assert lib.tamcmc_summary_window_enable(None, 20, 0, None) == E
    assert lib.tamcmc_summary_window_result(None, C.byref(t), xp, xp, xp, xp) == E
    assert np.all(x == 7.0) and t.n_used == 77
    assert lib.tamcmc_summary_window_result(None, None, None, None, None, None) == E
    n = C.c_int64(5)
    assert lib.tamcmc_summary_window_kernel_time(None, xp, C.byref(n)) == E and n.value == 5 and x[0] == 7.0


def test_tool_knows_the_option():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--window W[,first]" in r.stderr and ".windows" in r.stderr and r.stdout == ""
    for bad in (["--window"], ["--window", "0"], ["--window", "513"], ["--window", "7,8"], ["--window", "7,"], ["--window", "7,3,1"],
                ["--window", "x"], ["--window", "7", "--window", "8"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr, bad
    r = subprocess.run([exe, "a", "b", "c", "d", "e", "--window", "7,3", "--predictive"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Usage" not in r.stderr and "cannot read the default configuration" in r.stderr      # the option is taken


def test_core_arithmetic_against_long_double(tmp_path):
    """The header compiles as plain C++17 under g++: shapes 1, 2, 3, 25, 64, 256, 511 and 512 over z from 1e-300 to 1e300 and
    300 draws from Gamma(a) each, the Gaussian form at 1, 2, 7 and 512 bins, the ascending sum and the partition."""
    exe = str(tmp_path / "window_core_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "tamcmc-c-_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "window_core_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok window_core_check") and r.stdout.count("\n") == 1, (r.stdout, r.stderr[-3000:])


def test_reference_partition_and_sums():
    """The reference's windows against a bin-by-bin assignment, and its sums against Python's own additions."""
    import window_reference as R
    for Nx in (1, 2, 7, 65, 700):
        for W in (1, 2, 3, 7, 64, 512):
            for first in sorted({0, 1, min(3, W), W - 1, W} - {-1}):
                if first > W:
                    continue
                f, begin, end = R.partition(Nx, W, first)
                assert f == (first or W) and begin[0] == 0 and end[-1] == Nx and np.all(end > begin) and np.array_equal(begin[1:], end[:-1])
                owner = np.array([0 if i < f else 1 + (i - f) // W for i in range(Nx)])
                assert len(begin) == owner.max() + 1 == 1 + -(-max(Nx - f, 0) // W)
                for w, (b, e) in enumerate(zip(begin, end)):
                    assert np.all(owner[b:e] == w) and e - b <= W
    rng = np.random.default_rng(3)
    rows, y = rng.uniform(0.5, 2.0, size=(3, 23)), rng.exponential(size=23)
    S, length = R.window_sums(rows, y, 5, 3, dtype=np.float64)
    assert list(length) == [3, 5, 5, 5, 5]
    for s in range(3):
        for w, (b, e) in enumerate(((0, 3), (3, 8), (8, 13), (13, 18), (18, 23))):
            acc = y[b] / rows[s, b]
            for i in range(b + 1, e):
                acc = acc + y[i] / rows[s, i]
            assert S[s, w] == acc
    ref = R.window_reference(rows, y, 5, 3)
    one = R.window_reference(rows, y, 1)                      # one bin per window: the per-bin reference
    from predictive_reference import predictive_reference
    per_bin = predictive_reference(rows, y)
    assert all(np.array_equal(one[k], per_bin[k]) for k in ("log_cdf", "log_sf", "mean_resid", "pit"))
    assert np.all(np.abs(np.exp(ref["log_cdf"]) + np.exp(ref["log_sf"]) - 1) < 1e-17)


def test_reference_series_reaches_shape_512():
    """log_gamma_tails sums 260 terms of the series of P wherever Q >= 1/2, that is up to the median of Gamma(a) < a: at
    a = 512 and z = a the first term it leaves out, relative to the sum, is far below a long-double ulp."""
    a = 512
    t, s = LD(1), LD(1)
    for j in range(1, 260):
        t = t * LD(a) / LD(a + j)
        s = s + t
    left_out = t * LD(a) / LD(a + 260)
    print("first neglected term / sum at a = z = 512:", float(left_out / s))
    # (the terms after it fall by a / (a + j) < 2/3 each: their sum is below three times the first)
    assert 3 * float(left_out / s) < float(np.finfo(LD).eps) / 8


def test_reference_tails_against_mpmath():
    """The reference's log P(a, z) and log Q(a, z) at the shapes the windowed check reaches, against mpmath at 60 digits:
    within 8 long-double ulp of the largest term of its log-domain sums, 8 a (at a = 512 and z near a the terms reach 3200)."""
    mp = pytest.importorskip("mpmath")
    import predictive_reference as R
    mp.mp.dps = 60
    eps = float(np.finfo(LD).eps)
    worst = {}
    for a in (1, 2, 3, 25, 64, 256, 511, 512):
        z = np.array([1e-3, a / 2, a - 1, a - 0.3, a, a + 1, 2 * a, 4 * a, 1e4], dtype=np.float64)
        z = z[z > 0]
        lP, lQ = R.log_gamma_tails(a, z.astype(LD))
        w = 0.0
        for zz, gp, gq in zip(z, lP, lQ):
            wantP = mp.log(mp.gammainc(a, 0, mp.mpf(float(zz)), regularized=True))
            wantQ = mp.log(mp.gammainc(a, mp.mpf(float(zz)), mp.inf, regularized=True))
            for got, want in ((gp, wantP), (gq, wantQ)):
                g = mp.mpf(str(np.format_float_scientific(got, precision=25, unique=False)))
                w = max(w, float(abs(g - want) / max(1, abs(want))))
        worst[a] = w
        assert w <= 8 * eps * 8 * a, (a, w)
    print("worst relative error of the reference's gamma tails per shape:", worst)
