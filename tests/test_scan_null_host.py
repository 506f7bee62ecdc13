"""Monte-Carlo null of the scan (tamcmc_scan_null_*, include/tamcmc_accel.h), the part that needs no GPU: the symbols exist
with the declared prototypes, a NULL handle and every bad argument of _create are refused before any device is touched, the
generator, combine rule and calibration of tamcmc_scan_null.h pass their stand-alone check (tests/cpp/scan_null_core_check.cpp,
plain g++), and the reference the GPU test leans on (tests/scan_null_reference.py) reproduces the published Philox known
answers and its own counting rules on a case worked by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from support import ROOT, tool

H = "tamcmc_scan_null*"
PROTOTYPES = {
    "tamcmc_scan_null_create": ["tamcmc_scan_null**", "int", "int", "double", "int64_t", "int32_t", "const int32_t*", "uint64_t", "int64_t"],
    "tamcmc_scan_null_run": [H, "int64_t"],
    "tamcmc_scan_null_replicates": ["const " + H, "int64_t*"],
    "tamcmc_scan_null_result": [H, "int32_t", "int32_t", "double*", "int64_t*", "double*"],
    "tamcmc_scan_null_line": [H, "int32_t", "int32_t", "double", "int32_t", "double*"],
    "tamcmc_scan_null_pvalue": [H, "int32_t", "int32_t", "double", "double*", "double*"],
    "tamcmc_scan_null_variates": [H, "int64_t", "double*"],
    "tamcmc_scan_null_profile": [H, "int"],
    "tamcmc_scan_null_kernel_time": [H, "double*", "int64_t*"],
    "tamcmc_scan_null_destroy": [H],
}


def prototypes():
    txt = open(os.path.join(ROOT, "include", "tamcmc_accel.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(tamcmc_scan_null_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            a = re.sub(r"\s*\b[A-Za-z_]\w*$", "", a)                       # drop the parameter's name
            types.append(a.replace(" *", "*"))
        out[name] = types
    return out, txt


def test_symbols_and_signatures(accel_mod):
    lib = accel_mod.load_library()
    protos, txt = prototypes()
    assert protos == PROTOTYPES
    for n in PROTOTYPES:
        assert hasattr(lib, n) and n in accel_mod.capi.EXPORTS, n
        assert re.fullmatch(r"tamcmc_[a-z_]+", n)
    assert "typedef struct tamcmc_scan_null tamcmc_scan_null;" in txt
    assert "#define TAMCMC_SCAN_NULL_MAX_REPLICATES 16777216" in txt and accel_mod.ScanNull.MAX_REPLICATES == 1 << 24
    for meth in ("run", "result", "line", "pvalue", "variates", "kernel_time", "profile", "close", "__enter__", "__exit__"):
        assert callable(getattr(accel_mod.ScanNull, meth)), meth
    assert accel_mod.ScanNull is accel_mod.capi.ScanNull


def test_null_handle_is_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(8, 7.0)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    pos = np.full(8, 7, dtype=np.int64)
    pp = pos.ctypes.data_as(C.POINTER(C.c_int64))
    n = C.c_int64(5)
    assert lib.tamcmc_scan_null_run(None, 3) == E
    assert lib.tamcmc_scan_null_replicates(None, C.byref(n)) == E and n.value == 5
    assert lib.tamcmc_scan_null_result(None, 0, 0, xp, pp, xp) == E
    assert lib.tamcmc_scan_null_result(None, 0, 0, None, None, None) == E
    assert lib.tamcmc_scan_null_line(None, 0, 0, 0.01, 1, xp) == E
    assert lib.tamcmc_scan_null_pvalue(None, 0, 0, -3.0, xp, xp) == E
    assert lib.tamcmc_scan_null_variates(None, 0, xp) == E
    assert lib.tamcmc_scan_null_profile(None, 1) == E
    assert lib.tamcmc_scan_null_kernel_time(None, xp, C.byref(n)) == E and n.value == 5
    assert lib.tamcmc_scan_null_destroy(None) == 0
    assert np.all(x == 7.0) and np.all(pos == 7)


def test_bad_arguments_are_refused_before_any_device_use(accel_mod):
    """Every refusal of _create comes before the device count is asked for: the codes are the same with and without a GPU,
    and the handle stays NULL.  Widths, p and the shape limits are those of tamcmc_summary_scan_enable."""
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID

    def create(like=0, p=1.0, Nx=1000, W=(10, 20, 40), seed=3, first=0, n=None, out=True, dev=0):
        h = C.c_void_p()
        arr = (C.c_int32 * max(len(W), 1))(*W) if W is not None else None
        rc = lib.tamcmc_scan_null_create(C.byref(h) if out else None, dev, like, p, Nx, len(W) if n is None else n, arr, seed, first)
        assert rc != 0 or h.value
        if rc == 0:
            assert lib.tamcmc_scan_null_destroy(h) == 0
        else:
            assert not h.value
        return rc

    assert create(out=False) == E
    assert create(like=2) == accel_mod.capi.E_UNKNOWN_MODEL and create(like=-1) == accel_mod.capi.E_UNKNOWN_MODEL
    assert create(W=None, n=3) == E
    assert create(W=(), n=0) == E and create(W=(7,), n=-1) == E
    assert create(W=tuple(range(1, 10))) == E                                # nine widths
    assert create(W=(0,)) == E and create(W=(-3,)) == E and create(W=(513,)) == E
    assert create(W=(7, 7)) == E and create(W=(8, 7)) == E
    assert create(W=(7, 1001)) == E and create(Nx=6, W=(7,)) == E            # wider than the grid
    assert create(Nx=0, W=(1,)) == E and create(Nx=-5, W=(1,)) == E and create(Nx=1 << 31, W=(1,)) == E
    assert create(p=0.5) == E and create(p=0.0) == E and create(p=-1.0) == E and create(p=float("nan")) == E
    assert create(p=513.0, W=(1,)) == E and create(p=13.0, W=(10, 20, 40)) == E and create(p=64.0, W=(1, 9)) == E
    assert create(first=-1) == E
    # what is left is a good call: refused only for want of a device, or created
    nodev = accel_mod.capi.device_count() <= 0
    ok = accel_mod.capi.E_NODEVICE if nodev else 0
    assert create() == ok
    assert create(p=64.0, W=(1, 8)) == ok and create(p=12.9, W=(10, 20, 40)) == ok and create(p=512.0, W=(1,)) == ok
    assert create(like=1, p=-7.0, W=(1, 512)) == ok                          # chi_square ignores p
    assert create(Nx=1, W=(1,)) == ok and create(first=(1 << 62)) == ok and create(seed=(1 << 64) - 1) == ok
    assert create(dev=-1) == accel_mod.capi.E_NODEVICE and create(dev=1 << 20) == accel_mod.capi.E_NODEVICE
    if nodev:
        try:
            accel_mod.ScanNull(0, 1, 1000, (10, 20), 3)
        except accel_mod.AccelError as e:
            assert e.code == accel_mod.capi.E_NODEVICE
        else:
            raise AssertionError("no device, and no error")


def test_tool_knows_the_option():
    """chainsummary_hip --scan-null R[,seed]: needs --scan, R with floor(0.01 (R + 1)) >= 1, a usage error otherwise."""
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--scan-null R[,seed]" in r.stderr and "p_width p_joint" in r.stderr and r.stdout == ""
    for bad in (["--scan-null", "500"], ["--scan", "7", "--scan-null"], ["--scan", "7", "--scan-null", "98"], ["--scan", "7", "--scan-null", "0"],
                ["--scan", "7", "--scan-null", "-5"], ["--scan", "7", "--scan-null", "x"], ["--scan", "7", "--scan-null", "500,"],
                ["--scan", "7", "--scan-null", "500,x"], ["--scan", "7", "--scan-null", "500,1,2"], ["--scan", "7", "--scan-null", "16777217"],
                ["--scan", "7", "--scan-null", "500", "--scan-null", "600"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr, bad
    for good in (["--scan", "7", "--scan-null", "99"], ["--scan", "7,20", "--scan-null", "500,18446744073709551615", "--scan-below", "-8"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + good, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" not in r.stderr and "cannot read the default configuration" in r.stderr, good


def test_core_arithmetic(tmp_path):
    """tamcmc_scan_null.h compiles as plain C++17 under g++ and passes the stand-alone check."""
    exe = str(tmp_path / "scan_null_core_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tamcmc-c-_amd", "csrc"), "scan-null-core-check", "SCAN_NULL_CHECK=" + exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok scan_null_core_check") and r.stdout.count("\n") == 1, (r.stdout, r.stderr[-3000:])


def test_reference_generator_and_counting():
    import scan_null_reference as R

    def words(*a):
        return [int(w) for w in R.philox(*a)]

    assert words(0, 0, 0, 0, 0, 0) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert words(*([0xFFFFFFFF] * 6)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert words(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    lo, hi = R.uniform(0, 0)[0], R.uniform(0xFFFFFFFF, 0xFFFFFFFF)[0]
    assert lo == 2.0 ** -53 and hi == 1.0 - 2.0 ** -53 and 0.0 < lo and hi < 1.0
    x = np.array([1e-9, 0.25, 0.5 - 1e-12, 0.5, 1.0, 1.5 + 1e-15, 2.0 - 1e-9], dtype=R.LD)
    assert np.all(np.abs(R.cospi_ld(x) - np.cos(R.PI * x)) < 1e-18) and R.cospi_ld(np.array([0.5, 1.5]))[0] == 0
    q = np.array([1.0, 3.0, 2.0, 3.0, 0.5, 0.5, 2.5])
    assert R.sliding(q, 2).tolist() == [4.0, 5.0, 5.0, 3.5, 1.0, 3.0] and R.extremes(q, 2) == (5.0, 1, 1.0, 4)
    assert R.extremes(q, 1) == (3.0, 1, 0.5, 4) and R.extremes(q, 7) == (12.5, 0, 12.5, 0)
    m = np.array([[-5.0, -1.0], [-1.0, -6.0], [-3.0, -2.0], [-2.0, -2.0]])
    cnt, vmin = R.calibration(m)
    assert cnt.tolist() == [[1, 4], [4, 1], [2, 3], [3, 3]] and vmin.tolist() == [1, 1, 2, 3]
    assert R.line(m, 0, 0.4, False) == -3.0 and R.line(m, 0, 0.6, True) == -3.0 and R.line(m, 1, 0.8, True) == -2.0
    assert R.line(m, 0, 0.19, True) is None and R.line(m, 0, 1.0, False) is None
    assert R.pvalue(m, 0, -3.0) == (3 / 5, 4 / 5) and R.pvalue(m, 1, -7.0) == (1 / 5, 1 / 5)
    # the laws of the variates, on the reference alone: mean 1 and variance 1 / p; mean 0 and variance 1 / 2
    for like, p, mean, var in ((0, 1, 1.0, 1.0), (0, 3, 1.0, 1.0 / 3.0), (1, 1, 0.0, 0.5)):
        v, sens = R.variates(like, p, 20000, 3, 0)
        v = v.astype(np.float64)
        assert abs(v.mean() - mean) < 4.0 * np.sqrt(var / 20000) and abs(v.var() - var) < 0.05 * var, (like, p, v.mean(), v.var())
        assert np.all(sens >= 0) and np.all(sens <= 2.0 ** -50 * np.maximum(np.abs(v), 1e-300) * max(p, 2))
