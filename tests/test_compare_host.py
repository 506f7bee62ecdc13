"""The comparison of fits (tamcmc_compare_*; include/tamcmc_accel_compare.h, which tamcmc_accel.h includes), the part that
needs no GPU: the symbols exist with the declared prototypes and constants, a NULL handle and every bad argument of _create
are refused before any device is touched, the shared arithmetic of tamcmc_compare.h passes its stand-alone check
(tests/cpp/compare_core_check.cpp, plain g++), the command-line tool refuses bad usage and files that do not belong together
before it asks for a device, and the reference the GPU test leans on (tests/compare_reference.py) reproduces the Philox known
answers through tests/scan_null_reference.py, its own rules on cases worked by hand, and the bootstrap's exact moments on the
fixed case: E z = elpd_diff and Var z = N' S / (N' + 1); the long-double z of N = 1000, R = 4000, seed 12345 sits at -1.25
and -2.36 of their standard errors, inside the 6 the GPU test asserts of the library's z."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import compare_reference as CR
import scan_null_reference as SN
from support import CSRC, ROOT, tool

H = "tamcmc_compare*"
CH = "const tamcmc_compare*"
PROTOTYPES = {
    "tamcmc_compare_create": ["tamcmc_compare**", "int", "int32_t", "int64_t", "const double*", "const double*", "double", "uint64_t", "int64_t"],
    "tamcmc_compare_info": [CH, "int64_t*", "int64_t*"],
    "tamcmc_compare_diff": [CH, "int32_t", "int32_t", "tamcmc_compare_totals*"],
    "tamcmc_compare_bootstrap": [H, "int64_t", "int64_t"],
    "tamcmc_compare_replicates": [CH, "int64_t*"],
    "tamcmc_compare_z": [CH, "int32_t", "double*"],
    "tamcmc_compare_prob": [CH, "int32_t", "int32_t", "int64_t*", "int64_t*"],
    "tamcmc_compare_interval": [CH, "int32_t", "int32_t", "double", "double*"],
    "tamcmc_compare_weights": [CH, "int32_t", "double*"],
    "tamcmc_compare_stacking": [H, "double", "int64_t", "int64_t", "double*", "tamcmc_compare_stacking_info*"],
    "tamcmc_compare_stacking_cadence": [H, "int32_t"],
    "tamcmc_compare_variates": [H, "int64_t", "double*"],
    "tamcmc_compare_profile": [H, "int"],
    "tamcmc_compare_kernel_time": [H, "int32_t", "double*", "int64_t*"],
    "tamcmc_compare_destroy": [H],
}


def prototypes():
    txt = open(os.path.join(ROOT, "include", "tamcmc_accel_compare.h")).read()
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
    assert protos == PROTOTYPES
    assert sorted(PROTOTYPES) == sorted(accel_mod.capi.COMPARE_EXPORTS)
    for n in PROTOTYPES:
        assert hasattr(lib, n) and n not in accel_mod.capi.EXPORTS and not n.startswith("tamcmc_scan_null_"), n
    consts = dict(re.findall(r"#define TAMCMC_COMPARE_([A-Z0-9_]+)\s+(\d+)", txt))
    assert {k: int(v) for k, v in consts.items()} == dict(MAX_FITS=8, MAX_REPLICATES=1 << 24, TILE=2048, STACK_TILE=4096, PSEUDO_BMA=0,
                                                          PSEUDO_BMA_PLUS=1, STACKING=2)
    cmp = accel_mod.Compare
    assert (cmp.MAX_FITS, cmp.MAX_REPLICATES, cmp.TILE, cmp.STACK_TILE) == (8, 1 << 24, 2048, 4096) and cmp is accel_mod.capi.Compare
    assert accel_mod.capi.COMPARE_METHODS == dict(pseudo_bma=0, pseudo_bma_plus=1, stacking=2)
    for meth in ("from_loo", "diff", "bootstrap", "z", "prob", "interval", "weights", "stacking", "variates", "kernel_time", "profile", "close"):
        assert callable(getattr(cmp, meth)), meth
    assert "typedef struct tamcmc_compare tamcmc_compare;" in txt
    # the structs as ctypes sees them
    assert [f[0] for f in accel_mod.capi.CompareTotals._fields_] == re.search(r"typedef struct tamcmc_compare_totals \{(.*?)\}", txt, flags=re.S).group(1) \
        .replace("int64_t", "").replace("double", "").replace(";", ",").replace(" ", "").replace("\n", "").strip(",").split(",")
    assert C.sizeof(accel_mod.capi.CompareTotals) == 64 and C.sizeof(accel_mod.capi.CompareStackingInfo) == 32
    # tamcmc_accel.h brings the declarations in and declares none of them itself
    acc_h = open(os.path.join(ROOT, "include", "tamcmc_accel.h")).read()
    assert '#include "tamcmc_accel_compare.h"' in acc_h and "int tamcmc_compare_" not in acc_h
    # the kernels' file includes the shared arithmetic under the pragma, which reuses the scan null's generator where it is
    hip = open(os.path.join(CSRC, "tamcmc_compare.hip")).read()
    hdr = open(os.path.join(CSRC, "tamcmc_compare.h")).read()
    assert hip.index("#pragma clang fp contract(off)") < hip.index('#include "tamcmc_compare.h"')
    assert "asm" not in hip.lower() and "fma(" not in hip and "fma(" not in hdr and "atomicAdd" not in hip and "__atomic" not in hip
    assert '#include "tamcmc_scan_null.h"' in hdr and "tmn_philox(" not in hdr and "tmn_uniforms(seed, pair, i, 0u" in hdr
    for k, v in (("MAX_FITS", "8"), ("TILE", "(TM_CMP_THREADS * TM_CMP_UPT)"), ("THREADS", "256"), ("UPT", "8"), ("STACK_UPT", "16")):
        assert re.search(r"#define TM_CMP_%s %s" % (k, re.escape(v)), hdr), k
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "tamcmc_compare.o tamcmc_compare_api.o" in mk and "resource-usage-compare:" in mk and "compare-core-check:" in mk


def test_null_handle_is_refused_without_a_device(accel_mod):
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(8, 7.0)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    n, m = C.c_int64(5), C.c_int64(6)
    t = accel_mod.capi.CompareTotals()
    info = accel_mod.capi.CompareStackingInfo()
    assert lib.tamcmc_compare_info(None, C.byref(n), C.byref(m)) == E and (n.value, m.value) == (5, 6)
    assert lib.tamcmc_compare_diff(None, 0, 1, C.byref(t)) == E
    assert lib.tamcmc_compare_bootstrap(None, 3, 0) == E and lib.tamcmc_compare_bootstrap(None, (1 << 24) + 1, 0) == E
    assert lib.tamcmc_compare_replicates(None, C.byref(n)) == E and n.value == 5
    assert lib.tamcmc_compare_z(None, 1, xp) == E
    assert lib.tamcmc_compare_prob(None, 1, 0, C.byref(n), C.byref(m)) == E
    assert lib.tamcmc_compare_interval(None, 1, 0, 0.5, xp) == E
    for method in (0, 1, 2, 3):
        assert lib.tamcmc_compare_weights(None, method, xp) == E
    assert lib.tamcmc_compare_stacking(None, 1e-8, 100, 0, xp, C.byref(info)) == E
    assert lib.tamcmc_compare_stacking_cadence(None, 4) == E
    assert lib.tamcmc_compare_variates(None, 0, xp) == E
    assert lib.tamcmc_compare_profile(None, 1) == E
    assert lib.tamcmc_compare_kernel_time(None, 0, xp, C.byref(n)) == E and n.value == 5
    assert lib.tamcmc_compare_destroy(None) == 0
    assert np.all(x == 7.0)


def test_bad_arguments_are_refused_before_any_device_use(accel_mod):
    """Every refusal of _create comes before the device count is asked for: the codes are the same with and without a GPU,
    and the handle stays NULL."""
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    elpd = np.linspace(-3.0, -1.0, 8 * 16)
    ep = elpd.ctypes.data_as(C.POINTER(C.c_double))

    def create(K=2, N=16, e=ep, kh=None, scale=1.0, seed=3, first=0, out=True, dev=0):
        h = C.c_void_p()
        rc = lib.tamcmc_compare_create(C.byref(h) if out else None, dev, K, N, e, kh, scale, seed, first)
        assert rc != 0 or h.value
        if rc == 0:
            assert lib.tamcmc_compare_destroy(h) == 0
        else:
            assert not h.value
        return rc

    assert create(out=False) == E
    assert create(K=1) == E and create(K=0) == E and create(K=-2) == E and create(K=9) == E
    assert create(N=0) == E and create(N=-1) == E and create(N=1 << 31) == E
    assert create(e=None) == E
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert create(scale=bad) == E, bad
    assert create(first=-1) == E
    nodev = accel_mod.capi.device_count() <= 0
    ok = accel_mod.capi.E_NODEVICE if nodev else 0
    assert create() == ok and create(K=8) == ok and create(N=1) == ok and create(kh=ep) == ok and create(scale=0.5) == ok
    assert create(first=1 << 62) == ok and create(seed=(1 << 64) - 1) == ok and create(scale=5e-324) == ok
    assert create(dev=-1) == accel_mod.capi.E_NODEVICE and create(dev=1 << 20) == accel_mod.capi.E_NODEVICE
    if nodev:
        try:
            accel_mod.Compare(np.zeros((2, 5)))
        except accel_mod.AccelError as e:
            assert e.code == accel_mod.capi.E_NODEVICE
        else:
            raise AssertionError("no device, and no error")
    for shape in ((5,), (2, 3, 4)):
        try:
            accel_mod.Compare(np.zeros(shape))
        except ValueError:
            pass
        else:
            raise AssertionError("elpd of shape %r was taken" % (shape,))


def write_loo_file(path, x, y, elpd, khat, lead=("x", "y")):
    with open(path, "w") as f:
        f.write("# chainsummary_hip (test)\n# n_used= 10  n_rejected= 0\n# %s %s mean_M elpd_loo pareto_k\n" % lead)
        for i in range(len(x)):
            f.write("%.17g %.17g 1.0 %.17g %.17g\n" % (x[i], y[i], elpd[i], khat[i]))


def test_tool_refuses_bad_usage_and_mismatched_files(tmp_path):
    tool()
    exe = os.path.join(ROOT, "bin", "fitcompare_hip")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Usage: fitcompare_hip" in r.stderr and "--bootstrap R[,seed]" in r.stderr and r.stdout == ""
    x, y = np.arange(6.0), np.ones(6)
    a, b, c, d = (str(tmp_path / n) for n in ("a.txt", "b.txt", "c.txt", "d.txt"))
    write_loo_file(a, x, y, -x, 0.1 * x)
    write_loo_file(b, x, y, -x - 0.5, 0.1 * x)
    write_loo_file(c, x[:5], y[:5], -x[:5], 0.1 * x[:5])                     # a row short
    write_loo_file(d, x + 1e-9, y, -x, 0.1 * x)                              # another grid
    out = str(tmp_path / "out.txt")
    for bad in ([a, out], [a] * 9 + [out], [a, b, out, "--bootstrap"], [a, b, out, "--bootstrap", "0"], [a, b, out, "--bootstrap", "16777217"],
                [a, b, out, "--bootstrap", "10,x"], [a, b, out, "--scale", "0"], [a, b, out, "--scale", "nan"], [a, b, out, "--column"],
                [a, b, out, "--stacking", "-1"], [a, b, out, "--stacking", "1e-8,0"], [a, b, out, "--frobnicate"]):
        r = subprocess.run([exe] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: fitcompare_hip" in r.stderr, bad
    for files, why in (([a, c], "rows"), ([a, d], "leading columns"), ([a, str(tmp_path / "none.txt")], "unable to read")):
        r = subprocess.run([exe] + files + [out], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" not in r.stderr and why in r.stderr and not os.path.exists(out), (files, r.stderr)
    r = subprocess.run([exe, a, b, out, "--column", "elpd_lwo"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "no column elpd_lwo" in r.stderr and not os.path.exists(out)


def test_core_arithmetic(tmp_path):
    """tamcmc_compare.h compiles as plain C++17 under g++ and passes the stand-alone check."""
    exe = str(tmp_path / "compare_core_check")
    r = subprocess.run(["make", "-s", "-C", CSRC, "compare-core-check", "COMPARE_CHECK=" + exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok compare_core_check") and r.stdout.count("\n") == 1, (r.stdout, r.stderr[-3000:])


def test_reference_rules():
    # the generator behind the variates is the scan null's, known answers and all
    assert [int(w) for w in SN.philox(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(w) for w in SN.philox(*([0xFFFFFFFF] * 6))] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert [int(w) for w in SN.philox(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)] == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    bins = np.arange(9, dtype=np.uint64)
    for seed, m in ((12345, 0), (0x9E3779B97F4A7C15, (1 << 32) + 3)):
        ue, uo = SN.uniforms(seed, m, bins, 0)
        e0, s0 = CR.variates(9, seed, 2 * m)
        e1, _ = CR.variates(9, seed, 2 * m + 1)
        assert np.array_equal(e0, -np.log(ue)) and np.array_equal(e1, -np.log(uo)) and np.all(s0 == 1.5 * 2.0 ** -52 * e0)
        assert not np.array_equal(CR.variates(9, seed, 2 * m + 2)[0], e0)
    # the case worked by hand in tests/cpp/compare_core_check.cpp
    nan, inf = float("nan"), float("inf")
    elpd = np.array([[1.0, 2.0, nan, 4.0, 0.5], [0.5, 3.0, 1.0, 4.0, inf]])
    kh = np.array([[0.8, nan, 5.0, 0.1, 0.9], [0.1, inf, 0.2, 0.7, 0.9]])
    t = CR.pair_totals(elpd, kh, 0, 1)
    assert (t["n_included"], t["n_excluded"], t["n_better"], t["n_worse"], t["n_k_high"]) == (3, 2, 1, 1, 2)
    assert t["elpd_diff"] == -0.5 and t["diff_k_high"] == -0.5 and abs(t["se_diff"] - np.sqrt(7.0) / 2) < 1e-15
    assert CR.pair_totals(elpd, None, 1, 0)["n_k_high"] == -1
    assert [CR.rank(q, R) for q, R in ((0.0, 7), (1.0, 7), (0.5, 4), (0.51, 4), (0.05, 4000), (0.95, 4000))] == [0, 6, 1, 2, 199, 3799]
    za, zb = np.array([1.0, -1.0, 0.0, 2.0, 2.0]), np.array([1.0, 3.0, 0.0, -2.0, 2.0])
    assert CR.prob(za, zb) == (1, 3) and [CR.interval(za, zb, q) for q in (0.0, 0.2, 0.21, 0.8, 0.81, 1.0)] == [-4.0, -4.0, 0.0, 0.0, 4.0, 4.0]
    assert np.allclose(np.asarray(CR.softmax([0.0, np.log(3.0)]), dtype=float), [0.25, 0.75], rtol=0, atol=1e-15)
    # z of one replicate: N' B / A by hand, excluded units out
    e = np.array([1.0, 2.0, 5.0, 1.0, 9.0])
    z, sens = CR.z_ld(e, elpd)                                               # D = -0.5, 1, 0 with e = 1, 2, 1
    assert float(z[0]) == 3 * 1.5 / 4 and sens[0] > 0
    # stacking: identical fits have g = 1 at any w; a dominated fit's optimum is the corner
    P = CR.stack_P(np.array([[-1.0, -2.0, -3.0]] * 3), 0.5)
    g, gs, f = CR.stack_g([0.2, 0.3, 0.5], P)
    assert np.all(P == 1) and np.all(np.abs(g - 1) < 1e-18) and abs(f) < 1e-18 and np.all(gs > 0)
    base = np.sin(np.arange(50.0))
    P2 = CR.stack_P(np.stack([base, base - 0.01]), 1.0)
    assert abs(float(CR.stack_optimum_2(P2))) < 1e-18
    rng = np.random.default_rng(5)
    P3 = CR.stack_P(rng.normal(size=(2, 400)), 1.0)
    fstar = CR.stack_optimum_2(P3)
    assert all(fstar >= CR.stack_g([w, 1 - w], P3)[2] for w in np.linspace(0.0, 1.0, 101))


def test_reference_bootstrap_moments():
    """The fixed case in long double from the reference's own variates."""
    elpd, R, seed = CR.moments_case()
    assert elpd.shape == (2, 1000) and (R, seed) == (4000, 12345)
    z = np.array([CR.z_ld(CR.variates(1000, seed, g)[0], elpd)[0][0] for g in range(R)])
    t_mean, t_var = CR.moments_check(z, elpd[1])
    print(f"MOMENTS long double: mean {t_mean:+.3f} se, variance {t_var:+.3f} se")
    assert abs(t_mean) <= 6.0 and abs(t_var) <= 6.0
    assert round(t_mean, 2) == -1.25 and round(t_var, 2) == -2.36
