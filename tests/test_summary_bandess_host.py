"""ESS of the credible-band edges (tamcmc_summary_bandess_*, include/tamcmc_accel.h), the part that needs no GPU: the symbols
exist with the declared prototypes and struct layout, a NULL handle is refused before any device is touched, the
command-line tool knows the option and refuses it without --quantiles, the reference the GPU test leans on
(tests/bandess_reference.py) agrees with a term-by-term sum, and the shared integer arithmetic (tamcmc_bandess.h: packing,
ring, head, lag groups, E_k) agrees on the CPU with brute-force sums (tests/cpp/bandess_core_check.cpp, plain g++, built by
csrc/Makefile's bandess-core-check) -- once plainly and once under AddressSanitizer and UBSan, where a signed overflow in E_k
would be a failure."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from summary_support import prototypes
from support import tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tamcmc_summary_bandess_begin", "tamcmc_summary_bandess_result", "tamcmc_summary_bandess_counts", "tamcmc_summary_bandess_end"]
SCALARS = ["n_used", "n_rejected", "lag", "n_thresholds"]
VECTORS = ["min_ess", "bin_min_ess", "n_truncated", "n_constant"]


def test_symbols_and_signatures(accel_mod):
    lib = accel_mod.load_library()
    protos, txt = prototypes()
    for n in NAMES:
        assert hasattr(lib, n) and n in accel_mod.capi.EXPORTS, n
    assert protos["tamcmc_summary_bandess_begin"] == ["tamcmc_summary*", "int32_t", "const double*", "int32_t", "int32_t*"]
    assert protos["tamcmc_summary_bandess_result"] == ["tamcmc_summary*", "tamcmc_summary_bandess_totals*", "int32_t*"] + ["double*"] * 4 + ["int32_t*"]
    assert protos["tamcmc_summary_bandess_counts"] == ["tamcmc_summary*", "int32_t", "int32_t*", "int64_t*"]
    assert protos["tamcmc_summary_bandess_end"] == ["tamcmc_summary*"]
    m = re.search(r"typedef struct \{([^}]*)\}\s*tamcmc_summary_bandess_totals;", txt)
    Q = "[TAMCMC_SUMMARY_MAX_QUANTILES]"
    assert m and " ".join(m.group(1).split()) == \
        (f"int64_t n_used, n_rejected, lag, n_thresholds; double min_ess{Q}; int64_t bin_min_ess{Q}, n_truncated{Q}, n_constant{Q};")
    assert "#define TAMCMC_SUMMARY_MAX_QUANTILES 8" in txt and accel_mod.capi.MAX_QUANTILES == 8
    t = accel_mod.capi.SummaryBandEssTotals
    assert [f[0] for f in t._fields_] == SCALARS + VECTORS
    kinds = dict(t._fields_)
    for k, name in enumerate(SCALARS):                       # four 8-byte scalars, then four arrays of eight 8-byte values
        assert getattr(t, name).offset == 8 * k and kinds[name] is C.c_int64, name
    for k, name in enumerate(VECTORS):
        assert getattr(t, name).offset == 32 + 64 * k and getattr(t, name).size == 64, name
        assert kinds[name]._type_ is (C.c_double if name == "min_ess" else C.c_int64) and kinds[name]._length_ == 8, name
    assert C.sizeof(t) == 32 + 4 * 64
    assert accel_mod.Summary.BANDESS_ARRAYS == ("count_le", "p_hat", "ess", "tau", "mcse_p", "cut")
    assert accel_mod.Summary.BANDESS_TOTALS == tuple(SCALARS + VECTORS)
    for meth in ("bandess_begin", "bandess_result", "bandess_counts", "bandess_end", "band_ess"):
        assert callable(getattr(accel_mod.Summary, meth))
    # what the other modes expose stays as it is
    assert C.sizeof(accel_mod.capi.SummaryEssTotals) == 12 * 8 and C.sizeof(accel_mod.capi.SummaryLooTotals) == 8 * 8
    # the mode's limits agree with the header's and with ESS mode's
    h = open(os.path.join(ROOT, "tamcmc-c-_amd", "csrc", "tamcmc_bandess.h")).read()
    assert "#define TM_BANDESS_MAX_K 8" in h and "#define TM_BANDESS_MAX_N (1LL << 20)" in h and '#include "tamcmc_ess.h"' in h


def test_null_handle_is_refused_without_a_device(accel_mod):
    """A NULL object is every entry point's first refusal: nothing is written, *lag_used included."""
    lib = accel_mod.load_library()
    E = accel_mod.capi.E_INVALID
    x = np.full(16, 7.0)
    c = np.full(16, 7, dtype=np.int32)
    e = np.full(16, 7, dtype=np.int64)
    xp, cp, ep = x.ctypes.data_as(C.POINTER(C.c_double)), c.ctypes.data_as(C.POINTER(C.c_int32)), e.ctypes.data_as(C.POINTER(C.c_int64))
    t = accel_mod.capi.SummaryBandEssTotals()
    t.n_used = 77
    lag = C.c_int32(-5)
    assert lib.tamcmc_summary_bandess_begin(None, 1, xp, 0, C.byref(lag)) == E and lag.value == -5
    assert lib.tamcmc_summary_bandess_begin(None, 3, None, 255, None) == E
    assert lib.tamcmc_summary_bandess_begin(None, 0, xp, 0, C.byref(lag)) == E and lag.value == -5
    assert lib.tamcmc_summary_bandess_result(None, C.byref(t), cp, xp, xp, xp, xp, cp) == E
    assert lib.tamcmc_summary_bandess_result(None, None, None, None, None, None, None, None) == E
    assert lib.tamcmc_summary_bandess_counts(None, 0, cp, ep) == E and lib.tamcmc_summary_bandess_counts(None, 0, None, None) == E
    assert lib.tamcmc_summary_bandess_end(None) == E
    assert np.all(x == 7.0) and np.all(c == 7) and np.all(e == 7) and t.n_used == 77


def test_tool_knows_the_option():
    exe = tool()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--band-ess [L]" in r.stderr and ".bandess" in r.stderr and "value count_le p_hat ess tau mcse_p cut" in r.stderr
    assert "needs --quantiles" in r.stderr and r.stdout == ""
    # without --quantiles: refused, and the error says why
    for bad in (["--band-ess"], ["--band-ess", "31"], ["--band-ess", "--loo"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr and "--band-ess needs --quantiles" in r.stderr, bad
    for bad in (["--band-ess", "1024"], ["--band-ess", "7x"], ["--band-ess", "--band-ess"], ["--band-ess", "31", "--band-ess"], ["--band-ess", "-3"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e", "--quantiles", "0.5"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage: chainsummary_hip" in r.stderr, bad
    for good in (["--band-ess"], ["--band-ess", "31"], ["--band-ess", "--ess"], ["--ess", "3", "--band-ess", "0", "--block", "7"], ["--band-ess", "1023"]):
        r = subprocess.run([exe, "a", "b", "c", "d", "e", "--quantiles", "0.025,0.5,0.975"] + good, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" not in r.stderr and "cannot read the default configuration" in r.stderr, good     # the option is taken


@pytest.mark.parametrize("flags", ["", "-fsanitize=address,undefined -fno-sanitize-recover=all"])
def test_core_arithmetic_against_brute_force(tmp_path, flags):
    """The header compiles as plain C++17 under g++ and the check passes: every n in 4 ... 200 at L in {1, 3, 63, 65, 127, 129},
    random, constant, alternating and single-1 series fed in pieces of random sizes with rejected samples among them, two
    series of 3000 at L = 255 and 1023, E_k at n = 2^20 - 1 against __int128, the comparison at signed zeros, infinities and
    NaN.  The second run is the same program under AddressSanitizer and UBSan (a stand-alone binary: nothing is preloaded)."""
    exe = str(tmp_path / "bandess_core_check")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tamcmc-c-_amd", "csrc"), "bandess-core-check", "BANDESS_CHECK=" + exe] +
                       (["CHECKFLAGS=" + flags] if flags else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok bandess_core_check") and r.stdout.count("\n") == 1, (r.stdout[-3000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]


def test_reference_on_known_series():
    """tests/bandess_reference.py: counts() against a term-by-term sum of (n b_t - N)(n b_{t-k} - N) on random, constant and
    NaN-threshold series, E_0 = n N (n - N), and the finish of a constant series."""
    import bandess_reference as B
    rng = np.random.default_rng(5)
    n, nx, L = 41, 6, 9
    rows = rng.standard_normal((n, nx))
    thr = np.array([0.0, -0.5, 10.0, -10.0, np.nan, rows[3, 5]])
    N, Cc, E = B.counts(rows, thr, L)
    b = (rows <= thr).astype(int)
    assert list(N[2:5]) == [n, 0, 0] and np.array_equal(N, b.sum(axis=0)) and np.array_equal(Cc[0], N)
    for i in range(nx):
        for k in range(L + 1):
            assert int(Cc[k, i]) == sum(int(b[t, i] * b[t - k, i]) for t in range(k, n))
            assert int(E[k, i]) == sum((n * int(b[t, i]) - int(N[i])) * (n * int(b[t - k, i]) - int(N[i])) for t in range(k, n)), (i, k)
    tau, ess, cut = B.finish(E, n, L)
    assert np.all(np.isnan(ess[2:5])) and np.all(cut[2:5] == 0) and np.all(np.isfinite(ess[[0, 1, 5]])) and np.all(tau[[0, 1, 5]] >= 1.0 / np.log10(n))
    assert B.first_min([np.nan, 3.0, 2.0, 2.0]) == (2.0, 2) and B.first_min([np.nan])[1] == -1
    # Python ints: no width to overflow at the mode's largest n
    big = 2 ** 20 - 1
    assert big * big * big - big * (big - 1) * (2 * (big - 1)) + big * (big - 1) ** 2 < 2 ** 62
