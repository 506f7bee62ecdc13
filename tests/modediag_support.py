"""What the suites of the mode table's diagnostics share (tests/test_modediag_gpu.py, tests/test_mode_columns_gpu.py): the
checks of one ess / acov / cov / corr result against ess_reference and modediag_reference.  Importing this module needs no
GPU."""
import math

import numpy as np

import ess_reference as ER
import modediag_reference as DR
from support import LD, bits

U = 2.0 ** -52
WORST = {"lag": 0.0, "cov": 0.0, "rhat": 0.0, "corr": 0.0}
RHAT = {}                         # case -> (the library's rhat, the accepted derive rows), filled by the cases as they run
TOTALS = ("n_used", "lag", "min_ess", "col_min_ess", "max_rhat", "col_max_rhat", "n_truncated", "n_constant", "n_rhat_high")


def check_against_references(tag, r, rows, res, L, worst=WORST, const=None):
    """Checks 2 to 5 of one case: r = collect(), rows = the accepted derive rows, res = ModeTable.result().  The worst ratios
    go into `worst`.  const: the columns whose centred values square to exact zeros (default: the columns of equal values)."""
    WORST = worst
    n, nc = rows.shape
    assert r["n_used"] == n == res["n_used"] and r["lag"] == L == ER.lag_limit(L, n) and r["acov"].shape == (L + 1, nc), tag
    A, cov = r["acov"], r["cov"]
    if const is None:
        const = rows.min(axis=0) == rows.max(axis=0)
    # (2) identities
    assert np.array_equal(bits(cov), bits(cov.T)), tag
    assert np.array_equal(bits(np.diag(cov)), bits(A[0] / np.float64(n - 1))), tag
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(r["mcse"]), bits(res["sd"] / np.sqrt(r["ess"]))), tag
    assert const.any() and np.all(A[:, const] == 0.0) and not np.any(np.signbit(A[:, const])), tag
    for k in ("ess", "tau", "rhat", "mcse"):
        assert np.all(np.isnan(r[k][const])), (tag, k)
    assert np.all(r["cut"][const] == 0) and r["n_constant"] == const.sum(), tag
    assert not np.any(np.isnan(r["ess"][~const])), tag
    # (3) the finish on the library's own lag products; the totals from the arrays
    tau, ess, cut = ER.finish(A, n)
    floor = 1.0 / math.log10(float(n))
    assert np.array_equal(cut, r["cut"]), tag
    for got, want in ((r["tau"], tau), (r["ess"], ess)):
        on_floor = np.abs(tau - floor) <= 4 * U * floor
        ok = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)) | (on_floor & (np.abs(got - want) <= 4 * U * np.abs(want)))
        assert np.all(ok), (tag, np.flatnonzero(~ok))
    want_t = DR.totals(r["ess"], r["rhat"], r["cut"], A[0], L, n)
    for k in TOTALS:
        assert r[k] == want_t[k] or (isinstance(want_t[k], float) and np.isnan(want_t[k]) and np.isnan(r[k])), (tag, k, r[k], want_t[k])
    # (4) long double, on the library's own rows and mean
    d, e = DR.centred(rows, res["mean"])
    Aq, bound = DR.lag(d, e, L)
    err = np.abs(A.astype(LD) - Aq).astype(np.float64)
    assert np.all(err <= 10 * bound), (tag, float(np.max(err[bound > 0] / bound[bound > 0])))
    if np.any(bound > 0):
        WORST["lag"] = max(WORST["lag"], float(np.max(err[bound > 0] / bound[bound > 0])))
    Sq, sbound = DR.cov_sums(d, e)
    serr = np.abs(cov.astype(LD) * LD(n - 1) - Sq).astype(np.float64)
    sbound = sbound + U * np.abs(Sq).astype(np.float64)         # the division by n - 1, undone here: one rounding
    assert np.all(serr <= 10 * sbound), (tag, float(np.max(serr[sbound > 0] / sbound[sbound > 0])))
    if np.any(sbound > 0):
        WORST["cov"] = max(WORST["cov"], float(np.max(serr[sbound > 0] / sbound[sbound > 0])))
    # the correlation: NaN on constant rows and columns, 1.0 on the diagonal, within the propagated bound elsewhere
    corr = r["corr"]
    rq, rb = DR.corr(Sq, 10 * sbound)
    live = ~const
    assert np.all(np.isnan(corr[const, :])) and np.all(np.isnan(corr[:, const])), tag
    assert np.all(np.diag(corr)[live] == 1.0) and np.all(np.abs(corr[np.ix_(live, live)]) <= 1.0), tag
    cerr = np.abs(corr[np.ix_(live, live)].astype(LD) - rq[np.ix_(live, live)]).astype(np.float64)
    cb = rb[np.ix_(live, live)] + 8 * U
    if live.any():
        assert np.all(cerr <= cb), (tag, float(np.max(cerr / cb)))
        WORST["corr"] = max(WORST["corr"], float(np.max(cerr / cb)))
    RHAT[tag] = (r["rhat"].copy(), rows)                        # check 5: test_rhat_against_long_double


def check_rhat(tag, rhat, rows, worst=WORST):
    """Check 5.  Returns the worst relative error over the bound 8 h 2^-52."""
    WORST = worst
    n = rows.shape[0]
    h = n // 2
    const = rows.min(axis=0) == rows.max(axis=0)
    rh = ER.rhat(rows)
    assert np.all(np.isnan(rh[const].astype(np.float64))) and np.all(np.isnan(rhat[const])), tag
    rel = (np.abs(rhat[~const].astype(LD) - rh[~const]) / rh[~const]).astype(np.float64)
    ratio = float(rel.max() / (8 * h * U))
    cols = np.flatnonzero(~const)
    print(f"R-hat {tag}: worst relative error {rel.max():.3g} = {ratio:.3g} x the bound 8 h 2^-52, column {cols[int(rel.argmax())]}")
    WORST["rhat"] = max(WORST["rhat"], ratio)
    assert np.all(rel <= 8 * h * U), (tag, ratio)
