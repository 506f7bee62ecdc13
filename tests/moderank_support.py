"""What the suites of the mode table's rank diagnostics share (tests/test_moderank_gpu.py, tests/test_mode_columns_gpu.py):
the checks of one column's rank_series and of one rank_diag result against moderank_reference, ess_reference and
modediag_reference.  Importing this module needs no GPU."""
import math

import numpy as np

import ess_reference as ER
import modediag_reference as DR
import moderank_reference as RR
from support import LD, bits

U = 2.0 ** -52
WORST = {"z": 0.0, "lag": 0.0, "rhat": 0.0}


def snapshot(mt, L, cols=None, scratch=0):
    r = mt.rank_diag(L, cols, scratch)
    for s, name in enumerate(RR.SERIES):
        r["acov_" + name] = mt.rank_acov(s)
    return r


def same(a, b, tag):
    assert a.keys() == b.keys(), tag
    for k in a:
        if isinstance(a[k], np.ndarray) and a[k].dtype == np.float64:
            assert np.array_equal(bits(a[k]), bits(b[k])), (tag, k)
        elif isinstance(a[k], float):
            assert bits(a[k]) == bits(b[k]), (tag, k)
        else:
            assert np.array_equal(a[k], b[k]), (tag, k)


def nan_eq(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b)))


def check_column(tag, mt, c, v, n, q, rng, worst=WORST):
    """Checks 1 and 3 of one column: v = the library's derive rows of column c.  Returns rank_series(c)."""
    WORST = worst
    s = mt.rank_series(c)
    assert np.array_equal(s["rank2"], RR.rank2(v)) and int(s["rank2"].sum()) == n * (n + 1), (tag, c)
    assert bits(s["med"]) == bits(RR.median(v)) and bits(s["q05"]) == bits(RR.quantile(v, 0.05)) == bits(q[0, c]), (tag, c)
    assert bits(s["q95"]) == bits(RR.quantile(v, 0.95)) == bits(q[1, c]), (tag, c)
    f = np.abs(v - np.float64(s["med"]))                                   # the one subtraction
    assert np.array_equal(s["rank2_fold"], RR.rank2(f)) and int(s["rank2_fold"].sum()) == n * (n + 1), (tag, c)
    S = s["series"]
    assert np.array_equal(S[2], (v <= s["q05"]).astype(np.float64)) and np.array_equal(S[3], (v <= s["q95"]).astype(np.float64)), (tag, c)
    assert np.array_equal(bits(s["mean"]), bits(RR.welford_mean(S.T))), (tag, c)
    for r2, z in ((s["rank2"], S[0]), (s["rank2_fold"], S[1])):
        ur, first = np.unique(r2, return_index=True)
        uz = z[first]
        assert np.array_equal(bits(z), bits(uz[np.searchsorted(ur, r2)])), (tag, c, "z is a function of rank2")
        assert np.all(np.diff(uz) > 0), (tag, c, "z increases with rank2")
        mirror = 2 * (n + 1) - ur                                           # antisymmetry where both ranks occur
        both = np.isin(mirror, ur)
        zm = uz[np.searchsorted(ur, mirror[both])]
        mid = ur[both] == n + 1
        assert np.array_equal(bits(uz[both][~mid]), bits(-zm[~mid])) and np.all(bits(uz[both][mid]) == 0), (tag, c, "antisymmetry")
        if ur.size > 2050:
            keep = np.unique(np.concatenate([[0, ur.size - 1], rng.choice(ur.size, 2000, replace=False)]))
            ur, uz = ur[keep], uz[keep]
        _, bound, exact = RR.z_exact(ur, n)
        err = RR.z_error(uz, exact)
        ok = bound > 0
        assert np.all(err <= bound), (tag, c, float(np.max(err[ok] / bound[ok])))
        if ok.any():
            WORST["z"] = max(WORST["z"], float(np.max(err[ok] / bound[ok])))
    return s


def check_results(tag, r, n, L, series_of, worst=WORST):
    """Checks 1 (arrays), 4 of one rank_diag result r (with the four acov); series_of: {position in the selection: rank_series}."""
    WORST = worst
    ns = r["cols"].size
    assert r["n_used"] == n and r["lag"] == L == ER.lag_limit(L, n), tag
    floor = 1.0 / math.log10(float(n))
    fin = {}
    for s, name in enumerate(RR.SERIES):
        A = r["acov_" + name]
        assert A.shape == (L + 1, ns), tag
        tau, ess, cut = ER.finish(A, n)
        fin[name] = (tau, ess)
        assert np.array_equal(cut, r["cut"][s]), (tag, name)
    for got, (want, tau) in ((r["tau_bulk"], (fin["z"][0], fin["z"][0])), (r["ess_bulk"], (fin["z"][1], fin["z"][0])),
                             (r["ess_q05"], (fin["i05"][1], fin["i05"][0])), (r["ess_q95"], (fin["i95"][1], fin["i95"][0]))):
        on_floor = np.abs(tau - floor) <= 4 * U * floor
        ok = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)) | (on_floor & (np.abs(got - want) <= 4 * U * np.abs(want)))
        assert np.all(ok), (tag, np.flatnonzero(~ok))
    assert nan_eq(r["ess_tail"], RR.pick(r["ess_q05"], r["ess_q95"], True)), tag
    assert nan_eq(r["rhat"], RR.pick(r["rhat_bulk"], r["rhat_fold"], False)), tag
    want_t = RR.totals(r["cols"], r["ess_bulk"], r["ess_tail"], r["rhat"], r["cut"][0], r["acov_z"][0], L, n)
    for k in RR.TOTALS:
        assert r[k] == want_t[k] or (isinstance(want_t[k], float) and np.isnan(want_t[k]) and np.isnan(r[k])), (tag, k, r[k], want_t[k])
    h = n // 2
    for k, s in series_of.items():
        d, e = DR.centred(s["series"].T, s["mean"])
        Aq, bound = DR.lag(d, e, L)
        A = np.stack([r["acov_" + name][:, k] for name in RR.SERIES], axis=1)
        err = np.abs(A.astype(LD) - Aq).astype(np.float64)
        ok = bound > 0
        assert np.all(err <= 10 * bound), (tag, k, float(np.max(err[ok] / bound[ok])))
        if ok.any():
            WORST["lag"] = max(WORST["lag"], float(np.max(err[ok] / bound[ok])))
        rh = ER.rhat(d)
        for j, name in ((0, "rhat_bulk"), (1, "rhat_fold")):
            if np.isnan(float(rh[j])):
                assert np.isnan(r[name][k]), (tag, k, name)
                continue
            rel = float(abs(LD(r[name][k]) - rh[j]) / rh[j])
            WORST["rhat"] = max(WORST["rhat"], rel / (8 * h * U))
            assert rel <= 8 * h * U, (tag, k, name, rel / (8 * h * U))
        const = s["rank2"].min() == s["rank2"].max()
        if const:
            assert np.all(bits(s["series"][:2]) == 0) and np.all(s["series"][2:] == 1.0) and np.all(s["rank2"] == n + 1), (tag, k)
            for name in RR.OUT:
                assert np.isnan(r[name][k]), (tag, k, name)
            assert np.all(r["cut"][:, k] == 0), (tag, k)
