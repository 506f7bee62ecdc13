"""What the window-LOO suite (tests/test_summary_wloo_gpu.py) shares with the long-grid suite
(tests/test_summary_long_grids_gpu.py): the three passes, the bit-for-bit comparisons, the partition and the totals from the
library's own arrays, the exact cutoff and tail length of every window from the library's own l, and the check against
wloo_reference with the bounds that tests/test_summary_wloo_gpu.py's docstring states.  Importing this module needs no GPU."""
import numpy as np

from loopit_support import PIT_ARRAYS, SEEDS, _key, same_pit
from predictive_reference import totals_from_pit
from summary_support import ULP, diff, exact_structure, perturbed, perturbed_rows, same, x_of
from support import bits
from tamcmc_amd import capi
from window_reference import gathered, partition
from wloo_reference import wloo_reference

LOO_KEYS = ("elpd_lwo", "pareto_k", "cutoff")
CHECKED = LOO_KEYS + ("loo_log_cdf", "loo_log_sf", "loo_pit", "is_ess", "log_wsum")
PER_WINDOW = LOO_KEYS + ("tail_len",) + PIT_ARRAYS           # every per-window result of the mode and its sub-mode


def same_wloo(r1, r2):
    return all(np.array_equal(bits(r1[k]), bits(r2[k])) for k in LOO_KEYS) and \
        all(np.array_equal(r1[k], r2[k]) for k in ("tail_len", "first_bin", "last_bin")) and \
        all(np.array_equal(bits(float(r1[k])), bits(float(r2[k]))) for k in capi.Summary.WLOO_TOTALS)


def run_wloo(acc, pushes, Wd, first=0, block=0, loo_pushes=None, pit_pushes=None, **kw):
    """Fold pass, window-LOO pass and PIT pass.  Returns (pit result, loo result, fold result); wloo_result must give the
    same bits before wloo_pit_begin, after it and after the pass, and the fold results must not move."""
    with capi.Summary(acc, block, **kw) as s:
        for P in pushes:
            s.push(P)
        fold = s.result()
        nw = s.wloo_begin(Wd, first)
        for P in (pushes if loo_pushes is None else loo_pushes):
            s.push(P)
        loo = s.wloo_result()
        assert loo["n_windows"] == nw and loo["elpd_lwo"].shape == (nw,)
        s.wloo_pit_begin()
        assert same_wloo(s.wloo_result(), loo), "wloo_result changed over wloo_pit_begin"
        for P in (pushes if pit_pushes is None else pit_pushes):
            s.push(P)
        r = s.wloo_pit_result()
        assert same_wloo(s.wloo_result(), loo), "wloo_result changed over the PIT pass"
        assert same_pit(s.wloo_pit_result(), r), "a second wloo_pit_result without another pass"
        assert same(s.result(), fold), "the fold results changed in window-LOO mode"
        s.wloo_end()
    return r, loo, fold


def check_geometry(tag, loo, Nx, Wd, first):
    f, begin, end = partition(Nx, Wd, first)
    assert loo["n_windows"] == begin.size and loo["W"] == Wd and loo["first"] == f, tag
    assert np.array_equal(loo["first_bin"], begin) and np.array_equal(loo["last_bin"], end - 1), tag


def check_totals(tag, res, loo, fold):
    """The totals are their stated expressions on the returned arrays."""
    LDt = np.longdouble                                        # (np.cumsum: one term after the other, as the host adds them)
    e = np.cumsum(np.asarray(loo["elpd_lwo"]).astype(LDt))[-1]
    assert loo["elpd_lwo_total"] == float(e), tag
    assert loo["p_lwo"] == float(np.cumsum(np.asarray(fold["lppd"]).astype(LDt))[-1] - e), (tag, "p_lwo")
    kh = np.asarray(loo["pareto_k"])
    assert loo["n_k_high"] == int((kh > 0.7).sum()) and loo["n_k_inf"] == int(np.isposinf(kh).sum()) and loo["k_max"] == np.nanmax(kh), tag
    pit, lc, ls, ess = (np.asarray(res[k]) for k in ("loo_pit", "loo_log_cdf", "loo_log_sf", "is_ess"))
    ok = ~np.isnan(pit)
    want = np.where(lc < ls, np.exp(lc), -np.expm1(ls))
    assert np.all(np.abs(pit[ok] - want[ok]) <= 2.0 * np.spacing(want[ok])), (tag, "loo_pit from the smaller tail")
    assert np.all((pit[ok] >= 0) & (pit[ok] <= 1)) and np.all(lc[ok] <= 0) and np.all(ls[ok] <= 0), tag
    if ok.any():
        D, hist = totals_from_pit(pit[ok])
        assert res["loo_ks_D"] == D and np.array_equal(res["loo_pit_hist"], hist), (tag, "ks_D / pit_hist")
    for key, arr in (("min_loo_log_sf", ls), ("min_loo_log_cdf", lc), ("min_is_ess", ess)):
        v = np.asarray(arr, dtype=np.float64)
        k = -1 if np.all(np.isnan(v)) else int(np.argmin(np.where(np.isnan(v), np.inf, v)))
        assert res["bin_" + key] == k and (k < 0 or bits(res[key]) == bits(v[k])), (tag, key)


def window_sums_of(l, Nx, Wd, first):
    """(n, n_windows): the library's own l (library_l) added over each window in float64, one bin after the other in ascending
    order starting from the first term -- tmw_sum's order (tamcmc_wloo.h).  A loop over the W columns: np.sum and
    np.add.reduceat add pairwise."""
    f, begin, end = partition(Nx, Wd, first)
    length = end - begin
    S = np.array(l[:, begin])
    for i in range(1, int(length.max())):
        more = length > i
        S[:, more] = S[:, more] + l[:, begin[more] + i]
    return S


def exact_windows(tag, loo, l, Nx, Wd, first):
    """cutoff of every window, bit for bit, is the order statistic sort(-S)[n - M - 1] of the float64 ascending window sums S
    of the library's own l, and tail_len the count above it (summary_support.exact_structure with "bin" read as "window"): a
    bin in the wrong window or slot, or a window one bin short, changes S and with it the cutoff.  Returns S."""
    S = window_sums_of(l, Nx, Wd, first)
    assert S.shape == (len(l), loo["n_windows"]), tag
    exact_structure(tag, loo, S)
    return S


def at_windows(d, sel, nw):
    """The per-window arrays of a result taken at the windows `sel`; everything else as it is."""
    for k in PER_WINDOW:
        assert k not in d or np.asarray(d[k]).shape == (nw,), k
    return {k: (np.asarray(v)[sel] if k in PER_WINDOW + ("first_bin", "last_bin") else v) for k, v in d.items()}


def _diff(k, a, b):
    a, b = np.asarray(a), np.asarray(b)
    if k == "cutoff":                                          # NaN where there is no tail rule (n = 1): both, or neither
        na, nb = np.isnan(a.astype(np.float64)), np.isnan(b.astype(np.float64))
        if not np.array_equal(na, nb):
            return np.inf
        a, b = a[~na], b[~nb]
        if a.size == 0:
            return 0.0
    return diff(_key(k), a, b)


WORST = {}


def check_reference(tag, res, loo, rows, y, groups, rel, Wd, first=0, like=0, p=1, sigma=None, pool=None):
    """res and loo against wloo_reference on `rows`, with the bounds of the window-LOO suite's docstring.  Returns the reference.
    With `pool`, a dict, the case is made of several grids: the errors and the two bounds are maxima over the windows of all
    of them -- this call adds its own, and check_pool() holds the one against the other once the case is complete."""
    n = len(rows)
    ref = wloo_reference(rows, y, Wd, first, like, p, sigma)
    keys = CHECKED + ("elpd_from_weights", "log_wsum_direct")
    d = {k: 0.0 for k in keys}
    for seed in SEEDS:
        pr = perturbed_rows(rows, rel, seed, groups)
        px = perturbed(x_of(pr, y, like, p, sigma), rel, seed + 1000, groups)
        pert = wloo_reference(pr, y, Wd, first, like, p, sigma, xbins=px)
        for k in keys:
            d[k] = max(d[k], _diff(k, pert[k], ref[k]))
    r64 = wloo_reference(rows, y, Wd, first, like, p, sigma, dtype=np.float64)
    b64 = {k: _diff(k, r64[k], ref[k]) for k in keys}
    for k in keys:
        d[k] = max(d[k], b64[k])
    for k, dk in d.items():
        assert np.isfinite(dk), (tag, k, "the reference runs disagree on where the value is finite: the case has no bound")
    assert np.array_equal(loo["tail_len"], ref["tail_len"]), (tag, "tail_len")
    assert np.array_equal(np.isinf(loo["pareto_k"]), np.isinf(ref["pareto_k"])), (tag, "where k-hat is +inf")
    got = dict(res, elpd_from_weights=loo["elpd_lwo"], log_wsum_direct=res["log_wsum"], **{k: loo[k] for k in LOO_KEYS})
    ratios = {}
    for k, dk in d.items():
        err = _diff(k, got[k], ref[k])
        ratios[k] = err / (10.0 * dk) if dk > 0 else (0.0 if err == 0 else np.inf)
    print(f"RATIO wloo {tag}: " + " ".join(f"{k}={v:.3g} (bound {10.0 * d[k]:.3g})" for k, v in ratios.items()))
    if pool is not None:
        for k in keys:
            pool.setdefault("d", {})[k] = max(pool.get("d", {}).get(k, 0.0), d[k])
            pool.setdefault("err", {})[k] = max(pool.get("err", {}).get(k, 0.0), _diff(k, got[k], ref[k]))
        ratios = {}
    seen = WORST.setdefault("oracle" if tag.startswith("oracle") else "own", {})
    for k, v in ratios.items():
        seen[k] = max(seen.get(k, 0.0), v)
    print("WORST wloo so far: " + repr(WORST))
    lc, ls, ess = np.asarray(res["loo_log_cdf"]), np.asarray(res["loo_log_sf"]), np.asarray(res["is_ess"])
    one = np.abs(np.exp(lc) + np.exp(ls) - 1.0)
    shape = int(p) * Wd
    slack = (n + 2) * ULP + (10.0 * max(b64["loo_log_cdf"], b64["loo_log_sf"]) if like == 0 and shape > 1 else 0.0)
    print(f"SELF wloo {tag}: |P + Q - 1| = {float(np.nanmax(one)):.3g} (bound {slack:.3g}); is_ess in [{float(np.nanmin(ess)):.6g}, "
          f"{float(np.nanmax(ess)):.6g}] of n = {n}")
    for k, v in ratios.items():
        assert v <= 1.0, (tag, k, v)
    assert np.all(one[~np.isnan(one)] <= slack), (tag, float(np.nanmax(one)), slack)
    fin = ~np.isnan(ess)
    assert np.all(ess[fin] >= 1.0 - 1e-12) and np.all(ess[fin] <= n * (1.0 + 1e-12)), (tag, "is_ess outside 1 ... n")
    return ref


def check_reference_at(tag, windows, res, loo, rows, y, groups, rel, Wd, first=0, pool=None):
    """check_reference on the windows `windows` of a grid alone, with window 0 and the last one: the reference is given the
    gathered grid of window_reference.gathered() -- window 0's bins, the chosen whole middle windows, the last window's bins --
    whose partition (W, first) is exactly those windows (tests/test_summary_wloo_host.py pins that form to the whole-grid
    reference bit for bit).  rows: the model rows of the whole grid."""
    Nx, nw = rows.shape[1], loo["n_windows"]
    sel, cols, f = gathered(windows, Nx, Wd, first)
    return check_reference(tag, at_windows(res, sel, nw), at_windows(loo, sel, nw), rows[:, cols], y[cols], groups, rel, Wd, f, pool=pool)


def check_pool(tag, pool):
    ratios = {k: (pool["err"][k] / (10.0 * dk) if dk > 0 else (0.0 if pool["err"][k] == 0 else np.inf)) for k, dk in pool["d"].items()}
    print(f"RATIO wloo {tag}: " + " ".join(f"{k}={v:.3g} (bound {10.0 * pool['d'][k]:.3g})" for k, v in ratios.items()))
    seen = WORST.setdefault("own", {})
    for k, v in ratios.items():
        seen[k] = max(seen.get(k, 0.0), v)
        assert v <= 1.0, (tag, k, v)
