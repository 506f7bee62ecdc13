"""What the LOO-PIT suite (tests/test_summary_loopit_gpu.py) shares with the long-grid suite
(tests/test_summary_long_grids_gpu.py): the three passes, the bit-for-bit comparisons, the totals from the library's own
arrays and the check against loopit_reference with the bounds that tests/test_summary_loopit_gpu.py's docstring states.
Importing this module needs no GPU."""
import numpy as np

from loopit_reference import loopit_reference
from predictive_reference import totals_from_pit
from summary_support import ULP, diff, perturbed, perturbed_rows, same, x_of
from support import bits
from tamcmc_amd import capi

PIT_ARRAYS = capi.Summary.LOO_PIT_ARRAYS
PIT_TOTALS = capi.Summary.LOO_PIT_TOTALS
LOO_KEYS = ("elpd_loo", "pareto_k", "cutoff")
SEEDS = (1, 2, 3)
CHECKED = ("loo_log_cdf", "loo_log_sf", "loo_pit", "is_ess", "log_wsum")


def same_loo(r1, r2):
    return all(np.array_equal(bits(r1[k]), bits(r2[k])) for k in LOO_KEYS) and np.array_equal(r1["tail_len"], r2["tail_len"]) and \
        all(np.array_equal(bits(float(r1[k])), bits(float(r2[k]))) for k in capi.Summary.LOO_TOTALS)


def same_pit(r1, r2):
    return all(np.array_equal(bits(r1[k]), bits(r2[k])) for k in PIT_ARRAYS) and np.array_equal(r1["loo_pit_hist"], r2["loo_pit_hist"]) and \
        all(np.array_equal(bits(float(r1[k])), bits(float(r2[k]))) for k in PIT_TOTALS)


def run_pit(acc, pushes, block=0, pit_pushes=None, **kw):
    """Fold pass, LOO pass and PIT pass.  Returns (pit result, loo result, fold result); loo_result must give the same bits
    before loo_pit_begin, after it and after the pass, and the fold results must not move."""
    with capi.Summary(acc, block, **kw) as s:
        for P in pushes:
            s.push(P)
        fold = s.result()
        s.loo_begin()
        for P in pushes:
            s.push(P)
        loo = s.loo_result()
        s.loo_pit_begin()
        assert same_loo(s.loo_result(), loo), "loo_result changed over loo_pit_begin"
        for P in (pushes if pit_pushes is None else pit_pushes):
            s.push(P)
        r = s.loo_pit_result()
        assert same_loo(s.loo_result(), loo), "loo_result changed over the PIT pass"
        assert same_pit(s.loo_pit_result(), r), "a second loo_pit_result without another pass"
        assert same(s.result(), fold), "the fold results changed in the LOO-PIT sub-mode"
        s.loo_end()
    return r, loo, fold


def _key(k):
    return "pit" if k == "loo_pit" else k                     # summary_support.diff: absolute for a pit, relative otherwise


def check_totals(tag, res):
    """The totals are their stated expressions on the returned arrays; everything in range."""
    pit, lc, ls, ess = (np.asarray(res[k]) for k in ("loo_pit", "loo_log_cdf", "loo_log_sf", "is_ess"))
    ok = ~np.isnan(pit)
    want = np.where(lc < ls, np.exp(lc), -np.expm1(ls))
    assert np.all(np.abs(pit[ok] - want[ok]) <= 2.0 * np.spacing(want[ok])), (tag, "loo_pit from the smaller tail")
    assert np.all((pit[ok] >= 0) & (pit[ok] <= 1)) and np.all(lc[ok] <= 0) and np.all(ls[ok] <= 0), tag
    if ok.any():
        D, hist = totals_from_pit(pit[ok])
        assert res["loo_ks_D"] == D and np.array_equal(res["loo_pit_hist"], hist), (tag, "ks_D / pit_hist")

    def first_min(v):
        v = np.asarray(v, dtype=np.float64)
        if np.all(np.isnan(v)):
            return np.nan, -1
        k = int(np.argmin(np.where(np.isnan(v), np.inf, v)))
        return v[k], k
    for key, arr in (("min_loo_log_sf", ls), ("min_loo_log_cdf", lc), ("min_is_ess", ess)):
        v, k = first_min(arr)
        assert bits(res[key]) == bits(v) and res["bin_" + key] == k, (tag, key)


WORST = {}


def check_reference(tag, res, loo, rows, y, groups, rel, like=0, p=1, sigma=None, with_f64=True, sel=None):
    """res (and the elpd_loo of `loo`) against loopit_reference on `rows`, with the bounds of the LOO-PIT suite's docstring."""
    n = len(rows)
    if sel is not None:
        rows, y = rows[:, sel], y[sel]
        sigma = None if sigma is None else sigma[sel]
        res = {k: (np.asarray(v)[sel] if k in PIT_ARRAYS else v) for k, v in res.items()}
        loo = dict(loo, elpd_loo=np.asarray(loo["elpd_loo"])[sel])
    ref = loopit_reference(rows, y, like, p, sigma)
    keys = CHECKED + ("elpd_from_weights", "log_wsum_direct")
    d = {k: 0.0 for k in keys}
    for seed in SEEDS:
        pr = perturbed_rows(rows, rel, seed, groups)
        px = perturbed(x_of(pr, y, like, p, sigma), rel, seed + 1000, groups)
        pert = loopit_reference(pr, y, like, p, sigma, x=px)
        for k in keys:
            d[k] = max(d[k], diff(_key(k), pert[k], ref[k]))
    b64 = {k: 0.0 for k in keys}
    if with_f64:
        r64 = loopit_reference(rows, y, like, p, sigma, dtype=np.float64)
        b64 = {k: diff(_key(k), r64[k], ref[k]) for k in keys}
        for k in keys:
            d[k] = max(d[k], b64[k])
    for k, dk in d.items():
        assert np.isfinite(dk), (tag, k, "the reference runs disagree on where the value is finite: the case has no bound")
    got = dict(res, elpd_from_weights=loo["elpd_loo"], log_wsum_direct=res["log_wsum"])
    ratios = {}
    for k, dk in d.items():
        err = diff(_key(k), got[k], ref[k])
        ratios[k] = err / (10.0 * dk) if dk > 0 else (0.0 if err == 0 else np.inf)
    print(f"RATIO loopit {tag}: " + " ".join(f"{k}={v:.3g} (bound {10.0 * d[k]:.3g})" for k, v in ratios.items()))
    seen = WORST.setdefault("oracle" if tag.startswith("oracle") else "own", {})
    for k, v in ratios.items():
        seen[k] = max(seen.get(k, 0.0), v)
    print("WORST loopit so far: " + repr(WORST))
    lc, ls, ess = np.asarray(res["loo_log_cdf"]), np.asarray(res["loo_log_sf"]), np.asarray(res["is_ess"])
    one = np.abs(np.exp(lc) + np.exp(ls) - 1.0)
    slack = (n + 2) * ULP + (10.0 * max(b64["loo_log_cdf"], b64["loo_log_sf"]) if like == 0 and int(p) > 1 else 0.0)
    print(f"SELF loopit {tag}: |P + Q - 1| = {float(np.nanmax(one)):.3g} (bound {slack:.3g}); is_ess in [{float(np.nanmin(ess)):.6g}, "
          f"{float(np.nanmax(ess)):.6g}] of n = {n}")
    for k, v in ratios.items():
        assert v <= 1.0, (tag, k, v)
    assert np.all(one[~np.isnan(one)] <= slack), (tag, float(np.nanmax(one)), slack)
    fin = ~np.isnan(ess)
    assert np.all(ess[fin] >= 1.0 - 1e-12) and np.all(ess[fin] <= n * (1.0 + 1e-12)), (tag, "is_ess outside 1 ... n")
    return ref
