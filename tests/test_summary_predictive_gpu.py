"""Posterior predictive check of a stored chain on the GPU (tamcmc_summary_predictive_*, include/tamcmc_accel.h;
tamcmc_predictive.hip): per bin the log predictive CDF and survival function of the datum averaged over the chain, the PIT
and the mean residual, accumulated beside the fold kernel in the pass the user already makes.

Reference: tests/predictive_reference.py, an independent numpy transcription of the definitions in the header, run in long
double (its erfc is pinned against mpmath by tests/test_summary_predictive_host.py).

Exact checks (no tolerance): every result bit for bit independent of block_chains and of the split into pushes; the fold
results bit for bit the same with the check on and off; the predictive results untouched by a quantile pass and a LOO pass;
y = 0 gives log_cdf = -inf, log_sf = 0, pit = 0; ks_D, pit_hist and the two minima recomputed from the library's own arrays.

Against the reference on the GPU's own model rows (eval_batch with every chain in model_rows) the bound is, per case and
per quantity (the maximum over the bins), 10 x the larger of
    (a) the reference's own change when every model value is perturbed by 2^-50 relative (one random sign per value), and
    (b) the difference between the reference run in float64 and in long double (both sum over the samples one after the
        other, so (b) carries the n 2^-52 accumulation error of a float64 stream).
Differences are relative to max(1, |value|) for log_cdf, log_sf and mean_resid and absolute for pit.  The factor 10: one
random perturbation samples the typical sensitivity, not the worst.  Against the reference on the oracle's rows
(pyoracle.generate_batch(..., want_models=True)) the perturbation is 1e-12 relative -- the project's per-bin model bar --
one factor per distinct parameter row and bin, the maximum over five seeds, and the bound is 10 x that change.
Self-check: exp(log_cdf) + exp(log_sf) = 1 within (n + 2) 2^-52; for p > 1, where the two tails come from different
branches with an error of up to bound (b), within that bound plus (n + 2) 2^-52 instead.
Every worst ratio is printed before it is asserted (pytest -s).

Worst ratios observed on an MI355X over all cases below: on the GPU's own rows log_cdf 0.40, log_sf 0.27 and pit 0.42 (all
p = 64; for p <= 3 and chi_square log_cdf 0.36 -- 2 bins, 37 samples, a bound of 2e-16 -- and under 0.07 otherwise),
mean_resid 0.14 (200 samples); at 70 001 samples 8.7e-4, 9.9e-4, 1.6e-3 and 0.095; on the oracle's rows log_cdf 1.1e-4,
log_sf 1.1e-4, pit 1.3e-4, mean_resid 3.9e-4.  |P + Q - 1| was 2.2e-16 or less for p <= 3 and chi_square and 1.1e-14 at
p = 64.  With plain (uncompensated) sums the 2-bin case misses its log_cdf bound by a factor 1.25: an absolute error of
4e-16 on a value of -1e-9.
"""
import functools

import numpy as np
import pytest

import workloads as W
from predictive_reference import predictive_reference, totals_from_pit
from summary_support import (c2_case, c2_chain, check_pit, check_tails_reference, diff, edited, gpu_rows, perturbed_rows, row_groups,
                             same, same_pred, sigma_of, spectrum_for, true_model)
from support import bits, pyorc
from tamcmc_amd import capi, synth

pytestmark = pytest.mark.gpu

KEYS = capi.Summary.PREDICTIVE_ARRAYS


def check_reference(tag, res, rows, y, groups, rel, seeds, with_f64, like=0, p=1, sigma=None):
    """res against predictive_reference(rows) with the bounds of the module docstring; then the self-check and the
    totals.  Returns the reference."""
    reference = functools.partial(predictive_reference, like=like, p=p, sigma=sigma)
    ref = check_tails_reference(reference, "predictive", KEYS, tag, res, rows, y, groups, rel, seeds, with_f64, like, p, f64_always=False)
    check_totals(tag, res, len(rows))
    return ref


def check_totals(tag, res, n, n_rejected=0):
    """pit from the smaller tail, within 2 ulp; every total recomputed from the library's own arrays: exact."""
    assert res["n_used"] == n and res["n_rejected"] == n_rejected, tag
    lc, ls, pit = check_pit(tag, res)
    D, hist = totals_from_pit(pit)
    assert res["ks_D"] == D, (tag, res["ks_D"], D)
    assert np.array_equal(res["pit_hist"], hist) and int(res["pit_hist"].sum()) == pit.size, (tag, res["pit_hist"], hist)
    assert res["bin_min_log_sf"] == int(np.argmin(ls)) and res["min_log_sf"] == ls.min(), tag      # (argmin: the first of equals)
    assert res["bin_min_log_cdf"] == int(np.argmin(lc)) and res["min_log_cdf"] == lc.min(), tag


def run(acc, pushes, block=0):
    """A fold pass with the check on.  Returns (predictive result, fold result)."""
    with capi.Summary(acc, block, predictive=True) as s:
        for P in pushes:
            s.push(P)
        return s.predictive_result(), s.result()


def check_edits(tag, res, where, y):
    for name, k in where.items():
        lc, ls, pit, mr = (res[key][k] for key in ("log_cdf", "log_sf", "pit", "mean_resid"))
        if name == "x2000":
            assert np.isfinite(ls) and ls < -745.0 and pit == 1.0 and res["bin_min_log_sf"] == k, (tag, name, ls, pit)
        elif name == "zero":
            assert lc == -np.inf and ls == 0.0 and pit == 0.0 and mr == 0.0, (tag, name, lc, ls, pit)
        elif name == "tiny":
            assert np.isfinite(lc) and lc < -600.0 and -1e-290 < ls <= 0.0 and 0.0 <= pit < 1e-290, (tag, name, lc, ls, pit)
        elif name == "negative":
            assert lc == -np.inf and ls == 0.0 and pit == 0.0 and mr < 0.0, (tag, name, lc, ls, pit)
        elif name == "plus40":
            assert np.isfinite(ls) and ls < -1000.0 and pit == 1.0, (tag, name, ls, pit)
        elif name == "minus40":
            assert np.isfinite(lc) and lc < -1000.0 and 0.0 <= pit < 1e-300, (tag, name, lc, pit)


@pytest.mark.parametrize("Nx", [2, 63, 64, 65, 129, 700])
def test_grid_ends(accel_mod, Nx):
    """One bin per thread, 256 threads per workgroup, waves of 64: a partial wave, exactly one, one and a bin, two and a bin,
    several workgroups.  Id 2, p = 1, 37 samples, with the four data edits."""
    w, y0, P, _, _ = c2_case(Nx)
    y, where = edited(y0)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        res, _ = run(acc, [P])
    check_reference(f"grid-ends Nx={Nx}", res, rows, y, np.arange(len(P)), 2.0 ** -50, (1,), True)
    check_edits(f"grid-ends Nx={Nx}", res, where, y)


@pytest.mark.parametrize("S", [1, 2, 8, 9, 70, 200])
def test_sample_counts_and_order(accel_mod, S):
    """1 and 2 samples; a full group of 8 row loads and one more; several blocks.  Every result is bit for bit independent of
    block_chains (1, 7, 64, the default) and of one push against three uneven ones, and the fold results are bit for bit
    those of a summary without the check."""
    w, y0, P = c2_chain(65, S)
    y, where = edited(y0)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        first, fold = run(acc, [P], 1)
        for B in (7, 64, 0):
            res, f = run(acc, [P], B)
            assert same_pred(res, first), ("block_chains", B)
            assert same(f, fold), ("fold results, block_chains", B)
        if S >= 3:
            a, b = S // 3, S // 3 + 1
            res, f = run(acc, [P[:a], P[a:b], P[b:]], 7)
            assert same_pred(res, first) and same(f, fold), "three unequal pushes"
        with capi.Summary(acc, 7) as s:                                      # the check off
            s.push(P)
            assert same(s.result(), fold), "the fold results differ with the check on"
    check_reference(f"S={S}", first, rows, y, np.arange(S), 2.0 ** -50, (1,), True)
    check_edits(f"S={S}", first, where, y)
    if S == 1:                                                               # one sample: the sample's own tails and residual
        assert np.array_equal(bits(first["mean_resid"]), bits(y / rows[0]))
        ok = y > 0
        assert np.array_equal(bits(first["log_sf"][ok]), bits(-(y / rows[0])[ok]))


@pytest.mark.parametrize("p", [1, 2, 3, 17, 64])
def test_likelihood_p(accel_mod, p):
    """chi(2,2p): the loop-free path and the two loops of p > 1; z = p y / M falls on both sides of p - 1 and of p in nearly
    every wave (y / M is exponential here)."""
    w, y0, P = c2_chain(129, 70)
    y, where = edited(y0)
    with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=float(p) + 0.5) as acc:      # truncated as everywhere
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        first, fold = run(acc, [P], 64)
        res, f = run(acc, [P[:9], P[9:10], P[10:]], 7)
        assert same_pred(res, first) and same(f, fold)
    z = p * y / rows
    assert np.any((z > 0) & (z < p - 1)) or p == 1
    assert np.any((z >= p - 1) & (z <= p)) and np.any(z > p)
    check_reference(f"p={p}", first, rows, y, np.arange(70), 2.0 ** -50, (1,), True, p=p)
    check_edits(f"p={p}", first, where, y)


@pytest.mark.parametrize("mid,Nx", [(2, 129), (11, 700)])
def test_chi_square(accel_mod, mid, Nx):
    """The Gaussian of standard deviation sigma / sqrt(2), with y at M + 40 sigma and at M - 40 sigma: about -1600, not -inf."""
    w = synth.workload_c2(Nx=Nx) if mid == 2 else synth.workload_c1(Nx=Nx)
    P = synth.chain_params(w, 37)
    sigma = sigma_of(Nx)
    y, where = edited(spectrum_for(w), 1, true_model(w), sigma)
    with accel_mod.Accel(mid, w["plength"], w["x"], y, sigma_y=sigma, likelihood_case=1) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        first, fold = run(acc, [P], 8)
        res, f = run(acc, [P[:20], P[20:]], 0)
        assert same_pred(res, first) and same(f, fold)
    check_reference(f"chi-square id={mid}", first, rows, y, np.arange(37), 2.0 ** -50, (1,), True, like=1, sigma=sigma)
    check_edits(f"chi-square id={mid}", first, where, y)


def test_local_model(accel_mod):
    """Id 11 on the fused one-tile launch, p = 1 and p = 3."""
    w = synth.workload_c1(Nx=700)
    P = synth.chain_params(w, 37)
    y, where = edited(spectrum_for(w))
    for p in (1, 3):
        with accel_mod.Accel(11, w["plength"], w["x"], y, likelihood_p=float(p)) as acc:
            assert acc.geometry()["tiles"] == 1
            _, st, rows = gpu_rows(acc, P)
            assert np.all(st == 0)
            res, _ = run(acc, [P], 9)
        check_reference(f"id 11 p={p}", res, rows, y, np.arange(37), 2.0 ** -50, (1,), True, p=p)
        check_edits(f"id 11 p={p}", res, where, y)


def test_rejected_samples(accel_mod):
    """A NaN parameter and an empty truncation window among 30 healthy samples, first and last in a block and alone in a block
    of one: left out of every bin and counted; the results are bit for bit those of the healthy samples alone."""
    w = W.make(2, Nx=3000)
    b = W.split(w)
    y, where = edited(spectrum_for(w))
    good = W.perturbed(w, 30, scale=0.002)
    empty = W.perturbed(w, 1, scale=0.002, seed=8)[0]
    empty[b["q"] + 1] = -1.0
    nan = W.perturbed(w, 1, scale=0.002, seed=9)[0]
    nan[b["z"] + 9] = np.nan
    P = np.array([empty] + list(good[:2]) + [nan, nan] + list(good[2:25]) + [empty] + list(good[25:]))
    sel = np.arange(0, 3000, 23)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, stg, rows = gpu_rows(acc, good)
        assert np.all(stg == 0)
        clean, clean_fold = run(acc, [good], 3)
        for B in (4, 1, 0):
            with capi.Summary(acc, B, predictive=True) as s:
                _, st = s.push(P)
                res, fold = s.predictive_result(), s.result()
            assert sorted(st[st != 0]) == [1, 1, 2, 2]
            assert res["n_used"] == 30 and res["n_rejected"] == 4
            res["n_rejected"] = 0
            assert same_pred(res, clean), B
            assert all(np.array_equal(bits(fold[k]), bits(clean_fold[k])) for k in capi.Summary.ARRAYS), B
        with capi.Summary(acc, 1, predictive=True) as s:                     # nothing but rejected samples: n = 0
            s.push(P[[0, 3]])
            r0 = s.predictive_result()
        assert r0["n_used"] == 0 and r0["n_rejected"] == 2 and all(np.all(np.isnan(r0[k])) for k in KEYS)
    check_totals("rejected", clean, 30)
    check_edits("rejected", clean, where, y)
    sub = {k: np.asarray(clean[k])[sel] for k in KEYS}
    ref = predictive_reference(rows[:, sel], y[sel])
    r64 = predictive_reference(rows[:, sel], y[sel], dtype=np.float64)
    pert = predictive_reference(perturbed_rows(rows[:, sel], 2.0 ** -50, 1, np.arange(30)), y[sel])
    for k in KEYS:
        bound = 10.0 * max(diff(k, pert[k], ref[k]), diff(k, r64[k], ref[k]))
        err = diff(k, sub[k], ref[k])
        print(f"RATIO predictive rejected {k}: {err / bound if bound > 0 else float(err != 0):.3g} (bound {bound:.3g})")
        assert err <= bound, (k, err, bound)


def test_at_length(accel_mod):
    """70 001 samples of a 65-bin grid in blocks of 4096: the n 2^-52 accumulation of the two running sums, and 18 blocks
    that straddle 65 535."""
    S = 70001
    w = synth.workload_c2(Nx=65)
    y, where = edited(spectrum_for(w))
    P = synth.chain_params(w, S)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        res, _ = run(acc, [P], 4096)
    check_reference("at-length", res, rows, y, np.arange(S), 2.0 ** -50, (1,), True)
    check_edits("at-length", res, where, y)


@pytest.mark.parametrize("name", ["c2-700-p1", "c2-129-p3", "c2-129-chi-square", "triples"])
def test_against_the_oracle(accel_mod, name):
    like, p, sigma = 0, 1, None
    if name == "c2-700-p1":
        w, y0, P, _, _ = c2_case(700)
    elif name == "triples":
        w, y0, P = c2_chain(65, 41)
        P = np.repeat(P, 3, axis=0)
    else:
        w, y0, P = c2_chain(129, 70)
        p = 3 if name.endswith("p3") else 1
    if name.endswith("chi-square"):
        like, sigma = 1, sigma_of(129)
        y, where = edited(y0, 1, true_model(w), sigma)
    else:
        y, where = edited(y0)
    _, rst, M = pyorc().generate_batch(2, w["plength"], w["x"], y, P, np.ones(len(P)), sigma_y=sigma, likelihood_case=like,
                                       likelihood_p=float(p), want_models=True)
    assert np.all(rst == 0)
    with accel_mod.Accel(2, w["plength"], w["x"], y, sigma_y=sigma, likelihood_case=like, likelihood_p=float(p)) as acc:
        res, _ = run(acc, [P])
    check_reference(f"oracle {name}", res, M, y, row_groups(P), 1e-12, (1, 2, 3, 4, 5), False, like=like, p=p, sigma=sigma)
    check_edits(f"oracle {name}", res, where, y)


def test_other_modes_leave_the_state_alone(accel_mod):
    """A quantile pass and a LOO pass over the same rows on the same object: the predictive results keep their bits, can be
    read inside either mode, and the fold goes on afterwards as if nothing had happened."""
    w, y0, P = c2_chain(129, 70)
    y, _ = edited(y0)
    extra = synth.chain_params(w, 5, seed=4242)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc, 16, predictive=True) as s:
            s.push(P)
            first = s.predictive_result()
            assert same_pred(s.predictive_result(), first), "a second result"
            s.quantiles_begin((0.16, 0.5, 0.84))
            s.push(P)
            assert same_pred(s.predictive_result(), first), "inside quantile mode, a pass pushed"
            s.quantiles_step()
            s.quantiles_end()
            assert same_pred(s.predictive_result(), first), "after a quantile pass"
            s.loo_begin()
            s.push(P)
            assert same_pred(s.predictive_result(), first), "inside LOO mode, a pass pushed"
            s.loo_result()
            s.loo_end()
            assert same_pred(s.predictive_result(), first), "after a LOO pass"
            s.push(extra)
            after, after_fold = s.predictive_result(), s.result()
        both, both_fold = run(acc, [P, extra], 16)
        assert same_pred(after, both) and same(after_fold, both_fold), "a summary that never entered a mode differs"
        with capi.Summary(acc, 16) as s:                                     # and the modes' results do not depend on the check
            s.push(P)
            loo_off = s.loo(P)
        with capi.Summary(acc, 16, predictive=True) as s:
            s.push(P)
            loo_on = s.loo(P)
        assert all(np.array_equal(bits(np.asarray(loo_on[k], dtype=np.float64)), bits(np.asarray(loo_off[k], dtype=np.float64)))
                   for k in ("elpd_loo", "pareto_k", "cutoff", "elpd_loo_total", "p_loo"))


def test_refusals_and_state(accel_mod):
    w, y0, P = c2_chain(65, 9)
    y, _ = edited(y0)
    T = np.ones(len(P))
    E = capi.E_INVALID

    def refused(fn, *a, **k):
        with pytest.raises(accel_mod.AccelError) as e:
            fn(*a, **k)
        assert e.value.code == E

    for p in (0.0, 0.9, 65.0):                                               # chi(2,2p) with p outside 1 ... 64
        with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=p) as acc:
            with capi.Summary(acc) as s:
                refused(s.predictive_enable)
            refused(capi.Summary, acc, 0, predictive=True)
            with capi.Summary(acc) as s:                                     # (the constructor's failed attempt left nothing behind)
                pass
    with accel_mod.Accel(2, w["plength"], w["x"], y, sigma_y=sigma_of(65), likelihood_case=1, likelihood_p=0.0) as acc:
        with capi.Summary(acc, predictive=True) as s:                        # chi_square does not look at p
            s.push(P)
            assert s.predictive_result()["n_used"] == 9
    acc = accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=64.0)
    s = capi.Summary(acc, 4)
    refused(s.predictive_result)                                             # not enabled
    refused(s.predictive_kernel_time)
    s.push(P[:3])
    refused(s.predictive_enable)                                             # after a push
    s.quantiles_begin((0.5,))
    refused(s.predictive_enable)                                             # in quantile mode
    s.reset()
    acc.begin(P, T)                                                          # a batch in flight
    refused(s.predictive_enable)
    acc.end()
    acc.arm(len(P))                                                          # a batch armed
    refused(s.predictive_enable)
    acc.disarm()
    s.predictive_enable()                                                    # after a reset: allowed
    refused(s.predictive_enable)                                             # twice
    r0 = s.predictive_result()                                               # n = 0: everything is NaN
    assert r0["n_used"] == 0 and r0["n_rejected"] == 0 and all(np.all(np.isnan(r0[k])) for k in KEYS)
    assert np.isnan(r0["ks_D"]) and np.isnan(r0["min_log_sf"]) and np.isnan(r0["min_log_cdf"])
    assert r0["bin_min_log_sf"] == -1 and r0["bin_min_log_cdf"] == -1 and not r0["pit_hist"].any()
    s.push(P)
    full = s.predictive_result()
    acc.begin(P, T)
    refused(s.predictive_result)
    acc.end()
    s.reset()                                                                # keeps the setting, clears the state
    refused(s.predictive_enable)
    assert s.predictive_result()["n_used"] == 0 and np.all(np.isnan(s.predictive_result()["pit"]))
    s.push(P[:4])
    s.push(P[4:])
    assert same_pred(s.predictive_result(), full), "after a reset"
    s.profile(True)                                                          # the two getters: one launch each per block
    s.reset()
    s.push(P)
    ms_f, n_f = s.kernel_time()
    ms_p, n_p = s.predictive_kernel_time()
    s.profile(False)
    assert n_f == 3 and n_p == 3 and ms_f > 0.0 and ms_p > 0.0
    assert same_pred(s.predictive_result(), full), "with the timers on"
    refused(acc.close)                                                       # a live summary holds the context
    s.close()
    acc.close()
