"""Windowed predictive check of a stored chain on the GPU (tamcmc_summary_window_*, include/tamcmc_accel.h;
tamcmc_window.hip): per window of W bins the log predictive CDF and survival function of the window's summed residual
averaged over the chain, the PIT and the mean residual, accumulated beside the fold kernel in the pass the user already
makes.

Reference: tests/window_reference.py, an independent numpy transcription of the definitions in the header, run in long
double (tests/test_summary_window_host.py pins its tails against mpmath at shapes up to 512).

Exact checks (no tolerance): with W = 1 every array and total is the per-bin check's, bit for bit (p a power of two, and
chi_square); every result bit for bit independent of block_chains and of the split into pushes; the fold results and the
per-bin check's bit for bit the same with the windowed check on and off; the windows' results untouched by a quantile pass
and a LOO pass, and the same after a reset and a second pass; n_windows, the partition, ks_D, pit_hist and the two minima
recomputed from the library's own arrays.

Against the reference the rule is that of tests/test_summary_predictive_gpu.py, unchanged.  On the GPU's own model rows
(eval_batch with every chain in model_rows) the bound is, per case and per quantity (the maximum over the windows), 10 x
the larger of
    (a) the reference's own change when every model value is perturbed by 2^-50 relative (one random sign per value), and
    (b) the difference between the reference run in float64 and in long double (both sum one term after the other, so (b)
        carries the n 2^-52 accumulation error of a float64 stream -- the leading term at 70 001 samples -- and, at a
        shape of a few hundred, the cancellation of the three large terms of log Q).
Differences are relative to max(1, |value|) for log_cdf, log_sf and mean_resid and absolute for pit.  On the oracle's rows
(pyoracle.generate_batch(..., want_models=True)) the perturbation is 1e-12 relative, one factor per distinct parameter row
and bin, the maximum over five seeds, and the bound is 10 x that change.
Self-check: exp(log_cdf) + exp(log_sf) = 1 within (n + 2) 2^-52; where the shape p len exceeds 1 and the two tails come
from different branches with an error of up to bound (b), within that bound plus (n + 2) 2^-52 instead.
Every worst ratio is printed before it is asserted (pytest -s).

Worst ratios observed on an MI355X over all cases below: on the GPU's own rows log_cdf 0.36, pit 0.41, log_sf 0.46,
mean_resid 0.49; at shape 512 0.0058, 0.0046, 0.0046 and 0.19; at 70 001 samples 0.0042, 0.0053, 0.00097 and 0.075; on the
oracle's rows 3.1e-4, 3.1e-4, 1.3e-4 and 8.5e-4.  |P + Q - 1| was 8.4e-15 or less.
With tmp_chi_p at every shape -- the first build -- [65-200-p3] at W = 7, first = 0 missed its bound: log_cdf at 1.44 and
pit at 2.07, from the device's log times the shape (tamcmc_window.h, tmw_chi_a); it is at 0.24 and 0.11 now.
"""

import functools

import numpy as np
import pytest

from predictive_reference import predictive_reference
from summary_support import (accepted, c2_case, c2_chain, check_pit, check_tails_reference, collect, data_of, edited, edited_chi, open_case,
                             row_groups, same, same_pred, same_win, sigma_of, spectrum_for, true_model, with_rejected)
from support import bits, pyorc
from tamcmc_amd import capi, synth
from window_reference import partition, window_reference, window_totals

pytestmark = pytest.mark.gpu

KEYS = capi.Summary.WINDOW_ARRAYS
WORST = {}                                                   # tag of the test -> key -> worst ratio seen (printed per case as well)


def check_totals(tag, res, n, n_rejected, Nx, W, first):
    """n_windows and the partition as the header defines them; pit from the smaller tail, within 2 ulp; every total
    recomputed from the library's own arrays: exact."""
    f, begin, end = partition(Nx, W, first)
    assert res["n_used"] == n and res["n_rejected"] == n_rejected, (tag, res["n_used"], res["n_rejected"])
    assert res["n_windows"] == len(begin) == len(res["pit"]) and res["W"] == W and res["first"] == f, tag
    assert np.array_equal(res["first_bin"], begin) and np.array_equal(res["last_bin"], end - 1), tag
    lc, ls, pit = check_pit(tag, res)
    t = window_totals(pit, lc, ls)
    assert res["ks_D"] == t["ks_D"], (tag, res["ks_D"], t["ks_D"])
    assert np.array_equal(res["pit_hist"], t["pit_hist"]) and int(res["pit_hist"].sum()) == pit.size, (tag, res["pit_hist"])
    assert res["win_min_log_sf"] == t["win_min_log_sf"] and res["min_log_sf"] == t["min_log_sf"], tag
    assert res["win_min_log_cdf"] == t["win_min_log_cdf"] and res["min_log_cdf"] == t["min_log_cdf"], tag


def check_reference(tag, res, rows, y, groups, rel, seeds, with_f64, W, first=0, like=0, p=1, sigma=None, n_rejected=0):
    """res against window_reference(rows) with the bounds of the module docstring; then the self-check and the totals.
    Returns the reference."""
    reference = functools.partial(window_reference, W=W, first=first, like=like, p=p, sigma=sigma)
    ref = check_tails_reference(reference, "window", KEYS, tag, res, rows, y, groups, rel, seeds, with_f64, like, p * W, f64_always=True,
                                worst=WORST)
    check_totals(tag, res, len(rows), n_rejected, len(y), W, first)
    return ref


def run(acc, pushes, block=0, window=7, predictive=False):
    """A fold pass with the windowed check on.  Returns (window result, fold result[, predictive result])."""
    with capi.Summary(acc, block, predictive=predictive, window=window) as s:
        for P in pushes:
            s.push(P)
        out = (s.window_result(), s.result())
        return out + (s.predictive_result(),) if predictive else out


def firsts(W):
    return sorted({0, 1, min(3, W), W - 1} - ({W - 1} if W == 1 else set()))


# ---- 1. W = 1 is the per-bin check ----

@pytest.mark.parametrize("Nx", [2, 65, 700])
def test_one_bin_per_window_is_the_per_bin_check(accel_mod, Nx):
    """p = 1, 2, 64 and chi_square, 37 samples two of which are rejected: every array and total of window_result() equals
    predictive_result() of the same object bit for bit.  p = 3, where 3 (y / M) and (3 y) / M round differently: within
    the bound against the reference."""
    w, y0, P35 = c2_chain(Nx, 35)
    P = with_rejected(w, P35, [0, 20])
    for cfg in ("p1", "p2", "p64", "chi-square", "p3"):
        y, like, p, sigma = data_of(w, y0, cfg)
        with open_case(accel_mod, w, y, cfg) as acc:
            rows = accepted(acc, P, 2)
            res, _, pred = run(acc, [P], 8, window=1, predictive=True)
        tag = f"one-bin Nx={Nx} {cfg}"
        assert res["n_windows"] == Nx and res["n_used"] == 35 and res["n_rejected"] == 2, tag
        check_totals(tag, res, 35, 2, Nx, 1, 0)
        if cfg != "p3":
            for k in KEYS:
                assert np.array_equal(bits(res[k]), bits(pred[k])), (tag, k)
            assert np.array_equal(res["pit_hist"], pred["pit_hist"]), tag
            for k in ("ks_D", "min_log_sf", "min_log_cdf"):
                assert np.array_equal(bits(float(res[k])), bits(float(pred[k]))), (tag, k)
            assert res["win_min_log_sf"] == pred["bin_min_log_sf"] and res["win_min_log_cdf"] == pred["bin_min_log_cdf"], tag
        else:
            check_reference(tag, res, rows, y, np.arange(35), 2.0 ** -50, (1,), True, 1, 0, like, p, sigma, n_rejected=2)


# ---- 2. against the reference ----

CASES = [(2, 1), (7, 37), (65, 200), (700, 37), (5000, 37)]


@pytest.mark.parametrize("cfg", ["p1", "p3", "chi-square"])
@pytest.mark.parametrize("Nx,S", CASES)
def test_against_the_reference(accel_mod, Nx, S, cfg):
    """W = 2, 3, 7, 64, 100 and 512 (W > Nx: one window), first = 0, 1, 3 and W - 1, on the GPU's own rows, with rejected
    samples among them.  p = 3 allows W up to 170.  At Nx = 5000, first = 3 (1 where W <= 3) moves every tile edge of the sums
    kernel but the first off the multiples of W (a tile is min(256, 4096 / W) windows), and only W = 100 runs every first."""
    w, y0, P0 = c2_chain(Nx, S)
    n_bad = 0 if S == 1 else 3
    P = with_rejected(w, P0, [0, S // 2, S]) if n_bad else P0
    y, like, p, sigma = data_of(w, y0, cfg)
    misses = []
    with open_case(accel_mod, w, y, cfg) as acc:
        rows = accepted(acc, P, n_bad)
        for W in (2, 3, 7, 64, 100, 512):
            if like == 0 and p * W > 512:
                continue
            for first in (firsts(W) if Nx < 5000 or W == 100 else [3 if W > 3 else 1]):
                res, _ = run(acc, [P], 16, window=(W, first))
                collect(check_reference, misses, f"gpu-rows Nx={Nx} S={S} {cfg} W={W} first={first}", res, rows, y, np.arange(S), 2.0 ** -50, (1,), True,
                        W, first, like, p, sigma, n_rejected=n_bad)
    print("WORST gpu-rows", WORST.get("gpu-rows"))
    assert not misses, misses


@pytest.mark.parametrize("name,p,W", [("p64-W8", 64, 8), ("p1-W512", 1, 512)])
def test_the_largest_shape(accel_mod, name, p, W):
    """Shape 512 exactly, from p = 64 over 8 bins and from p = 1 over 512: 700 and 5000 bins, 37 samples."""
    misses = []
    for Nx in (700, 5000):
        w, y0, P = c2_chain(Nx, 37)
        y = edited_chi(y0)
        with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=float(p)) as acc:
            rows = accepted(acc, P, 0)
            for first in (0, 3):
                res, _ = run(acc, [P], 16, window=(W, first))
                collect(check_reference, misses, f"shape-512 {name} Nx={Nx} first={first}", res, rows, y, np.arange(37), 2.0 ** -50, (1,), True, W, first, 0, p)
    print("WORST shape-512", WORST.get("shape-512"))
    assert not misses, misses


@pytest.mark.parametrize("name", ["c2-700-p1", "c2-129-p3", "c2-129-chi-square"])
def test_against_the_oracle(accel_mod, name):
    like, p, sigma = 0, 1, None
    if name == "c2-700-p1":
        w, y0, P, _, _ = c2_case(700)
    else:
        w, y0, P = c2_chain(129, 70)
        p = 3 if name.endswith("p3") else 1
    if name.endswith("chi-square"):
        like, sigma = 1, sigma_of(129)
        y = edited(y0, 1, true_model(w), sigma)[0]
    else:
        y = edited_chi(y0)
    _, rst, M = pyorc().generate_batch(2, w["plength"], w["x"], y, P, np.ones(len(P)), sigma_y=sigma, likelihood_case=like,
                                       likelihood_p=float(p), want_models=True)
    assert np.all(rst == 0)
    misses = []
    with accel_mod.Accel(2, w["plength"], w["x"], y, sigma_y=sigma, likelihood_case=like, likelihood_p=float(p)) as acc:
        for W, first in ((7, 3), (64, 0), (100, 99)):
            res, _ = run(acc, [P], window=(W, first))
            collect(check_reference, misses, f"oracle {name} W={W} first={first}", res, M, y, row_groups(P), 1e-12, (1, 2, 3, 4, 5), False, W, first, like, p, sigma)
    print("WORST oracle", WORST.get("oracle"))
    assert not misses, misses


# ---- 3. exact independence ----

@pytest.mark.parametrize("cfg", ["p1", "p3", "chi-square"])
def test_block_size_and_push_split_cannot_change_a_bit(accel_mod, cfg):
    """block_chains 1, 3, 64 and the default, and three different splits into pushes: identical bits in every array and
    total; the fold results and the per-bin check's are those of objects without the windowed check."""
    w, y0, P0 = c2_chain(129, 70)
    P = with_rejected(w, P0, [0, 33, 70])
    y = data_of(w, y0, cfg)[0]
    with open_case(accel_mod, w, y, cfg) as acc:
        first, fold, pred = run(acc, [P], 1, window=(7, 3), predictive=True)
        assert first["n_used"] == 70 and first["n_rejected"] == 3
        for B in (3, 64, 0):
            res, f, pr = run(acc, [P], B, window=(7, 3), predictive=True)
            assert same_win(res, first) and same(f, fold) and same_pred(pr, pred), ("block_chains", B)
        for cuts in ((1,), (9, 10), (24, 48, 72)):
            res, f = run(acc, np.split(P, cuts), 7, window=(7, 3))               # (the per-bin check off: the windows keep their bits)
            assert same_win(res, first) and same(f, fold), ("pushes", cuts)
        with capi.Summary(acc, 7) as s:                                          # both checks off
            s.push(P)
            assert same(s.result(), fold), "the fold results differ with the windowed check on"
        with capi.Summary(acc, 7, predictive=True) as s:                         # the per-bin check alone
            s.push(P)
            assert same_pred(s.predictive_result(), pred), "the per-bin check's results differ with the windowed check on"
        with capi.Summary(acc, 7) as s:                                          # enabled in the other order
            s.window_enable(7, 3)
            s.predictive_enable()
            s.push(P)
            assert same_win(s.window_result(), first) and same_pred(s.predictive_result(), pred)


def test_other_modes_and_reset_leave_the_state_alone(accel_mod):
    """A quantile pass and a LOO pass over the same rows on the same object: the windows' results keep their bits and can be
    read inside either mode; the fold goes on afterwards as if nothing had happened; reset keeps the setting and a second
    pass gives the same bits."""
    w, y0, P = c2_chain(129, 70)
    y = edited_chi(y0)
    extra = synth.chain_params(w, 5, seed=4242)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc, 16, window=(20, 11)) as s:
            s.push(P)
            first = s.window_result()
            assert same_win(s.window_result(), first), "a second result"
            s.quantiles_begin((0.16, 0.5, 0.84))
            s.push(P)
            assert same_win(s.window_result(), first), "inside quantile mode, a pass pushed"
            s.quantiles_step()
            s.quantiles_end()
            assert same_win(s.window_result(), first), "after a quantile pass"
            s.loo_begin()
            s.push(P)
            assert same_win(s.window_result(), first), "inside LOO mode, a pass pushed"
            s.loo_result()
            s.loo_end()
            assert same_win(s.window_result(), first), "after a LOO pass"
            s.push(extra)
            after, after_fold = s.window_result(), s.result()
            s.reset()
            r0 = s.window_result()
            assert r0["n_used"] == 0 and r0["n_windows"] == first["n_windows"] and all(np.all(np.isnan(r0[k])) for k in KEYS)
            with pytest.raises(accel_mod.AccelError):
                s.window_enable(20, 11)                                          # the setting is still on
            s.push(P[:33])
            s.push(P[33:])
            assert same_win(s.window_result(), first), "a second pass after a reset"
        both, both_fold = run(acc, [P, extra], 16, window=(20, 11))
        assert same_win(after, both) and same(after_fold, both_fold), "a summary that never entered a mode differs"
        with capi.Summary(acc, 16) as s:                                         # and the modes' results do not depend on the check
            s.push(P)
            loo_off = s.loo(P)
            q_off = s.quantiles(P, (0.16, 0.5, 0.84))
        with capi.Summary(acc, 16, window=(20, 11)) as s:
            s.push(P)
            loo_on = s.loo(P)
            q_on = s.quantiles(P, (0.16, 0.5, 0.84))
        assert all(np.array_equal(bits(np.asarray(loo_on[k], dtype=np.float64)), bits(np.asarray(loo_off[k], dtype=np.float64)))
                   for k in ("elpd_loo", "pareto_k", "cutoff", "elpd_loo_total", "p_loo"))
        assert np.array_equal(bits(q_on["lo"]), bits(q_off["lo"])) and np.array_equal(bits(q_on["hi"]), bits(q_off["hi"]))


# ---- 5. refusals ----

def test_refusals_and_state(accel_mod):
    w, y0, P = c2_chain(65, 9)
    y = edited_chi(y0)
    T = np.ones(len(P))
    E = capi.E_INVALID

    def refused(fn, *a, **k):
        with pytest.raises(accel_mod.AccelError) as e:
            fn(*a, **k)
        assert e.value.code == E

    def works(s, W, first=0):
        """The object is as it was: the enable the refusals left undone goes through, and the check runs."""
        assert s.window_enable(W, first) == len(partition(65, W, first)[1])
        s.push(P)
        r = s.window_result()
        check_totals(f"after a refusal W={W}", r, 9, 0, 65, W, first)

    with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=3.0) as acc:
        with capi.Summary(acc) as s:
            refused(s.window_enable, 0)                                          # W = 0
            refused(s.window_enable, 513)                                        # W = 513
            refused(s.window_enable, -1)
            refused(s.window_enable, 7, 8)                                       # first > W
            refused(s.window_enable, 7, -1)
            refused(s.window_enable, 171)                                        # p W = 513
            refused(s.window_result)                                             # not enabled
            refused(s.window_kernel_time)
            refused(capi.Summary, acc, 0, window=171)
            works(s, 170, 170)                                                   # p W = 510
    for p in (0.0, 0.9, 513.0):                                                  # chi(2,2p) with p < 1, or p alone past the shape
        with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=p) as acc:
            with capi.Summary(acc) as s:
                refused(s.window_enable, 1)
    with accel_mod.Accel(2, w["plength"], w["x"], y, sigma_y=sigma_of(65), likelihood_case=1, likelihood_p=0.0) as acc:
        with capi.Summary(acc, window=512) as s:                                 # chi_square does not look at p
            s.push(P)
            assert s.window_result()["n_used"] == 9 and s.window_result()["n_windows"] == 1
    acc = accel_mod.Accel(2, w["plength"], w["x"], y)
    s = capi.Summary(acc, 4)
    s.push(P[:3])
    refused(s.window_enable, 7)                                                  # after a push
    s.quantiles_begin((0.5,))
    refused(s.window_enable, 7)                                                  # in quantile mode
    s.quantiles_end()
    s.loo_begin()
    refused(s.window_enable, 7)                                                  # in LOO mode
    s.reset()
    acc.begin(P, T)                                                              # a batch in flight
    refused(s.window_enable, 7)
    acc.end()
    acc.arm(len(P))                                                              # a batch armed
    refused(s.window_enable, 7)
    acc.disarm()
    assert s.window_enable(7, 3) == 10                                           # after a reset: allowed
    refused(s.window_enable, 7, 3)                                               # twice
    refused(s.window_enable, 8)
    r0 = s.window_result()                                                       # n = 0: everything is NaN
    assert r0["n_used"] == 0 and r0["n_rejected"] == 0 and r0["n_windows"] == 10 and all(np.all(np.isnan(r0[k])) for k in KEYS)
    assert np.isnan(r0["ks_D"]) and np.isnan(r0["min_log_sf"]) and np.isnan(r0["min_log_cdf"])
    assert r0["win_min_log_sf"] == -1 and r0["win_min_log_cdf"] == -1 and not r0["pit_hist"].any()
    s.push(P)
    full = s.window_result()
    check_totals("refusals", full, 9, 0, 65, 7, 3)
    acc.begin(P, T)
    refused(s.window_result)
    acc.end()
    s.profile(True)                                                              # the getters: one event pair each per block
    s.reset()
    s.push(P)
    ms_f, n_f = s.kernel_time()
    ms_w, n_w = s.window_kernel_time()
    s.profile(False)
    assert n_f == 3 and n_w == 3 and ms_f > 0.0 and ms_w > 0.0
    assert same_win(s.window_result(), full), "with the timers on"
    refused(acc.close)                                                           # a live summary holds the context
    s.close()
    acc.close()


# ---- 6. what the check is for ----

PLANTED = dict(seed=0, window=17)


def test_a_broad_excess_no_single_bin_shows(accel_mod):
    """700 bins of y = M e with exponential e, M the model at the generating parameters; in window 17 of 35 (bins 340 ... 359)
    y = 2 M instead: log Q(20, 40) = -8.6 for the window, -2 in each of its bins.  100 samples narrowly scattered about those
    parameters.  On the reference alone: the planted window has the smallest log_sf of all windows, and the bin with the
    smallest per-bin log_sf lies outside it.  Then the library names the same window and the same bin."""
    w = synth.workload_c2(Nx=700)
    M0 = true_model(w)
    y = M0 * np.random.default_rng(PLANTED["seed"]).exponential(size=700)
    k = PLANTED["window"]
    y[20 * k:20 * (k + 1)] = 2.0 * M0[20 * k:20 * (k + 1)]
    P = synth.chain_params(w, 100, scale=0.05)
    _, rst, M = pyorc().generate_batch(2, w["plength"], w["x"], y, P, np.ones(100), want_models=True)
    assert np.all(rst == 0)
    ref_w, ref_b = window_reference(M, y, 20), predictive_reference(M, y)
    order = np.sort(ref_w["log_sf"])
    worst_bin = int(np.argmin(ref_b["log_sf"]))
    print(f"PLANTED window log_sf {float(ref_w['log_sf'][k]):.4g}, the next window {float(order[1]):.4g}; in its bins "
          f"{float(ref_b['log_sf'][20 * k:20 * (k + 1)].min()):.4g} ... {float(ref_b['log_sf'][20 * k:20 * (k + 1)].max()):.4g}; "
          f"the smallest per-bin log_sf {float(ref_b['log_sf'][worst_bin]):.4g} in bin {worst_bin}")
    assert int(np.argmin(ref_w["log_sf"])) == k and not 20 * k <= worst_bin < 20 * (k + 1), "set-up error: choose another seed"
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        res, _, pred = run(acc, [P], window=20, predictive=True)
    assert res["n_windows"] == 35 and res["win_min_log_sf"] == k and pred["bin_min_log_sf"] == worst_bin
    assert abs(res["min_log_sf"] - float(ref_w["log_sf"][k])) < 1e-9 * abs(res["min_log_sf"])


# ---- 7. a long chain ----

def test_at_length(accel_mod):
    """70 001 samples of a 65-bin grid, W = 7, first = 3, in blocks of 64 and in one block of 70 001: the same bits, and the
    n 2^-52 accumulation of the two running sums within the bound."""
    S = 70001
    w = synth.workload_c2(Nx=65)
    y = edited_chi(spectrum_for(w))
    P = synth.chain_params(w, S)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        rows = accepted(acc, P, 0)
        res, fold = run(acc, [P], 64, window=(7, 3))
        one, fold1 = run(acc, [P], S, window=(7, 3))
    assert same_win(one, res) and same(fold1, fold)
    check_reference("at-length", res, rows, y, np.arange(S), 2.0 ** -50, (1,), True, 7, 3)
