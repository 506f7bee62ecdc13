"""Posterior summaries of a stored chain on long grids (tamcmc_summary_*, include/tamcmc_accel.h): every rule of the summary
object that depends on the length of the grid, on both sides of its edge.  The other summary suites stop at 5000 bins.

  default block   block_chains = 0 is min(64, 64 MiB / (8 Nx)), at least 1 (tms_default_block, tamcmc_summary_walk.h):
                  64 at GA = 131 072 bins, 63 at GB = 131 073, 2 at GC = 4 194 304, 1 at GD = 4 194 305
  scan chunk      min(B, 4096, 256 MiB / (24 total)) samples (tmsc_chunk, tamcmc_scan.h): with the eight widths WIDTHS8 on GB the
                  memory term is 10 -- a block of 63 is six chunks of 10 and one of 3 --, with one width on GD it is 2, with three
                  widths on GD it is 0 and the chunk 1; at 700 bins and a block of 2600 it is 2443, the smallest shape that has it
  LOO tail        M = ceil(min(n / 5, 3 sqrt n)) candidates sorted in LDS arrays of 2048: 1024 at n = 116 508 (P = 1024), 1025 at
                  116 509 and 116 510 (P = 2048); 2048 at 466 033 fills the arrays (passed, not kept: OBSERVED), 466 034 is refused
  tiles, groups   GB is one bin past 512 fold workgroups, 64 scan tiles and 2048 lag groups
  LOO, LOO-PIT    the LOO tail and LOO-PIT kernels give a bin to a thread, the finalize and prepare kernels a workgroup to a bin
                  (4.2e6 workgroups on GC / GD); fold, LOO and PIT pass in the default blocks of 63 (GB), 2 (GC) and 1 (GD)
                  against 7, 3 and 3; M = 14 with the 70 samples of GB, 1 with the 5 of GC / GD (no Pareto fit: k-hat = +inf)
  window-LOO      scratch [block_chains][n_windows], sized at wloo_begin; a sums tile holds min(256, 4096 / W) windows: on GB
                  W = 20 is 6554 windows in 33 tiles, W = 512 257 in 33; on GD W = 1 is 4 194 305 windows, 16 385 tiles a sample
                  and 65 537 workgroups of the tail and PIT kernels; W = 7 with first = 3, 20 and 512 on both grids

Chains: id 2 on the C2 star's grid (c2_chain); 70 accepted samples on GA / GB with a rejected row at pushes 5 and 63 -- inside
the first block, and the last row of a block of 64 / the first of the second block of 63 --, 5 accepted and one rejected on
GC / GD.  The reference rows are the GPU's own (gpu_rows): the model-row launch is pinned against the oracle at these lengths
by tests/test_long_grids_gpu.py.

No tolerance is new.  Exact, on every bin, window and position: block_chains cannot change a bit (default against 7, 64, 3);
min_M / max_M; the quantile brackets and their end (np.sort in float64); W = 1 windows are the per-bin check; a scan position
is the disjoint window that starts there; a list of widths is each width alone; the band-ESS counts and finish; the ESS
finish on the library's own lag products; every total recomputed from the library's own arrays.  The fold's long-double
reduction (accumulation_reference: bound b of tests/test_summary_large_gpu.py) runs on all bins.  The heavier long-double
references -- predictive_reference, window_reference on the windows that hold them, scan_reference at those positions and at
the last position of every width, the ESS lag products -- run on the bins of subset_bins(): the grid's ends, T - 1, T, T + 1
and the two sides of the last full group of T for T = 64, 256, 2048, 4096, the scan-tile edges 2047 + 2048 k +- 1 for k = 31,
32, 62, 63 where the halo of W = 512 crosses a tile, and 512 bins drawn by default_rng(20262); bounds: check_tails_reference
(rel 2^-50, seed 1, with float64), check_acov, check_loo_reference, as the per-mode suites call them.  scan_reference forms the
sums of every position of the grid it is given (W passes over the grid), so at scattered positions the same ascending sums
are formed from the gathered bins (scan_reference_at) and pinned bit for bit to scan_reference(positions=...) on the first
3000 bins.  bandess_reference.counts works in Python integers; at 8 x 131 073 series the same formula runs in int64 (exact:
every term is below 70^3) and is pinned to counts() on the subset.  The LOO cutoff is compared as test_at_length of
tests/test_summary_loo_gpu.py compares it -- within 4 ulp of the float64 order statistic, the device's log being within an ulp
of numpy's -- because the library's own l would take one push per sample; tail_len is exact.

Bound b and lppd.  delta = dl + n 2^-52 max|l| bounds the error of lppd only while n 2^-52 max|l| is the larger part of it: at
70 001 samples it is, at the 5 samples of GC / GD and |l| < 0.1 it is not, and there a plain float64 evaluation of the header's
own recurrence with numpy's exp and log -- no device involved -- exceeds delta by a factor 1.95 in 13 of 4 194 304 bins; the
library by 1.68.  What delta leaves out is the rounding of the log-sum-exp itself, which does not shrink with |l|: r is
formed in n - 1 steps of the running-maximum recurrence (tamcmc_summary.hip), each with a device exp of 1 ulp on a term of
at most r (2^-52 relative to r), a product (2^-53, the rescaling branch) and a sum (2^-53), so r has a relative error of up
to (n - 1) 2^-51; r / n adds 2^-53; all of it goes into log(r / n) as an absolute error; the device log adds 2^-52 |log(r / n)|
<= 2^-52 log n, since 1 <= r <= n; the sum a + log(r / n) adds 2^-53 |lppd|.  log_sum_exp_term() is that sum, (4 n - 3) 2^-53 +
2^-52 log n + 2^-53 |lppd|, added to delta for lppd alone; the ratio to delta as it stands is printed beside it.  Bound b of
tests/test_summary_large_gpu.py is unchanged.

The launch splits `per` of tm_launch_window and tm_launch_scan (2^23 workgroups, 2^30 / 2^31 threads a launch) are not reached
here or anywhere: with the block and chunk rules as they are a launch that large needs tens of GB of model rows.  Nor, in
LOO and window-LOO mode: heap and log-weight offsets past 2^31 elements, which need M Nx > 2^31 -- M = 512 on GD, for example,
is 29 128 samples in blocks of one row and 17 GB each for the heap and the log weights (the code casts every such offset to
size_t) --; and the launch split `per` of wloo_launch_sums (2^23 workgroups, 2^31 threads), reached only with far more samples
in a block than the block rule allows on a grid with that many windows.

In LOO and window-LOO mode on GB and GD (tests of section 7) cutoff and tail_len are exact on every bin and window against the
library's own l (summary_support.library_l: one push per sample, affordable at 70 and at 5 samples; for a window the float64
sum of its bins' l in ascending order, wloo_support.exact_windows); the references -- check_loo_reference, the LOO-PIT suite's
and the window-LOO suite's check_reference (loopit_support, wloo_support), the latter on the gathered grid of the windows that
hold the subset with the first and the last window -- run on subset_bins().

Worst ratios to the bounds, memory and times observed on an MI355X (pytest -s prints them): see OBSERVED below.
"""
import functools
import time

import numpy as np
import pytest

import bandess_reference as B
import loopit_support as LP
import wloo_support as WL
from predictive_reference import _log_mean_exp, _seq_sum, log_gamma_tails, predictive_reference, totals_from_pit
from scan_reference import scan_reference, scan_totals
from summary_support import (ESS_WORST, LD, Q8, accepted, accumulation_reference, band_pass, c2_chain, check, check_acov, check_finish,
                             check_loo_reference, check_pit, check_tails_reference, exact_structure, gpu_rows, library_l, ranks_of, rows_around,
                             run_ess, same, same_pred, same_scan, same_scans, same_traj, same_win, select, spectrum_for, steps, summarize, tail_M,
                             truth_of, unresolved_bits, with_rejected, x_of)
from support import bits
from tamcmc_amd import capi, synth
from window_reference import partition, window_reference, window_totals, windows_holding

pytestmark = pytest.mark.gpu

OBSERVED = """
Worst ratios to the bounds (22 cases, 982 GPU tests in the session):
  fold, bound b with the log-sum-exp term   mean_M 0.24, mean_l 0.18, lppd 0.13, var_M 5.4e-3, var_l 0.15, totals 1.8e-2 (all at
                                            4.2e6 bins, 5 samples; at 131 073 bins, 70 samples: 0.072, 0.074, 0.028, 5.4e-4, 0.024, 8.7e-4)
  lppd to bound b as it stands              0.49 at 131 072 / 131 073 bins, 1.68 at 4 194 304 / 4 194 305 (module docstring)
  per-bin check                             pit 0.039, log_cdf 0.038, log_sf 0.040, mean_resid 0.10
  windows (W = 7 first = 3, W = 512)        pit 0.030, log_cdf 0.057, log_sf 0.039, mean_resid 0.10; at W = 512 1.9e-4 and under but mean_resid
  scan (eight widths on GB, three on GD)    pit 0.039, log_cdf 0.050, log_sf 0.040, mean_resid 0.16
  ESS lag products                          acov_M 0.020, acov_l 0.088; finish 0 ulp, R-hat 2.1e-14 relative
  band ESS                                  counts and E_k exact, tau and ess 0 ulp
  LOO, n = 116 508 / 116 509 / 116 510      elpd_loo 0.10, k-hat 0.013; n = 466 033: 0.10 and 0.010
  |P + Q - 1|                               1.8e-14 or less
  LOO on GB / GD (subset_bins)              elpd_loo 0.083 / 0.047, k-hat 0.0097 / 0 (every k-hat +inf with 5 samples, in the reference too)
  LOO-PIT on GB / GD                        loo_log_cdf 0.073 / 0.075, loo_log_sf 0.080 / 0.044, loo_pit 0.076 / 0.058, is_ess 0.067 / 0.029, log_wsum
                                            0.0084 / 0.0043, elpd_loo against the reference's weights 0.055 / 0.028
  window-LOO, W = 1, 7, 20, 512 on GB, GD   elpd_lwo 0.1, k-hat 0.1, cutoff 0.1, loo_log_cdf 0.075, loo_log_sf 0.080, loo_pit 0.076, is_ess 0.1, log_wsum 0.1
                                            (0.1, all at W = 512: the result equals the float64 reference, whose distance from the long-double
                                            one is the bound's tenth; below W = 512 0.099 for elpd_lwo at W = 1 on GB and 0.077 and under otherwise)
Device memory: the largest case is the scan of (7, 20, 40) on GD, about 1.5 GB (state 805 MB, scratch 302 MB, the fold's and the
rows').  Slowest case: test_scan_on_the_longest_grid, 6.1 s (5.7 s on the device side); the 4.2e6-bin fold and window cases
take 5.6 ... 5.7 s, most of it the long-double reduction of all bins on the host.
LOO at n = 466 033 (M = 2048): 8.8 s, of which the fold and the LOO pass take 0.69 s; the slowest case of
tests/test_summary_large_gpu.py took 3.6 s in the same session.  The project has no marker for slow cases, so that case is not
kept; the refusal at 466 034, which needs the fold pass alone, takes 0.7 s.
LOO, LOO-PIT and window-LOO (11 cases): the largest is window-LOO with W = 1 on GD and block_chains = 3, about 1.5 GB: 264 bytes a
window for the mode and its sub-mode (heap, state and scratch 386 MB, log weights, state and scratch 721 MB: tamcmc_wloo.h) beside
the fold's state and the rows'; the per-bin LOO-PIT state on GD is about 0.5 GB.  Slowest: test_loo_and_loo_pit on GD, 5.1 s (3.4 s
on the device side, one push per sample for the library's own l among it), on GC 3.9 s, test_window_loo with W = 1 on GD 3.6 s; every
other case 1.9 s or less.
"""

GA, GB, GC, GD = 131072, 131073, 4194304, 4194305
WIDTHS8 = (1, 10, 20, 40, 64, 128, 256, 512)
MAX_LAG = 69
WORST = {}


# ---- the three rules, restated from their headers ----

def default_block(Nx):
    """tms_default_block (tamcmc_summary_walk.h): 64, lowered so that a block's rows take at most 64 MiB."""
    return max(1, min(64, (64 << 20) // (8 * Nx)))


def scan_total(Nx, widths):
    return sum(Nx - W + 1 for W in widths)


def scan_fit(total):
    """The memory term of tmsc_chunk (tamcmc_scan.h): 256 MiB of scratch at 24 bytes per (sample, width, position)."""
    return (256 << 20) // (24 * total)


def scan_chunk(block, total):
    return max(1, min(block, 4096, scan_fit(total)))


# ---- cases ----

@functools.lru_cache(maxsize=None)
def chain(Nx):
    """(workload, spectrum, pushed rows, number of rejected rows among them), computed once and never changed."""
    long = Nx >= GC
    w, y, P0 = c2_chain(Nx, 5 if long else 70)
    at = [2] if long else [5, 62]                           # pushes 2; 5 and 63
    P = with_rejected(w, P0, at)
    P.setflags(write=False)
    return w, y, P, len(at)


_ROWS = {}


def rows_of(acc, Nx):
    """The GPU's own rows of the accepted samples; computed once per grid."""
    if Nx not in _ROWS:
        _, _, P, n_bad = chain(Nx)
        _ROWS[Nx] = accepted(acc, P, n_bad)
        _ROWS[Nx].setflags(write=False)
        assert np.all(_ROWS[Nx] > 0)
    return _ROWS[Nx]


def open_grid(accel_mod, Nx):
    w, y, _, _ = chain(Nx)
    return accel_mod.Accel(2, w["plength"], w["x"], y)


@functools.lru_cache(maxsize=None)
def subset_bins(Nx, drawn=512):
    """The bins at which the heavier references are evaluated (module docstring), ascending; `drawn` of them are drawn."""
    b = {0, 1, Nx - 2, Nx - 1}
    for T in (64, 256, 2048, 4096):
        full = (Nx // T) * T                                 # the first bin behind the last full group of T
        b.update((T - 1, T, T + 1, full - 1, full))
    for k in (31, 32, 62, 63):
        b.update((2047 + 2048 * k - 1, 2047 + 2048 * k, 2047 + 2048 * k + 1))
    b.update(int(v) for v in np.random.default_rng(20262).integers(0, Nx, size=drawn))
    out = np.array(sorted(v for v in b if 0 <= v < Nx), dtype=np.int64)
    out.setflags(write=False)
    return out


def record(tag, ratios):
    seen = WORST.setdefault(tag, {})
    for k, v in ratios.items():
        seen[k] = max(seen.get(k, 0.0), v)


# ---- 1. the fold ----

def log_sum_exp_term(n, lppd):
    """What bound b leaves out of lppd (module docstring): the roundings of r and of a + log(r / n) themselves."""
    return (4 * n - 3) * 2.0 ** -53 + 2.0 ** -52 * np.log(float(n)) + 2.0 ** -53 * np.abs(lppd)


@pytest.mark.parametrize("Nx", [GA, GB, GC, GD])
def test_fold_default_block(accel_mod, Nx):
    """The default block -- 64, 63, 2 and 1 samples, counted off the fold launches of a push of 64 (GA, GB) or 6 rows -- gives
    the bits of block_chains = 7; min_M / max_M are the rows' own; the long-double reduction of all bins within bound b."""
    w, y, P, n_bad = chain(Nx)
    Bd = default_block(Nx)
    assert Bd == {GA: 64, GB: 63, GC: 2, GD: 1}[Nx]
    t0 = time.perf_counter()
    with open_grid(accel_mod, Nx) as acc:
        rows = rows_of(acc, Nx)
        res, logL, st = summarize(acc, [P])
        res7, logL7, st7 = summarize(acc, [P], 7)
        with capi.Summary(acc) as s:
            s.profile(True)
            head = P[:64]
            s.push(head)
            launches = s.kernel_time()[1]
            s.profile(False)
    print(f"TIME fold Nx={Nx}: {time.perf_counter() - t0:.2f} s on the device side")
    assert launches == -(-len(head) // Bd), ("fold launches of one push", launches, len(head), Bd)
    assert res["n_used"] == len(rows) and res["n_rejected"] == n_bad and int((st != 0).sum()) == n_bad
    assert same(res, res7), "the default block and block_chains = 7 differ"
    assert np.array_equal(bits(logL), bits(logL7)) and np.array_equal(st, st7)
    assert np.array_equal(bits(res["min_M"]), bits(rows.min(axis=0))) and np.array_equal(bits(res["max_M"]), bits(rows.max(axis=0)))
    ref, bound = accumulation_reference(rows, y, None, 0)
    ref["n_rejected"] = n_bad
    stated = float(np.max(np.abs(res["lppd"].astype(LD) - ref["lppd"]) / bound["lppd"]))
    print(f"RATIO long-grid fold Nx={Nx} lppd to bound b without the log-sum-exp term: {stated:.3g}")
    record("fold-lppd-without-the-log-sum-exp-term", dict(lppd=stated))
    bound["lppd"] = bound["lppd"] + log_sum_exp_term(len(rows), ref["lppd"])
    record("fold", check(f"long-grid fold Nx={Nx} accumulation alone", res, ref, bound))


# ---- 2. quantiles ----

def test_quantiles(accel_mod):
    """Q8 on GB at 6 bits a pass to the end and at 1 bit for six passes: the bracket holds the truth after every pass, ends on
    it in every bin, and narrows the same with the default block (63) and with block_chains = 7."""
    _, _, P, _ = chain(GB)
    with open_grid(accel_mod, GB) as acc:
        rows = rows_of(acc, GB)
        truth = truth_of(rows, Q8)
        u0 = unresolved_bits(rows)
        out = {}
        for block in (0, 7):
            with capi.Summary(acc, block) as s:
                s.push(P)
                traj, ranks = select(s, Q8, 6, lambda k: s.push(P), truth=truth, u0=u0)
            assert np.array_equal(ranks, ranks_of(Q8, len(rows))) and len(traj) - 1 == -(-u0 // 6)
            assert np.array_equal(bits(traj[-1][0]), bits(truth)) and np.array_equal(bits(traj[-1][1]), bits(truth)), block
            with capi.Summary(acc, block) as s:
                s.push(P)
                out[block] = (traj, steps(s, Q8, 1, lambda k: s.push(P), truth, 6))
    assert same_traj(out[0][0], out[7][0]) and same_traj(out[0][1], out[7][1]), "block_chains = 7 narrows differently"


# ---- 3. the per-bin and the windowed check ----

def window_totals_exact(tag, res, n, n_bad, Nx, W, first):
    """check_totals of tests/test_summary_window_gpu.py: the partition and every total from the library's own arrays."""
    f, begin, end = partition(Nx, W, first)
    assert res["n_used"] == n and res["n_rejected"] == n_bad and res["n_windows"] == len(begin) == len(res["pit"]) and res["first"] == f, tag
    assert np.array_equal(res["first_bin"], begin) and np.array_equal(res["last_bin"], end - 1), tag
    lc, ls, pit = check_pit(tag, res)
    t = window_totals(pit, lc, ls)
    assert res["ks_D"] == t["ks_D"] and np.array_equal(res["pit_hist"], t["pit_hist"]), tag
    assert all(res[k] == t[k] for k in ("win_min_log_sf", "min_log_sf", "win_min_log_cdf", "min_log_cdf")), tag


@pytest.mark.parametrize("Nx", [GB, GD])
def test_windows_and_the_per_bin_check(accel_mod, Nx):
    """W = 1 is the per-bin check in every bin; W = 7 with first = 3 and W = 512 against the reference on the windows that
    hold the subset, the per-bin check on the subset itself; the default block against block_chains = 7 (3 on GD)."""
    _, y, P, n_bad = chain(Nx)
    sub = subset_bins(Nx)
    other = 7 if Nx == GB else 3
    t0 = time.perf_counter()
    with open_grid(accel_mod, Nx) as acc:
        rows = rows_of(acc, Nx)
        n = len(rows)
        out = {}
        for window in (1, (7, 3), 512):
            for block in (0, other):
                with capi.Summary(acc, block, predictive=True, window=window) as s:
                    s.push(P)
                    out[window, block] = (s.window_result(), s.predictive_result(), s.result())
            assert same_win(out[window, 0][0], out[window, other][0]) and same_pred(out[window, 0][1], out[window, other][1]) and \
                same(out[window, 0][2], out[window, other][2]), ("block_chains", window)
    print(f"TIME windows Nx={Nx}: {time.perf_counter() - t0:.2f} s on the device side")
    win1, pred, _ = out[1, 0]
    assert win1["n_windows"] == Nx
    for k in capi.Summary.WINDOW_ARRAYS:
        assert np.array_equal(bits(win1[k]), bits(pred[k])), ("W = 1 against the per-bin check", k)
    assert np.array_equal(win1["pit_hist"], pred["pit_hist"])
    for k in ("ks_D", "min_log_sf", "min_log_cdf"):
        assert np.array_equal(bits(float(win1[k])), bits(float(pred[k]))), k
    assert win1["win_min_log_sf"] == pred["bin_min_log_sf"] and win1["win_min_log_cdf"] == pred["bin_min_log_cdf"]
    window_totals_exact(f"Nx={Nx} W=1", win1, n, n_bad, Nx, 1, 0)
    D, hist = totals_from_pit(pred["pit"])
    assert pred["ks_D"] == D and np.array_equal(pred["pit_hist"], hist) and pred["n_used"] == n and pred["n_rejected"] == n_bad
    groups = np.arange(n)
    check_tails_reference(predictive_reference, "predictive", capi.Summary.PREDICTIVE_ARRAYS, f"long-predictive Nx={Nx}", pred, rows[:, sub], y[sub],
                          groups, 2.0 ** -50, (1,), True, 0, 1, f64_always=False, positions=sub, worst=WORST)
    for W, first in ((7, 3), (512, 0)):
        res = out[(W, first) if first else W, 0][0]
        window_totals_exact(f"Nx={Nx} W={W}", res, n, n_bad, Nx, W, first)
        sel, cols, f = windows_holding(sub, Nx, W, first)
        reference = functools.partial(window_reference, W=W, first=f)
        check_tails_reference(reference, "window", capi.Summary.WINDOW_ARRAYS, f"long-window Nx={Nx} W={W} first={first}", res, rows[:, cols], y[cols],
                              groups, 2.0 ** -50, (1,), True, 0, W, f64_always=True, positions=sel, worst=WORST)


# ---- 4. the scan ----

def scan_reference_at(rows, y, W, positions, dtype=LD):
    """scan_reference(rows, y, W, positions=positions) of tests/scan_reference.py, chi(2,2p) with p = 1, from the bins of those
    positions alone: the same ascending sums, one term after the other from bin j, and the same tails."""
    J = np.asarray(positions, dtype=np.int64)
    q = np.asarray(y).astype(dtype) / np.asarray(rows).astype(dtype)
    S = q[:, J].copy()
    for i in range(1, W):
        S = S + q[:, J + i]
    logP, logQ = log_gamma_tails(int(W), dtype(1) * S, dtype)
    lc, ls = _log_mean_exp(logP), _log_mean_exp(logQ)
    pit = np.where(lc < ls, np.exp(lc), -np.expm1(ls))
    return dict(log_cdf=lc, log_sf=ls, mean_resid=_seq_sum(S / dtype(int(W))) / dtype(S.shape[0]), pit=pit)


def run_scan(acc, P, block, widths):
    with capi.Summary(acc, block, scan=widths) as s:
        s.push(P)
        return [s.scan_result(k) for k in range(len(widths))], s.result()


def run_window(acc, P, block, W, first):
    with capi.Summary(acc, block, window=(W, first)) as s:
        s.push(P)
        return s.window_result()


def scan_is_the_windows(tag, acc, P, block, res, W, firsts):
    """Every full window of window=(W, first) equals the scan position at its first bin, bit for bit.  Returns the positions."""
    seen = []
    for first in firsts:
        win = run_window(acc, P, block, W, first)
        full = np.flatnonzero(win["last_bin"] - win["first_bin"] + 1 == W)
        at = win["first_bin"][full]
        for k in capi.Summary.SCAN_ARRAYS:
            assert np.array_equal(bits(np.asarray(res[k])[at]), bits(np.asarray(win[k])[full])), (tag, W, first, k)
        assert win["n_used"] == res["n_used"] and win["n_rejected"] == res["n_rejected"], (tag, W, first)
        seen.append(at)
    return np.unique(np.concatenate(seen))


def scan_totals_exact(tag, res, n, n_bad, Nx, W):
    n_pos = Nx - W + 1
    assert res["n_used"] == n and res["n_rejected"] == n_bad and res["W"] == W and res["n_positions"] == n_pos == len(res["pit"]), tag
    assert np.array_equal(res["first_bin"], np.arange(n_pos)) and np.array_equal(res["last_bin"], np.arange(n_pos) + W - 1), tag
    lc, ls, _ = check_pit(tag, res)
    t = scan_totals(lc, ls)
    assert all(res[k] == t[k] for k in ("min_log_sf", "min_log_cdf", "pos_min_log_sf", "pos_min_log_cdf")), tag


def scan_against_the_reference(tag, res, rows, y, W, bins):
    """The positions `bins` that the width has, and its last one: check_tails_reference on the bins those windows hold."""
    Nx = len(y)
    pos = np.unique(np.concatenate([bins[bins <= Nx - W], [Nx - W]]))
    cols = np.unique((pos[:, None] + np.arange(W)[None, :]).ravel())         # a window's bins stay neighbours in `cols`
    reference = functools.partial(scan_reference_at, W=W, positions=np.searchsorted(cols, pos))
    check_tails_reference(reference, "scan", capi.Summary.SCAN_ARRAYS, tag, res, rows[:, cols], y[cols], np.arange(len(rows)), 2.0 ** -50, (1,), True,
                          0, W, f64_always=True, positions=pos, worst=WORST)


def test_scan_reference_at_is_scan_reference(accel_mod):
    """The gathered form of the reference is the reference: the first 3000 bins of GB, W = 7 and 512, both precisions."""
    _, y, _, _ = chain(GB)
    with open_grid(accel_mod, GB) as acc:
        rows = rows_of(acc, GB)[:, :3000]
    for W in (7, 512):
        pos = np.array([0, 1, 2, 700, 2047, 2048, 3000 - W])
        for dtype in (LD, np.float64):
            a, b = scan_reference(rows, y[:3000], W, dtype=dtype, positions=pos), scan_reference_at(rows, y[:3000], W, pos, dtype)
            assert all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a), (W, dtype)


def test_scan_chunks_set_by_memory(accel_mod):
    """WIDTHS8 on GB: 1 047 561 positions, so the memory term is 10 and a block of 63 (the default) or 64 is worked in chunks
    of 10 -- earlier chunks of the block before all but the first; block_chains = 7 is one chunk a block.  The same bits from
    all three; every total from the library's own arrays; the reference at the subset and at the last position."""
    _, y, P, n_bad = chain(GB)
    total = scan_total(GB, WIDTHS8)
    assert default_block(GB) == 63 and scan_fit(total) == 10 and scan_chunk(63, total) == 10 and scan_chunk(64, total) == 10 and scan_chunk(7, total) == 7
    sub = subset_bins(GB)
    t0 = time.perf_counter()
    with open_grid(accel_mod, GB) as acc:
        rows = rows_of(acc, GB)
        res, fold = run_scan(acc, P, 0, WIDTHS8)
        for block in (64, 7):
            other, fold_b = run_scan(acc, P, block, WIDTHS8)
            assert same_scans(other, res) and same(fold_b, fold), ("block_chains", block)
    print(f"TIME scan GB eight widths: {time.perf_counter() - t0:.2f} s on the device side")
    n = len(rows)
    for k, W in enumerate(WIDTHS8):
        scan_totals_exact(f"GB W={W}", res[k], n, n_bad, GB, W)
        scan_against_the_reference(f"long-scan GB W={W}", res[k], rows, y, W, sub)


def test_scan_width_7_is_the_windows_at_every_position(accel_mod):
    """Width 7 on GB against the disjoint check through all seven `first`: every position, no tolerance; alone and as a
    member of a memory-bound list it has the same bits."""
    _, _, P, _ = chain(GB)
    with open_grid(accel_mod, GB) as acc:
        (res,), _ = run_scan(acc, P, 0, (7,))
        seen = scan_is_the_windows("GB", acc, P, 0, res, 7, range(1, 8))
        assert np.array_equal(seen, np.arange(GB - 6))
        listed, _ = run_scan(acc, P, 0, (7,) + WIDTHS8[1:])
        assert scan_chunk(63, scan_total(GB, (7,) + WIDTHS8[1:])) == 10 and same_scan(listed[0], res)


def test_scan_on_the_longest_grid(accel_mod):
    """GD.  One width 7: the memory term is 2, so block_chains = 7 is worked in chunks of 2 and the default block of 1 in
    chunks of 1: the same bits, equal to the windows of first = 3 and 7, and to the reference at the subset.  Widths (7, 20,
    40): 12 582 851 positions, past 256 MiB / 24, so the memory term is 0 and the chunk 1 whatever the block: the default block
    and block_chains = 3 (three chunks a block) give the same bits, and each width those of its run alone."""
    _, y, P, n_bad = chain(GD)
    t1, t3 = scan_total(GD, (7,)), scan_total(GD, (7, 20, 40))
    assert default_block(GD) == 1 and scan_fit(t1) == 2 and scan_chunk(7, t1) == 2 and scan_chunk(1, t1) == 1
    assert t3 > 11184810 and scan_fit(t3) == 0 and scan_chunk(3, t3) == 1
    sub = subset_bins(GD)
    t0 = time.perf_counter()
    with open_grid(accel_mod, GD) as acc:
        rows = rows_of(acc, GD)
        (res,), fold = run_scan(acc, P, 0, (7,))
        (res_b7,), fold_b7 = run_scan(acc, P, 7, (7,))
        assert same_scan(res_b7, res) and same(fold_b7, fold), "chunks of 2 in a block of 7"
        seen = scan_is_the_windows("GD", acc, P, 0, res, 7, (3, 7))
        assert len(seen) == (GD - 3) // 7 + GD // 7            # the full windows of first = 3, and of first = 7 with window 0
        three, fold3 = run_scan(acc, P, 0, (7, 20, 40))
        three_b3, fold3_b3 = run_scan(acc, P, 3, (7, 20, 40))
        assert same_scans(three_b3, three) and same(fold3_b3, fold3) and same(fold3, fold), "chunks of 1 in a block of 3"
        assert same_scan(three[0], res), "width 7 alone"
        for k, W in ((1, 20), (2, 40)):
            (alone,), _ = run_scan(acc, P, 3, (W,))
            assert same_scan(alone, three[k]), ("alone", W)
    print(f"TIME scan GD: {time.perf_counter() - t0:.2f} s on the device side")
    n = len(rows)
    for k, W in enumerate((7, 20, 40)):
        scan_totals_exact(f"GD W={W}", three[k], n, n_bad, GD, W)
        scan_against_the_reference(f"long-scan GD W={W}", three[k], rows, y, W, sub)


def test_scan_chunk_set_by_memory_at_its_smallest_shape(accel_mod):
    """700 bins, WIDTHS8: 4577 positions, a memory term of 2443 samples -- below the cap of 4096.  2600 samples in one block are
    a chunk of 2443 and one of 157; rejected rows sit on both sides of that edge and at both ends.  The same bits as from
    blocks of 64."""
    Nx, S = 700, 2600
    w, y, P0 = c2_chain(Nx, S - 4)
    fit = scan_fit(scan_total(Nx, WIDTHS8))
    assert 64 < fit < S < 4096 and scan_chunk(S, scan_total(Nx, WIDTHS8)) == fit
    P = with_rejected(w, P0, [0, fit - 2, fit - 2, S - 4])
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc, 64, scan=WIDTHS8) as s:
            _, st = s.push(P)
            small, fold = [s.scan_result(k) for k in range(8)], s.result()
        big, fold_big = run_scan(acc, P, S, WIDTHS8)
    assert len(P) == S and list(np.flatnonzero(st != 0)) == [0, fit - 1, fit, S - 1]
    assert small[0]["n_used"] == S - 4 and small[0]["n_rejected"] == 4
    assert same_scans(big, small) and same(fold_big, fold)


# ---- 5. band ESS and ESS ----

class Int64Counts(B.Counts):
    """bandess_reference.Counts with the counts formed in int64 (module docstring)."""

    def __init__(self, rows, thr, Lmax):
        self.rows, self.thr, self.n = rows, np.atleast_2d(thr), len(rows)
        self.per = [self.counts(rows, t, Lmax) for t in self.thr]
        self._fin = {}

    @staticmethod
    def counts(rows, thr, L):
        b = np.asarray(rows) <= np.asarray(thr)[None, :]
        n, nx = b.shape
        assert n ** 3 * 4 < 2 ** 62
        N = b.sum(axis=0, dtype=np.int64)
        head = np.concatenate([np.zeros((1, nx), dtype=np.int64), np.cumsum(b, axis=0, dtype=np.int64)])      # head[k]: the first k
        C, E = np.zeros((L + 1, nx), dtype=np.int64), np.zeros((L + 1, nx), dtype=np.int64)
        for k in range(L + 1):
            C[k] = (b[k:] & b[:n - k]).sum(axis=0, dtype=np.int64)
            H, T = head[k], N - head[n - k]
            E[k] = n * n * C[k] - n * N * (2 * N - H - T) + (n - k) * N * N
        return N, C, E


def test_band_ess(accel_mod):
    """K = 8 thresholds -- the order statistics Q8 of every bin's own rows, the minimum, the maximum and a duplicate among them
    -- at L = 69 on GB: counts, E_k, cuts, p_hat and mcse_p exact in every bin, tau and ess within the suite's 4 ulp; the
    default block against block_chains = 7."""
    _, _, P, n_bad = chain(GB)
    sub = subset_bins(GB)
    t0 = time.perf_counter()
    with open_grid(accel_mod, GB) as acc:
        rows = rows_of(acc, GB)
        thr = truth_of(rows, Q8)
        out = {}
        for block in (0, 7):
            with capi.Summary(acc, block) as s:
                s.push(P)
                out[block] = band_pass(s, [P], thr, MAX_LAG)
    print(f"TIME band ESS GB: {time.perf_counter() - t0:.2f} s on the device side")
    assert B.same_band(out[0], out[7]) and all(np.array_equal(a, b) for key in ("C", "E") for a, b in zip(out[0][key], out[7][key]))
    ref = Int64Counts(rows, thr, MAX_LAG)
    for j in (0, 3, 6):                                     # the int64 counts are the reference's, on the subset
        N, C, E = B.counts(rows[:, sub], thr[j][sub], MAX_LAG)
        assert np.array_equal(N, ref.per[j][0][sub]) and np.array_equal(C, ref.per[j][1][:, sub]) and \
            np.array_equal(E, ref.per[j][2][:, sub].astype(object)), j
    B.check_exact("long-grid GB", out[0], ref, MAX_LAG, n_rejected=n_bad)


def test_ess(accel_mod):
    """L = 69 on GB (70 accepted samples: one past the chunk of 64; 2049 lag groups of 64 bins): the finish on the library's
    own lag products in every bin, the lag products against long double on the subset, the default block against
    block_chains = 7."""
    _, y, P, n_bad = chain(GB)
    t0 = time.perf_counter()
    with open_grid(accel_mod, GB) as acc:
        rows = rows_of(acc, GB)
        res = run_ess(acc, [P], MAX_LAG)
        res7 = run_ess(acc, [P], MAX_LAG, 7)
    print(f"TIME ESS GB: {time.perf_counter() - t0:.2f} s on the device side")
    assert res["lag"] == MAX_LAG and res["n_used"] == len(rows) and res["n_rejected"] == n_bad
    keys = capi.Summary.ESS_ARRAYS + capi.Summary.ESS_TOTALS + ("acov_M", "acov_l")
    assert all(np.array_equal(bits(np.asarray(res[k], dtype=np.float64)), bits(np.asarray(res7[k], dtype=np.float64))) for k in keys), "block_chains = 7"
    check_finish("long-grid GB", res, rows)
    check_acov("long-grid GB", res, rows, y, sel=subset_bins(GB))


# ---- 6. the LOO tail at the width of its sort ----

def loo_rows(acc, P):
    out = [gpu_rows(acc, P[k:k + 32768]) for k in range(0, len(P), 32768)]
    st, rows = np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out])
    assert np.all(st == 0)
    return rows


FULL_TAIL = 466033                                           # the largest n with M <= 2048


@pytest.mark.parametrize("n,M", [(116508, 1024), (116509, 1025), (116510, 1025)])
def test_loo_tail_width(accel_mod, n, M):
    """2 bins; M = 1024 sorts in 1024 slots, 1025 in 2048.  (3 sqrt(116 509) = 1024.003: the last chain with M = 1024 has
    116 508 samples.  n = 466 033, M = 2048, passed the same checks but is not kept: OBSERVED.)  tail_len exact, the cutoff as test_at_length of
    tests/test_summary_loo_gpu.py has it, elpd_loo and k-hat within that suite's bound on the GPU's own rows."""
    w = synth.workload_c2(Nx=2)
    y = spectrum_for(w)
    P = rows_around(w, n)
    assert tail_M(n) == M and tail_M(116508) == 1024 and tail_M(FULL_TAIL) == 2048 and tail_M(FULL_TAIL + 1) == 2049
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        t0 = time.perf_counter()
        rows = loo_rows(acc, P)
        print(f"TIME loo n={n}: the rows {time.perf_counter() - t0:.2f} s")
        t0 = time.perf_counter()
        with capi.Summary(acc, 4096) as s:
            s.push(P)
            res = s.loo(P)
        print(f"TIME loo n={n}: fold and LOO pass {time.perf_counter() - t0:.2f} s")
    assert res["n_used"] == n
    xs = np.sort(x_of(rows, y, dtype=np.float64), axis=0)
    cut = xs[n - M - 1]
    assert np.all(np.abs(res["cutoff"] - cut) <= 4 * np.spacing(np.abs(cut)))
    z = xs - xs[-1]
    assert np.array_equal(res["tail_len"], (z > z[n - M - 1]).sum(axis=0)) and np.all(res["tail_len"] == M)
    with np.errstate(over="ignore"):                         # the reference's weights of theta: exp overflows to the 0 weight it means
        check_loo_reference(f"long-grid n={n}", res, x_of(rows, y), np.arange(n), 2.0 ** -50, (1,), x64=xs)


def test_loo_refused_past_the_full_tail(accel_mod):
    """466 034 accepted samples have M = 2049: loo_begin is refused, and the fold goes on as if nothing had happened."""
    w = synth.workload_c2(Nx=2)
    y = spectrum_for(w)
    P = rows_around(w, FULL_TAIL + 1)
    assert tail_M(FULL_TAIL + 1) == 2049
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc, 4096) as s:
            s.push(P)
            before = s.result()
            assert before["n_used"] == FULL_TAIL + 1
            with pytest.raises(accel_mod.AccelError) as e:
                s.loo_begin()
            assert e.value.code == capi.E_INVALID
            assert same(s.result(), before)
            s.quantiles_begin((0.5,))                        # not left inside a mode
            s.quantiles_end()


# ---- 7. LOO, LOO-PIT and window-LOO on the long grids ----

_L, _PER_BIN = {}, {}


def accepted_rows(P):
    """The pushed rows without the rejected ones of with_rejected (a NaN parameter)."""
    return P[~np.isnan(P).any(axis=1)]


def l_of(acc, Nx):
    """The library's own l of the accepted samples on every bin (library_l: one push per sample); computed once per grid."""
    if Nx not in _L:
        _L[Nx] = library_l(acc, accepted_rows(chain(Nx)[2]))
        _L[Nx].setflags(write=False)
    return _L[Nx]


def per_bin_loo(acc, Nx):
    """(LOO-PIT result, LOO result, fold result) of the three passes with the default block; computed once per grid."""
    if Nx not in _PER_BIN:
        _PER_BIN[Nx] = LP.run_pit(acc, [chain(Nx)[2]], 0)
    return _PER_BIN[Nx]


def own_worst(mod, call):
    """The worst ratios that `call`, a check_reference of the support module `mod`, adds to mod.WORST, apart from what the
    module's own suite recorded there in the same session."""
    before = mod.WORST.pop("own", {})
    try:
        call()
    finally:
        mine = mod.WORST.get("own", {})
        mod.WORST["own"] = {k: max(before.get(k, 0.0), mine.get(k, 0.0)) for k in set(before) | set(mine)}
    return mine


def loo_totals_exact(tag, loo, fold):
    """The totals of loo_result from the library's own arrays, summed in bin order in long double as the host does (np.cumsum)."""
    e = np.cumsum(np.asarray(loo["elpd_loo"]).astype(LD))[-1]
    assert loo["elpd_loo_total"] == float(e) and loo["looic"] == float(-2 * LD(float(e))), tag
    assert loo["p_loo"] == float(np.cumsum(np.asarray(fold["lppd"]).astype(LD))[-1] - e), (tag, "p_loo")
    kh = np.asarray(loo["pareto_k"])
    with np.errstate(invalid="ignore"):
        assert loo["n_k_high"] == int((kh > 0.7).sum()) and loo["n_k_inf"] == int(np.isposinf(kh).sum()), tag
    assert np.isnan(loo["k_max"]) if np.all(np.isnan(kh)) else loo["k_max"] == np.nanmax(kh), tag


@pytest.mark.parametrize("Nx", [GB, GC, GD])
def test_loo_and_loo_pit(accel_mod, Nx):
    """Fold pass, LOO pass and PIT pass with the default block (63 on GB, 1 on GD) and with block_chains = 7 (3 on GD); on GC
    block 2 against block 3: every array and total has the same bits, the fold results are those the object gave before it
    entered the mode, n_used and n_rejected are exact.  One workgroup per bin in the finalize and prepare kernels: 4.2e6
    workgroups on GC / GD.  On GB and GD cutoff and tail_len are exact in every bin against the library's own l, the totals
    are recomputed from the library's own arrays, and the bins of subset_bins() are held to psis_reference
    (check_loo_reference) and loopit_reference (the LOO-PIT suite's check_reference) on the GPU's own rows.  With the 5 samples
    of GD M = 1, no bin has a Pareto fit and every k-hat is +inf, in the reference too."""
    _, y, P, n_bad = chain(Nx)
    b0, b1 = {GB: (0, 7), GC: (2, 3), GD: (0, 3)}[Nx]
    assert default_block(Nx) == {GB: 63, GC: 2, GD: 1}[Nx]
    tag = f"long-loo Nx={Nx}"
    t0 = time.perf_counter()
    with open_grid(accel_mod, Nx) as acc:
        rows = rows_of(acc, Nx) if Nx != GC else None
        res, loo, fold = per_bin_loo(acc, Nx) if b0 == 0 else LP.run_pit(acc, [P], b0)
        with capi.Summary(acc, b1) as s:                        # the other block: each result fetched once
            s.push(P)
            plain = s.result()
            both = s.loo(P, pit=True)
            fold_b = s.result()
        l = l_of(acc, Nx) if Nx != GC else None
    print(f"TIME {tag}: {time.perf_counter() - t0:.2f} s on the device side")
    n = len(P) - n_bad
    assert LP.same_pit(res, both) and LP.same_loo(loo, both) and same(fold, fold_b), ("block_chains", b0, b1)
    assert same(fold, plain), "the fold results before LOO mode, another block"
    assert tail_M(n) == (14 if Nx == GB else 1)
    for r in (res, loo, fold):
        assert r["n_used"] == n and r["n_rejected"] == n_bad, tag
    assert all(np.asarray(loo[k]).shape == (Nx,) for k in LP.LOO_KEYS + ("tail_len",)) and all(np.asarray(res[k]).shape == (Nx,) for k in LP.PIT_ARRAYS)
    if Nx == GC:
        return
    exact_structure(tag, loo, l)
    loo_totals_exact(tag, loo, fold)
    LP.check_totals(tag, res)
    sub = subset_bins(Nx)
    part = dict(loo, **{k: np.asarray(loo[k])[sub] for k in LP.LOO_KEYS + ("tail_len",)})
    with np.errstate(over="ignore"):
        check_loo_reference(tag, part, x_of(rows[:, sub], y[sub]), np.arange(n), 2.0 ** -50, (1,), x64=x_of(rows[:, sub], y[sub], dtype=np.float64),
                            totals=False)
        record("loopit", own_worst(LP, lambda: LP.check_reference(tag, res, loo, rows, y, np.arange(n), 2.0 ** -50, sel=sub)))


@pytest.mark.parametrize("Wd,first", [(1, 0), (7, 3), (20, 0), (512, 0)])
@pytest.mark.parametrize("Nx", [GB, GD])
def test_window_loo(accel_mod, Nx, Wd, first):
    """Window-LOO with its PIT pass, the default block against block_chains = 7 (3 on GD) bit for bit.  On GB W = 20 gives 6554
    windows in 33 tiles of the sums kernel and W = 512 gives 257 windows in 33 tiles; on GD W = 1 gives 4 194 305 windows: 16 385
    tiles per sample, 65 537 workgroups of the tail and PIT kernels, a scratch of one sample (three with block 3).  Exact on
    every window: n_windows, first_bin and last_bin are the partition's; cutoff and tail_len from the float64 ascending sums of
    the library's own l (wloo_support.exact_windows); the totals from the returned arrays; at W = 1 every array and total is
    the per-bin LOO and LOO-PIT result of test_loo_and_loo_pit (p = 1).  At W = 20 the object with the other block then runs a
    per-bin LOO and PIT pass, which gives the bits of an object that never saw the mode, and the fold keeps its bytes.  Against
    wloo_reference in its gathered form: the windows that hold subset_bins(), with the first and the last window -- at W = 512
    on GB those of subset_bins(GB, 32), 41 windows, since the long-double reference of all 221 with 70 samples takes 11 s on the host."""
    _, y, P, n_bad = chain(Nx)
    other = 7 if Nx == GB else 3
    tag = f"long-wloo Nx={Nx} W={Wd} first={first}"
    t0 = time.perf_counter()
    with open_grid(accel_mod, Nx) as acc:
        rows = rows_of(acc, Nx)
        res, loo, fold = WL.run_wloo(acc, [P], Wd, first, 0)
        with capi.Summary(acc, other) as s:                     # the other block: each result fetched once
            s.push(P)
            both = s.window_loo(P, Wd, first, pit=True)
            later = s.loo(P, pit=True) if Wd == 20 else None
            fold_b = s.result()
        l = l_of(acc, Nx)
        if Wd in (1, 20):
            pit1, loo1, fold1 = per_bin_loo(acc, Nx)
    print(f"TIME {tag}: {time.perf_counter() - t0:.2f} s on the device side")
    n = len(rows)
    assert LP.same_pit(res, both) and WL.same_wloo(loo, both) and same(fold, fold_b), ("block_chains", other)
    for r in (res, loo, fold):
        assert r["n_used"] == n and r["n_rejected"] == n_bad, tag
    WL.check_geometry(tag, loo, Nx, Wd, first)
    nw = loo["n_windows"]
    if Nx == GB:
        assert nw == {1: GB, 7: 18726, 20: 6554, 512: 257}[Wd]
    WL.check_totals(tag, res, loo, fold)
    WL.exact_windows(tag, loo, l, Nx, Wd, first)
    if Wd == 1:
        for a, b in (("elpd_lwo", "elpd_loo"), ("pareto_k", "pareto_k"), ("cutoff", "cutoff"), ("tail_len", "tail_len")):
            assert np.array_equal(bits(loo[a]), bits(loo1[b])), (tag, a)
        for a, b in (("elpd_lwo_total", "elpd_loo_total"), ("p_lwo", "p_loo"), ("k_max", "k_max"), ("n_k_high", "n_k_high"), ("n_k_inf", "n_k_inf")):
            assert np.array_equal(bits(float(loo[a])), bits(float(loo1[b]))), (tag, a)
        assert LP.same_pit(res, pit1), (tag, "the PIT arrays and totals against the per-bin LOO-PIT")
    if Wd == 20:
        assert LP.same_pit(later, pit1) and LP.same_loo(later, loo1), (tag, "a per-bin LOO pass after window-LOO mode")
        assert same(fold, fold1), (tag, "the fold results")
    sub = subset_bins(GB, 32) if (Nx, Wd) == (GB, 512) else subset_bins(Nx)
    sel, cols, f = windows_holding(sub, Nx, Wd, first)
    with np.errstate(over="ignore"):
        record("wloo", own_worst(WL, lambda: WL.check_reference(tag, WL.at_windows(res, sel, nw), WL.at_windows(loo, sel, nw), rows[:, cols], y[cols],
                                                                np.arange(n), 2.0 ** -50, Wd, f)))


def test_print_worst():
    """The worst ratios of this run per statistic, for the record (pytest -s)."""
    for tag, seen in list(WORST.items()) + [("ess", ESS_WORST), ("bandess-ulps", B.WORST)]:
        print(f"WORST {tag}: " + " ".join(f"{k}={v:.3g}" for k, v in seen.items()))
