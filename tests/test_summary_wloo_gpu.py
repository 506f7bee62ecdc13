"""Leave-one-window-out PSIS-LOO and LOO-PIT per window on the GPU (tamcmc_summary_wloo_*, include/tamcmc_accel.h;
tamcmc_wloo.hip): the per-bin machinery fed with the window sums of l, over the windows of the windowed check.

Reference: wloo_reference() of tests/wloo_reference.py -- summary_support.psis_reference on window sums formed in long double
from the GPU's own rows, and loopit_reference's weights composed with window_reference's tails for the sub-mode.

Exact checks (no tolerance): W = 1 is LOO mode and its LOO-PIT sub-mode bit for bit (p a power of two for the PIT arrays: for
p = 3 the windowed check's tails take 3 (y / M) where the per-bin check takes (3 y) / M, as tests/test_summary_window_gpu.py
says, so there the PIT arrays are held to the reference instead); n_windows, first_bin and last_bin are the partition's; every
result is bitwise independent of block_chains (1, 7, 64, n, n + 1) and of the split of either pass into pushes, pushes of one
row included; host and device pointers give the same bits; a chain with rejected rows gives the bits of the chain without
them; wloo_result returns the same bits before wloo_pit_begin, after it and after the pass; the fold, predictive, window and
scan results and a later per-bin LOO pass keep their bytes; across the tiles of the sums kernel and the workgroups of the tail
and PIT kernels (test_across_sums_tiles, test_across_tail_workgroups: grids of up to 8704 bins, every class of W) cutoff is the
order statistic of the float64 ascending window sums of the library's own l in every window, and tail_len the count above it.

Against the reference the bound is the LOO-PIT suite's: per case and per quantity (the maximum over the windows; relative to
max(1, |value|), absolute for loo_pit), 10 x the larger of
    (a) the reference's own change when the rows AND the per-bin x = -l are each perturbed by 2^-50 relative, one sign per
        distinct row and bin, the maximum over three seeds, and
    (b) the difference between the reference run in float64, the sums added in ascending order, and in long double.
tail_len and the places where k-hat is +inf must be equal.  On the oracle's rows the perturbation is 1e-12 relative, the
project's per-bin model bar.  Every worst ratio is printed before it is asserted (pytest -s).

Worst ratios observed on an MI355X over all cases below, on the GPU's own rows: elpd_lwo 0.12, pareto_k 0.11, cutoff 0.1, loo_log_cdf 0.083,
loo_log_sf 0.12, loo_pit 0.1, is_ess 0.1, log_wsum 0.11, elpd_lwo against the reference's weights 0.11 (across the tiles and workgroups
alone: 0.1, 0.11, 0.1, 0.076, 0.077, 0.1, 0.1, 0.11 and 0.1; a ratio of 0.1 is a result that equals the float64 reference where the
bound is 10 x that reference's distance from the long-double one); on the oracle's rows 0.00025, 5.8e-5, 3.2e-5,
0.00094, 0.00092, 0.0014, 0.00014, 6e-5 and 0.00025.  The planted window: loo_log_sf = -8.63901 against the windowed check's -8.63862, is_ess 99.96 of 100.
"""
import time

import numpy as np
import pytest

import workloads as W
from loopit_support import PIT_ARRAYS, PIT_TOTALS, same_pit
from summary_support import (ULP, c2_case, c2_chain, gpu_rows, library_l, other_cases, row_groups, same, same_pred, same_scans, same_win,
                             spectrum_for, tail_M, true_model)
from support import bits, in_torch_process, pyorc
from tamcmc_amd import capi, synth
from wloo_support import (LOO_KEYS, check_geometry, check_pool, check_reference, check_reference_at, check_totals,
                          exact_windows, run_wloo, same_wloo)

pytestmark = pytest.mark.gpu


def open_cfg(accel_mod, w, y, cfg, mid=2):
    if cfg == "chi-square":
        sigma = 0.05 + 0.2 * np.abs(np.sin(np.arange(len(y))))
        return accel_mod.Accel(mid, w["plength"], w["x"], y, sigma_y=sigma, likelihood_case=1), 1, 1, sigma
    p = int(cfg[1:])
    return accel_mod.Accel(mid, w["plength"], w["x"], y, likelihood_p=float(p)), 0, p, None


# ---- 1. W = 1 is the per-bin mode ----

def per_bin(acc, P, block=0):
    with capi.Summary(acc, block) as s:
        s.push(P)
        return s.loo(P, pit=True)


@pytest.mark.parametrize("S", [1, 20, 21, 37, 441, 455, 456, 1000])
def test_one_bin_per_window_is_the_per_bin_mode(accel_mod, S):
    """elpd_lwo, pareto_k, cutoff, tail_len and the totals equal loo_result's and the five PIT arrays loo_pit_result's, bit
    for bit: no tail rule (n = 1), raw weights (n <= 20), the first Pareto fit (21), M = 63, 64, 65 on either side of a step
    of the search's trip count, and 1000 samples.  At 37 samples also p = 2, chi_square, the local model id 11 and p = 3
    (there the PIT arrays against the reference: module docstring)."""
    w, y, P = c2_chain(65, S)
    cases = [("p1", w, y, P, 2)]
    if S == 37:
        cases += [("p2", w, y, P, 2), ("chi-square", w, y, P, 2), ("p3", w, y, P, 2)]
        c1 = other_cases()["c1-id11-fused"]
        cases.append(("p1", c1[0], spectrum_for(c1[0]), c1[1], 11))
    for cfg, cw, cy, cP, mid in cases:
        tag = f"one-bin S={S} {cfg} id{mid}"
        acc, like, p, sigma = open_cfg(accel_mod, cw, cy, cfg, mid)
        with acc:
            Nx = acc.Nx
            _, st, rows = gpu_rows(acc, cP)
            assert np.all(st == 0)
            bin_ = per_bin(acc, cP, 7)
            for first in (0, 1):
                res, loo, fold = run_wloo(acc, [cP], 1, first, 7)
                check_geometry(tag, loo, Nx, 1, first)
                assert loo["n_windows"] == Nx and np.array_equal(loo["first_bin"], np.arange(Nx)) and np.array_equal(loo["last_bin"], np.arange(Nx))
                for a, b in (("elpd_lwo", "elpd_loo"), ("pareto_k", "pareto_k"), ("cutoff", "cutoff")):
                    assert np.array_equal(bits(loo[a]), bits(bin_[b])), (tag, a)
                assert np.array_equal(loo["tail_len"], bin_["tail_len"]), tag
                for a, b in (("elpd_lwo_total", "elpd_loo_total"), ("p_lwo", "p_loo"), ("k_max", "k_max"), ("n_k_high", "n_k_high"),
                             ("n_k_inf", "n_k_inf"), ("n_used", "n_used"), ("n_rejected", "n_rejected")):
                    assert np.array_equal(bits(float(loo[a])), bits(float(bin_[b]))), (tag, a)
                if cfg != "p3":
                    assert same_pit(res, bin_), (tag, "the PIT arrays and totals")
                check_totals(tag, res, loo, fold)
        if cfg == "p3":
            check_reference(tag, res, loo, rows, cy, np.arange(len(cP)), 2.0 ** -50, 1, 0, like, p, sigma)


# ---- 2. geometry ----

def grids(Wd, f):
    """Grids of 2 ... 700 bins whose last window is full, partial and a single bin, one with Nx < first, and the longest."""
    cand = {f + 2 * Wd, f + Wd, f + 2 * Wd + max(Wd // 2, 1), f + Wd + max(Wd // 2, 1), f + 2 * Wd + 1, f + Wd + 1, f + 1, f - 1, f}
    if f == Wd or f + Wd > 700:
        cand.add(700)
    return sorted(n for n in cand if 2 <= n <= 700)


@pytest.mark.parametrize("Wd", [2, 3, 5, 20, 64, 511, 512])
def test_geometry(accel_mod, Wd):
    """first in {0, 1, W - 1, W}; the last window full, partial and a single bin; Nx < first (one window).  These grids of
    at most f + 2 W + 1 bins hold one to four windows, all in the first tile of the sums kernel; only the 700-bin grid of
    W = 2 reaches a second tile (test_across_sums_tiles crosses the tiles).  n_windows, first_bin and last_bin are the partition's, and
    every window's results are the reference's within the bound, so every bin went to its own window and every window got
    its own shape.  The case is W: its grids hold one to a few windows each, and a maximum over one window of how far two
    reference runs happen to differ is no bound (at one window of 62 bins the float64 run lands within 3e-17 of the
    long-double one, a fifth of an ulp of 1, where tamcmc_window.h measures 4.6e-15 for the tails at that shape), so errors and
    bounds are maxima over the windows of all grids of the case."""
    pool = {}
    for first in sorted({0, 1, Wd - 1, Wd}):
        f = Wd if first == 0 else first
        for Nx in grids(Wd, f):
            w, y, P = c2_chain(Nx, 37)
            tag = f"geometry W={Wd} first={first} Nx={Nx}"
            with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
                _, st, rows = gpu_rows(acc, P)
                assert np.all(st == 0)
                res, loo, fold = run_wloo(acc, [P], Wd, first, 16)
            check_geometry(tag, loo, Nx, Wd, first)
            if Nx < f:
                assert loo["n_windows"] == 1 and loo["last_bin"][0] == Nx - 1, tag
            check_totals(tag, res, loo, fold)
            check_reference(tag, res, loo, rows, y, np.arange(len(P)), 2.0 ** -50, Wd, first, pool=pool)
    check_pool(f"geometry W={Wd}", pool)


def windows_per_tile(Wd):
    """The whole windows a workgroup of the sums kernel stages (wloo_launch_sums, tamcmc_wloo.hip): 4096 bins, at most 256."""
    return min(256, 4096 // Wd)


def grid_of(N, r, Wd, f):
    """The grid of N windows whose last one has r bins: n_windows = 1 + ceil((Nx - f) / W)."""
    return f + (N - 2) * Wd + r


def across(accel_mod, name, Wd, counts):
    """Body of the two tests below.  first in {0, 1, W - 1, W} x the window counts `counts`, the last window full, half and a
    single bin -- one of the three per (first, count), in rotation, so that every length meets every count and every first:
    the 16 grids of a width take 1.1 ... 2.2 s on an MI355X box, 0.9 ... 1.9 s of it the long-double reference on the host, and
    with all three lengths would take three times that.  Every grid goes through run_wloo with block 16, then
      exact, every window: the partition; the totals from the returned arrays; cutoff bit for bit the order statistic
        sort(-S)[n - M - 1] of the float64 ascending sums S of the library's own l, tail_len the count above it (exact_windows);
      the reference, on the gathered grid of check_reference_at: the windows at a tile edge (wpt - 1, wpt, 2 wpt - 1, 2 wpt), the
        first two, the last two and 32 drawn by default_rng(20262); errors and bounds pooled over the case's grids.
    Not checked: that the windows of the first tile have the bits they have on the grid cut down to that tile.  The model's
    value in a bin depends on the grid's length: at W = 20, first = 0 the rows of the 4090-bin grid and of its first 4080 bins
    (the same x, y and parameters) differ by one ulp in bin 1 of the first sample and in others, so l and every window result
    differ too.  The exact cutoff above takes that check's place."""
    wpt = windows_per_tile(Wd)
    assert tail_M(37) == 8
    lengths = sorted({Wd, max(Wd // 2, 1), 1}, reverse=True)
    pool, seen, t_dev, t_ref = {}, set(), 0.0, 0.0
    for a, first in enumerate(sorted({0, 1, Wd - 1, Wd})):
        f = Wd if first == 0 else first
        for b, N in enumerate(counts):
            r = lengths[(a + b) % len(lengths)]
            Nx = grid_of(N, r, Wd, f)
            if (first, Nx) in seen:
                continue
            seen.add((first, Nx))
            w, y, P = c2_chain(Nx, 37)
            tag = f"{name} W={Wd} first={first} N={N} r={r} Nx={Nx}"
            t0 = time.perf_counter()
            with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
                _, st, rows = gpu_rows(acc, P)
                assert np.all(st == 0)
                res, loo, fold = run_wloo(acc, [P], Wd, first, 16)
                l = library_l(acc, P)
            t1 = time.perf_counter()
            assert loo["n_windows"] == N, tag
            check_geometry(tag, loo, Nx, Wd, first)
            check_totals(tag, res, loo, fold)
            exact_windows(tag, loo, l, Nx, Wd, first)
            edges = [v for v in (wpt - 1, wpt, 2 * wpt - 1, 2 * wpt, 0, 1, N - 2, N - 1) if 0 <= v < N]
            drawn = np.random.default_rng(20262).choice(N, size=min(32, N), replace=False)
            t2 = time.perf_counter()
            check_reference_at(tag, np.concatenate([edges, drawn]), res, loo, rows, y, np.arange(len(P)), 2.0 ** -50, Wd, first, pool=pool)
            t_dev, t_ref = t_dev + t1 - t0, t_ref + time.perf_counter() - t2
    print(f"TIME {name} W={Wd}: {len(seen)} grids, {t_dev:.2f} s on the device side, {t_ref:.2f} s in the reference")
    check_pool(f"{name} W={Wd}", pool)


@pytest.mark.parametrize("Wd", [2, 3, 16, 17, 20, 64, 511, 512])
def test_across_sums_tiles(accel_mod, Wd):
    """N = wpt, wpt + 1, 2 wpt and 2 wpt + 1 windows, wpt = min(256, 4096 / W) the windows of a tile of the sums kernel: the
    second tile (w0 > 0), the tile edge and a last tile of one window, which test_geometry's grids never reach.  W = 2 with a
    partial first window; 3, the smallest width that otherwise never leaves the first tile; 16 and 17 on either side of
    wpt = 256 | 240; 20 (204); 64 (64); 511 (8 windows of 4088 bins) and 512 (8).  The longest grid has 8704 bins.  What is
    checked: across().
    Mutant (not committed): in tamcmc_wloo_sums_kernel, for W >= 3 and w0 > 0, the thread of a tile's first window adds len - 1
    terms; in bounds.  This module before this test: 38 passed; this test: fails at every W >= 3 on the exact cutoff (W = 2 spared)."""
    wpt = windows_per_tile(Wd)
    across(accel_mod, "tiles", Wd, (wpt, wpt + 1, 2 * wpt, 2 * wpt + 1))


@pytest.mark.parametrize("Wd", [3, 20])
def test_across_tail_workgroups(accel_mod, Wd):
    """N = 63, 64, 65 and 129 windows: the tail and PIT kernels give a window to a thread and 64 threads to a workgroup, and
    with W >= 3 the suite had at most 43 windows.  One wave short of full, full, one window in a second workgroup, one in a
    third.  What is checked: across()."""
    across(accel_mod, "workgroups", Wd, (63, 64, 65, 129))



# ---- 3. against the reference ----

@pytest.mark.parametrize("name", ["c2-700-S400-W20", "c2-700-S456-W7-first3", "c2-65-S1000-W5", "c2-2-S37-W2", "id11-W20", "p2-W64",
                                  "p3-W20-first7", "chi-square-W20", "chi-square-W512"])
def test_against_the_reference(accel_mod, name):
    """The cases the issue's probe ran on the oracle's rows, here on the GPU's own; the shortest grid; the local model id 11
    on the fused launch; p = 2 and 3 (shapes 128 and 60) and chi_square, at W = 512 too."""
    mid, cfg, first = 2, "p1", 0
    if name.startswith("c2-700-S400"):
        (w, y, P), Wd = c2_chain(700, 400), 20
    elif name.startswith("c2-700-S456"):
        (w, y, P), Wd, first = c2_chain(700, 456), 7, 3
    elif name.startswith("c2-65"):
        (w, y, P), Wd = c2_chain(65, 1000), 5
    elif name.startswith("c2-2"):
        (w, y, P), Wd = c2_chain(2, 37), 2
    elif name.startswith("id11"):
        w, P, _ = other_cases()["c1-id11-fused"]
        y, Wd, mid = spectrum_for(w), 20, 11
    else:
        w, y, P = c2_chain(700, 100)
        cfg = name.rsplit("-W", 1)[0] if name.startswith("chi") else name.split("-")[0]
        Wd = int(name.split("-W")[1].split("-")[0])
        first = 7 if "first7" in name else 0
    acc, like, p, sigma = open_cfg(accel_mod, w, y, cfg, mid)
    with acc:
        Nx = acc.Nx
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0), name
        res, loo, fold = run_wloo(acc, [P], Wd, first)
        a = len(P) // 3
        other, loo_o, _ = run_wloo(acc, [P], Wd, first, 7, [P[:a], P[a:a + 1], P[a + 1:]], [P[:1], P[1:]])
    assert same_pit(res, other) and same_wloo(loo, loo_o), name
    check_geometry(name, loo, Nx, Wd, first)
    check_totals(name, res, loo, fold)
    ref = check_reference(name, res, loo, rows, y, np.arange(len(P)), 2.0 ** -50, Wd, first, like, p, sigma)
    if Wd > 1 and name.startswith("c2-700-S400"):
        # the statistic is not the sum of the per-bin values: the issue's probe saw up to 6.2e-3 of difference
        with accel_mod.Accel(2, w["plength"], w["x"], y) as acc2:
            bin_ = per_bin(acc2, P)
        sums = np.add.reduceat(bin_["elpd_loo"], loo["first_bin"])
        print(f"DISTINCT {name}: max |elpd_lwo - sum of elpd_loo over the window| = {float(np.max(np.abs(loo['elpd_lwo'] - sums))):.3g}; "
              f"k-hat in [{float(np.min(loo['pareto_k'])):.3g}, {float(np.max(loo['pareto_k'])):.3g}]")
        assert np.max(np.abs(loo["elpd_lwo"] - sums)) > 1e-6
    assert ref["tail_len"].shape == loo["tail_len"].shape


@pytest.mark.parametrize("name", ["c2-700-S400-W20", "c2-700-S456-W7-first3", "c2-65-S1000-W5"])
def test_against_the_oracle(accel_mod, name):
    """The same three cases on the oracle's rows: the perturbation is the project's per-bin model bar."""
    if name.startswith("c2-700-S400"):
        (w, y, P), Wd, first = c2_chain(700, 400), 20, 0
    elif name.startswith("c2-700-S456"):
        (w, y, P), Wd, first = c2_chain(700, 456), 7, 3
    else:
        (w, y, P), Wd, first = c2_chain(65, 1000), 5, 0
    _, rst, M = pyorc().generate_batch(2, w["plength"], w["x"], y, P, np.ones(len(P)), want_models=True)
    assert np.all(rst == 0)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        res, loo, fold = run_wloo(acc, [P], Wd, first)
    check_totals(name, res, loo, fold)
    check_reference(f"oracle {name}", res, loo, M, y, row_groups(P), 1e-12, Wd, first)
    assert np.nanmax(loo["pareto_k"]) <= 0.7, (name, "the issue's probe saw no window above 0.7")


# ---- 4. nothing but the samples and their order decides a bit ----

@pytest.mark.parametrize("cfg", ["p1", "p3", "chi-square"])
def test_block_size_and_push_split_cannot_change_a_bit(accel_mod, cfg):
    """block_chains 1, 7, 64, n and n + 1; both passes in pushes of one row; W = 20 with first = 7 on 700 bins (36 windows),
    and W = 3 on the same grid (234 windows: the tail and PIT kernels' second wave is partial)."""
    w, y, P = c2_chain(700, 37)
    n = len(P)
    ones = [P[k:k + 1] for k in range(n)]
    acc, _, _, _ = open_cfg(accel_mod, w, y, cfg)
    with acc:
        for Wd, first in ((20, 7), (3, 0)):
            base, loo, _ = run_wloo(acc, [P], Wd, first, 1)
            for B in (7, 64, n, n + 1, 0):
                res, loo_b, _ = run_wloo(acc, [P], Wd, first, B)
                assert same_pit(res, base) and same_wloo(loo_b, loo), (cfg, Wd, "block_chains", B)
            res, loo_b, _ = run_wloo(acc, ones, Wd, first, 7)
            assert same_pit(res, base) and same_wloo(loo_b, loo), (cfg, Wd, "pushes of one row")
            res, loo_b, _ = run_wloo(acc, [P], Wd, first, 64, [P[:5], P[5:6], P[6:]], ones)
            assert same_pit(res, base) and same_wloo(loo_b, loo), (cfg, Wd, "the passes split differently")


def test_rejected_samples(accel_mod):
    """A NaN parameter and an empty truncation window among 30 healthy samples, first and last in the chain, at block edges
    and alone in a block of one: left out of every window, counted, and the bits are those of the chain without them."""
    w = W.make(2, Nx=700)
    b = W.split(w)
    y = spectrum_for(w)
    good = W.perturbed(w, 30, scale=0.002)
    empty = W.perturbed(w, 1, scale=0.002, seed=8)[0]
    empty[b["q"] + 1] = -1.0
    nan = W.perturbed(w, 1, scale=0.002, seed=9)[0]
    nan[b["z"] + 9] = np.nan
    P = np.array([empty] + list(good[:3]) + [nan, nan] + list(good[3:25]) + [empty] + list(good[25:]) + [nan])
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, stg, rows = gpu_rows(acc, good)
        assert np.all(stg == 0)
        clean, loo, fold = run_wloo(acc, [good], 20, 7, 3)
        for B in (4, 1, 0):                                     # B = 4: rejected rows at 0, 4 and 5 -- a block's first and second
            res, loo_b, _ = run_wloo(acc, [P], 20, 7, B)
            assert res["n_used"] == 30 and res["n_rejected"] == 5 and loo_b["n_used"] == 30 and loo_b["n_rejected"] == 5
            for k in PIT_ARRAYS + PIT_TOTALS[2:]:
                assert np.array_equal(bits(np.asarray(res[k], dtype=np.float64)), bits(np.asarray(clean[k], dtype=np.float64))), (B, k)
            for k in LOO_KEYS + ("elpd_lwo_total", "p_lwo", "k_max"):
                assert np.array_equal(bits(np.asarray(loo_b[k], dtype=np.float64)), bits(np.asarray(loo[k], dtype=np.float64))), (B, k)
            assert np.array_equal(loo_b["tail_len"], loo["tail_len"]) and np.array_equal(res["loo_pit_hist"], clean["loo_pit_hist"])
    check_reference("rejected", clean, loo, rows, y, np.arange(30), 2.0 ** -50, 20, 7)


def test_ties(accel_mod):
    """Every row twice, one row fifty times, and all rows equal: every tail sample is found -- wloo_pit_result would refuse
    otherwise -- and with all rows equal there is no tail (tail_len = 0, k-hat = +inf) and the weights are equal, so the
    tails are the windowed check's."""
    w, y, P = c2_chain(65, 60)
    P2 = np.repeat(P, 2, axis=0)
    P50 = np.concatenate([P[:30], np.tile(P[7], (50, 1)), P[30:]])
    Pe = np.tile(P[5], (50, 1))
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        for tag, Q in (("twice", P2), ("fifty", P50)):
            _, st, rows = gpu_rows(acc, Q)
            assert np.all(st == 0)
            res, loo, fold = run_wloo(acc, [Q], 5, 0, 16)
            other, loo_o, _ = run_wloo(acc, [Q], 5, 0, 1, None, [Q[:1], Q[1:3], Q[3:]])
            assert same_pit(res, other) and same_wloo(loo, loo_o), tag
            check_totals(tag, res, loo, fold)
            check_reference(f"ties-{tag}", res, loo, rows, y, row_groups(Q), 2.0 ** -50, 5)
        eq, loo_eq, _ = run_wloo(acc, [Pe], 5, 0, 7)
        with capi.Summary(acc, 7, window=5) as s:
            s.push(Pe)
            post = s.window_result()
    assert np.all(loo_eq["tail_len"] == 0) and np.all(np.isposinf(loo_eq["pareto_k"])) and loo_eq["n_k_inf"] == loo_eq["n_windows"] == 13
    n = 50
    for a, b in (("loo_log_cdf", "log_cdf"), ("loo_log_sf", "log_sf")):
        assert np.all(np.abs(eq[a] - post[b]) <= (n + 2) * ULP), (a, float(np.max(np.abs(eq[a] - post[b]))))
    assert np.all(np.abs(eq["is_ess"] - n) <= n * (n + 2) * ULP) and np.all(np.abs(eq["log_wsum"] - np.log(50.0)) <= 2.0 * np.spacing(np.log(50.0)))


def test_at_length(accel_mod):
    """70 001 samples of a 65-bin grid, W = 5, in blocks of 4096: M = 794, a search of 10 steps down a column of 795 slots,
    17 pushes of blocks that straddle 65 535.  The exact checks cover every window, the reference three of the thirteen."""
    S = 70001
    w = synth.workload_c2(Nx=65)
    y = spectrum_for(w)
    P = synth.chain_params(w, S)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        with capi.Summary(acc, 4096) as s:
            s.push(P)
            fold = s.result()
            res = s.window_loo(P, 5, pit=True)
    assert tail_M(S) == 794 and res["n_used"] == S and res["n_windows"] == 13 and np.all(res["tail_len"] == 794)
    check_totals("at-length", res, res, fold)
    # the reference on the first, the middle and the last window: their 15 bins are a grid of three full windows
    sel = np.array([0, 6, 12])
    cols = (5 * sel[:, None] + np.arange(5)[None, :]).reshape(-1)
    part = {k: (np.asarray(v)[sel] if isinstance(v, np.ndarray) and v.shape == (13,) else v) for k, v in res.items()}
    check_reference("at-length", part, part, rows[:, cols], y[cols], np.arange(S), 2.0 ** -50, 5)


# ---- 5. the rest of the object ----

def test_other_results_keep_their_bytes(accel_mod):
    """The fold, predictive, window and scan results of an object are the same bytes before window-LOO mode, inside its
    sub-mode after a pass, and after wloo_end; and a per-bin LOO pass after it gives the bits of one that never saw the mode."""
    w, y, P, _, _ = c2_case(257)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        fresh = per_bin(acc, P, 16)
        with capi.Summary(acc, 16, predictive=True, window=(16, 5), scan=(4, 16)) as s:
            s.push(P)
            before = (s.result(), s.predictive_result(), s.window_result(), [s.scan_result(k) for k in range(2)])

            def unchanged(where):
                now = (s.result(), s.predictive_result(), s.window_result(), [s.scan_result(k) for k in range(2)])
                assert same(now[0], before[0]) and same_pred(now[1], before[1]) and same_win(now[2], before[2]) and \
                    same_scans(now[3], before[3]), where
            s.wloo_begin(20, 7)                                # other windows than the windowed check's
            unchanged("after wloo_begin")
            s.push(P)
            s.wloo_result()
            s.wloo_pit_begin()
            unchanged("after wloo_pit_begin")
            s.push(P)
            s.wloo_pit_result()
            unchanged("after the PIT pass")
            s.wloo_end()
            unchanged("after wloo_end")
            later = s.loo(P, pit=True)
            unchanged("after a per-bin LOO pass")
    for k in ("elpd_loo", "pareto_k", "cutoff") + PIT_ARRAYS:
        assert np.array_equal(bits(later[k]), bits(fresh[k])), k
    assert np.array_equal(later["tail_len"], fresh["tail_len"])


def test_refusals_and_state(accel_mod):
    w, y, P, _, _ = c2_case(257)
    T = np.ones(len(P))
    E = capi.E_INVALID
    extra = synth.chain_params(w, 5, seed=4242)
    others = synth.chain_params(w, len(P), seed=977)            # as many rows, other rows

    def refused(fn, *a):
        with pytest.raises(accel_mod.AccelError) as e:
            fn(*a)
        assert e.value.code == E

    acc = accel_mod.Accel(2, w["plength"], w["x"], y)
    clean, clean_loo, _ = run_wloo(acc, [P], 20, 7)
    s = capi.Summary(acc, 8)
    refused(s.wloo_begin, 20)                                                # no sample yet
    refused(s.wloo_result)
    refused(s.wloo_pit_begin)
    refused(s.wloo_pit_result)
    refused(s.wloo_pit_kernel_time)
    refused(s.wloo_end)
    s.push(P)
    full = s.result()
    for bad in ((0, 0), (513, 0), (-1, 0), (20, 21), (20, -1)):              # W or first out of range
        refused(s.wloo_begin, *bad)
    # every cross-mode begin is refused, both ways
    modes = (("quantile", lambda: s.quantiles_begin([0.5]), s.quantiles_end), ("loo", s.loo_begin, s.loo_end),
             ("ess", lambda: s.ess_begin(0), s.ess_end), ("bandess", lambda: s.bandess_begin(full["mean_M"]), s.bandess_end))
    for name, begin, end in modes:
        begin()
        refused(s.wloo_begin, 20)
        end()
    assert s.wloo_begin(20, 7) == 14
    for name, begin, end in modes:
        refused(begin)
    refused(s.wloo_begin, 20, 7)                                             # twice
    refused(s.predictive_enable)
    refused(s.window_enable, 20)
    refused(s.scan_enable, 4)
    refused(s.wloo_pit_begin)                                                # nothing pushed in the mode
    refused(s.wloo_result)                                                   # (discards an empty pass)
    s.push(P[:20])
    refused(s.wloo_pit_begin)                                                # the pass is incomplete -- and survives:
    s.push(P[20:])
    assert same_wloo(s.wloo_result(), clean_loo), "the pass did not survive a refused wloo_pit_begin"
    s.push(P[3:4])                                                           # one sample too many: discarded, repeatable
    refused(s.wloo_result)
    s.push(P[:-1])                                                           # a short count
    refused(s.wloo_result)
    s.push(others)                                                           # other rows, the right count: another result, not refused
    assert not same_wloo(s.wloo_result(), clean_loo)
    s.push(P)                                                                # ... and a pass on top of it is one pass too many
    refused(s.wloo_result)
    s.push(P)
    assert same_wloo(s.wloo_result(), clean_loo), "after discarded passes"
    acc.begin(P, T)                                                          # a batch in flight
    refused(s.wloo_pit_begin)
    refused(s.wloo_result)
    acc.end()
    acc.arm(len(P))                                                          # a batch armed
    refused(s.wloo_pit_begin)
    acc.disarm()
    s.wloo_pit_begin()
    refused(s.wloo_pit_begin)                                                # twice
    refused(s.wloo_pit_result)                                               # nothing pushed
    s.push(P[:-1])                                                           # a pass of S - 1 samples
    refused(s.wloo_pit_result)
    s.push(P)
    s.push(P[3:4])                                                           # one sample too many
    refused(s.wloo_pit_result)
    s.push(others)                                                           # S other rows: the counts are right, the tail samples are not found
    refused(s.wloo_pit_result)
    s.push(P[:20])                                                           # the right pass, in two pushes
    s.push(P[20:])
    assert same_pit(s.wloo_pit_result(), clean), "after discarded passes"
    assert same_wloo(s.wloo_result(), clean_loo)
    assert same(s.result(), full)
    s.wloo_end()
    refused(s.wloo_pit_result)
    refused(s.wloo_result)
    s.push(extra)                                                            # folds on as if nothing had happened
    after = s.result()
    with capi.Summary(acc, 8) as s2:
        s2.push(P)
        s2.push(extra)
        assert same(s2.result(), after), "a summary that never entered the mode differs"
    allP = np.concatenate([P, extra])
    d = s.window_loo(allP, 20, 7, pit=True)                                  # the convenience call leaves the mode
    assert d["n_used"] == len(P) + 5 and all(k in d for k in PIT_ARRAYS + LOO_KEYS)
    assert set(s.window_loo(allP, 20)) == set(capi.Summary.WLOO_ARRAYS + ("tail_len", "first_bin", "last_bin") + capi.Summary.WLOO_TOTALS)
    refused(s.wloo_end)
    with pytest.raises(accel_mod.AccelError):                                # ... also when the pass is refused
        s.window_loo(P, 20)
    refused(s.wloo_end)
    s.wloo_begin(20)
    s.push(allP)
    s.wloo_pit_begin()
    s.push(P[:9])
    s.reset()                                                                # leaves the sub-mode and the mode, forgets every sample
    refused(s.wloo_pit_result)
    refused(s.wloo_result)
    assert s.result()["n_used"] == 0
    s.push(P)
    assert same(s.result(), full)
    s.wloo_begin(5)
    s.push(P)
    s.wloo_pit_begin()
    s.push(P[:9])
    refused(acc.close)                                                       # a live summary holds the context
    s.close()                                                                # inside the sub-mode, a pass half pushed
    acc.close()
    # chi(2,2p): the sub-mode needs p >= 1 and p W <= 512; the mode itself does not
    with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=3.0) as acc3:
        with capi.Summary(acc3, 8) as s:
            s.push(P)
            for Wd, ok in ((170, True), (171, False)):
                s.wloo_begin(Wd)
                s.push(P)
                s.wloo_result()
                if ok:
                    s.wloo_pit_begin()
                else:
                    refused(s.wloo_pit_begin)
                s.wloo_end()
    with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=0.5) as acc0:
        with capi.Summary(acc0, 8) as s:
            s.push(P)
            s.wloo_begin(5)
            s.push(P)
            s.wloo_result()
            refused(s.wloo_pit_begin)


def test_profile_and_kernel_time(accel_mod):
    """profile / kernel_time as in LOO mode: one timed launch per block of the LOO pass, one per wloo_result, the prepare
    kernel; the PIT pass's blocks on a timer of their own."""
    w, y, P, _, _ = c2_case(257)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc, 8) as s:
            s.push(P)
            s.profile(True)
            s.wloo_begin(20)
            s.push(P)
            s.wloo_result()
            ms, n = s.kernel_time()
            assert n == 5 + 1 and ms > 0.0                                    # 37 samples in blocks of 8, and the finalize kernel
            s.wloo_pit_begin()
            s.push(P)
            s.wloo_pit_result()
            assert s.kernel_time()[1] == 5 + 1 + 1                            # the prepare kernel
            ms, n = s.wloo_pit_kernel_time()
            assert n == 5 and ms > 0.0
            s.wloo_end()


# ---- 6. what the mode is for ----

def test_planted_run(accel_mod):
    """The windowed suite's planted run (tests/test_summary_window_gpu.py): 700 bins of y = M e, in window 17 of 35 y = 2 M.
    That window is the minimum of the window loo_log_sf and lies below log(0.01 / n_windows).  Observed on an MI355X: see
    the PLANTED line: loo_log_sf = -8.63901 beside the windowed check's -8.63862 (which uses the window's data twice), against
    log(0.01 / 35) = -8.16; is_ess 99.96 of 100 and k-hat -0.03: a chain this narrow barely moves when the window leaves."""
    w = synth.workload_c2(Nx=700)
    M0 = true_model(w)
    y = M0 * np.random.default_rng(0).exponential(size=700)
    k = 17
    y[20 * k:20 * (k + 1)] = 2.0 * M0[20 * k:20 * (k + 1)]
    P = synth.chain_params(w, 100, scale=0.05)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        res, loo, _ = run_wloo(acc, [P], 20, 0, 64, window=20)
        with capi.Summary(acc, 64, window=20) as s:
            s.push(P)
            post = s.window_result()
    print(f"PLANTED window {k}: loo_log_sf = {res['loo_log_sf'][k]:.6g}, the windowed check's log_sf = {post['log_sf'][k]:.6g}, "
          f"is_ess = {res['is_ess'][k]:.6g}, pareto_k = {loo['pareto_k'][k]:.4g}, elpd_lwo = {loo['elpd_lwo'][k]:.6g}")
    assert res["n_used"] == 100 and loo["n_windows"] == 35
    assert res["bin_min_loo_log_sf"] == k and int(np.argmin(res["loo_log_sf"])) == k
    assert res["loo_log_sf"][k] < np.log(0.01 / 35)


# ---- 7. device pointers ----

def _device_check():
    """Body of test_device_pointers, in a process where torch owns the device first (as bench.py)."""
    import torch
    import tamcmc_amd as accel_mod
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    w, y, P = c2_chain(700, 200, 3.0)
    n = len(P)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc, 7) as s:
            L0, st0 = s.push(P)
            host = s.window_loo(P, 20, 7, pit=True)
        acc.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dP = torch.from_numpy(np.ascontiguousarray(P)).to(dev)
        dL = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
        dS = torch.full((n,), -9, dtype=torch.int32, device=dev)
        with capi.Summary(acc, 64) as s:
            s.push_device(n, dP.data_ptr())
            s.wloo_begin(20, 7)
            s.push_device(n, dP.data_ptr())
            assert same_wloo(s.wloo_result(), host)
            s.wloo_pit_begin()
            s.push_device(10, dP.data_ptr(), dL.data_ptr(), dS.data_ptr())   # enqueued, no sync; with and without outputs
            s.push_device(n - 10, dP[10:].data_ptr(), dL[10:].data_ptr(), dS[10:].data_ptr())
            r = s.wloo_pit_result()
            assert same_pit(r, host)
            assert np.array_equal(bits(dL.cpu().numpy()), bits(L0)) and np.array_equal(dS.cpu().numpy(), st0)
            s.wloo_end()
        acc.set_stream(0)
    print("wloo device path ok")


def test_device_pointers():
    in_torch_process("test_summary_wloo_gpu", "_device_check", "wloo device path ok")
