"""Sliding-window predictive scan of a stored chain on the GPU (tamcmc_summary_scan_*, include/tamcmc_accel.h;
tamcmc_scan.hip): the windowed check of tests/test_summary_window_gpu.py at every start position and for several widths at
once, accumulated beside the fold kernel in the pass the user already makes.

Exact checks (no tolerance): position j of width W equals, in all four arrays, the full window starting at bin j of the
disjoint check window=(W, first), for every first = 1 ... W (and at W = 1 the per-bin check, except at p = 3 where the per-bin
check itself forms (3 y) / M and not 3 (y / M): tests/test_summary_window_gpu.py, test 1); the same across the tiles and
halos of the sums kernel on a 5000-bin grid; every width's arrays and totals bit for bit independent of the other widths in
the list, of block_chains -- the chunk edge at 4096 samples inside a block included --, of the split into pushes and of the
order in which the three checks were enabled; the fold, per-bin and windowed results bit for bit the same with the scan on
and off; the scan's results untouched by a quantile, a LOO and an ESS pass and the same after a reset and a second pass;
totals and regions recomputed from the library's own arrays.

Against the reference (tests/scan_reference.py, long double) the rule and the bounds are those of the windowed check
(check_tails_reference in tests/summary_support.py, called as tests/test_summary_window_gpu.py calls it): on the GPU's own rows 10 x the larger of (a) the reference's change under a
2^-50 relative perturbation of the rows and (b) its float64-minus-long-double difference; on the oracle's rows 10 x the
change under a 1e-12 perturbation, the maximum over five seeds; |P + Q - 1| as there.  Every worst ratio is printed before
it is asserted (pytest -s).  At 70 001 samples the reference is evaluated at every sixth position and at both ends -- its
cost is the tails of 70 001 x positions window sums in long double, and the n 2^-52 term under test does not depend on the
position; the bits of all positions are compared between the two block sizes.

Worst ratios observed on an MI355X over all cases below: on the GPU's own rows log_cdf 0.077, pit 0.17, log_sf 0.14,
mean_resid 0.25; at shape 512 8.8e-5, 1.6e-4, 3.2e-4 and 0.12; at 70 001 samples 0.0043, 0.0031, 0.0010 and 0.15; on the
oracle's rows 2.7e-4, 2.5e-4, 2.3e-4 and 6.1e-4.  |P + Q - 1| was 1.1e-14 or less.  The planted case: the disjoint windows'
best log_sf -4.446 (window 18), the best single bin -5.348 (bin 109), the line -8.161, the scan -8.63863 at position 350,
one region, positions 350 ... 351."""

import functools
import itertools

import numpy as np
import pytest

from predictive_reference import predictive_reference
from scan_reference import default_line, regions, scan_reference, scan_totals
from summary_support import (accepted, c2_case, c2_chain, check_pit, check_tails_reference, collect, data_of, edited, edited_chi, open_case,
                             row_groups, same, same_pred, same_scan, same_scans, same_win, sigma_of, spectrum_for, true_model,
                             with_rejected)
from support import bits, pyorc
from tamcmc_amd import capi, synth
from window_reference import window_reference

pytestmark = pytest.mark.gpu

KEYS = capi.Summary.SCAN_ARRAYS
TILE = 2048                                                  # TM_SCAN_TILE: positions per workgroup of the sums kernel
WORST = {}                                                   # tag of the test -> key -> worst ratio seen (printed per case as well)


def widths_for(Nx, like, p, want):
    """`want` cut to the widths that fit the grid and the shape cap."""
    return tuple(W for W in want if W <= Nx and (like != 0 or p * W <= 512))


def run(acc, pushes, block=0, scan=(7,), window=None, predictive=False):
    """A fold pass with the scan on.  Returns (list of scan results per width, fold result, window result or None, predictive
    result or None)."""
    with capi.Summary(acc, block, predictive=predictive, window=window, scan=scan) as s:
        for P in pushes:
            s.push(P)
        return ([s.scan_result(k) for k in range(len(np.atleast_1d(scan)))], s.result(),
                s.window_result() if window is not None else None, s.predictive_result() if predictive else None)


def run_window(acc, pushes, W, first, block=0):
    with capi.Summary(acc, block, window=(W, first)) as s:
        for P in pushes:
            s.push(P)
        return s.window_result()


def check_totals(tag, res, n, n_rejected, Nx, W):
    """The positions as the header defines them; pit from the smaller tail, within 2 ulp; the totals recomputed from the
    library's own arrays: exact."""
    n_pos = Nx - W + 1
    assert res["n_used"] == n and res["n_rejected"] == n_rejected, (tag, res["n_used"], res["n_rejected"])
    assert res["W"] == W and res["n_positions"] == n_pos == len(res["pit"]), tag
    assert np.array_equal(res["first_bin"], np.arange(n_pos)) and np.array_equal(res["last_bin"], np.arange(n_pos) + W - 1), tag
    lc, ls, _ = check_pit(tag, res)
    t = scan_totals(lc, ls)
    for k in ("min_log_sf", "min_log_cdf", "pos_min_log_sf", "pos_min_log_cdf"):
        assert res[k] == t[k], (tag, k, res[k], t[k])


def check_regions(tag, s, k, res, Nx):
    """scan_regions(k) of both sides, at the default line and at two others, against the definition restated in
    tests/scan_reference.py on the library's own arrays: exact."""
    W = res["W"]
    for which, key in ((0, "log_sf"), (1, "log_cdf")):
        for line in (None, -0.5, float(np.median(res[key])) - 1e-9):
            if line is not None and not line < 0:
                continue
            got = s.scan_regions(k, which, line)
            want = regions(res[key], W, Nx, line, res["mean_resid"])
            assert got == want, (tag, which, line, got[:2], want[:2])


def check_reference(tag, res, rows, y, groups, rel, seeds, with_f64, W, like=0, p=1, sigma=None, n_rejected=0, positions=None):
    """res against scan_reference(rows) with the bounds of the module docstring; then the self-check and the totals."""
    reference = functools.partial(scan_reference, W=W, like=like, p=p, sigma=sigma, positions=positions)
    check_tails_reference(reference, "scan", KEYS, tag, res, rows, y, groups, rel, seeds, with_f64, like, p * W, f64_always=True,
                          positions=positions, worst=WORST)
    check_totals(tag, res, len(rows), n_rejected, len(y), W)


def first_for(b, W):
    """The `first` of the disjoint check that has a window start at bin b > 0 (bin 0 starts window 0, full where first = W)."""
    return W if b % W == 0 else b % W


def compare_with_windows(tag, acc, pushes, res, Nx, W, firsts, block=0):
    """Every full window of window=(W, first), first in `firsts`, equals position first_bin of the scan bit for bit in all
    four arrays.  Returns the set of positions compared."""
    seen = set()
    for first in firsts:
        win = run_window(acc, pushes, W, first, block)
        full = np.flatnonzero(win["last_bin"] - win["first_bin"] + 1 == W)
        at = win["first_bin"][full]
        for k in KEYS:
            assert np.array_equal(bits(np.asarray(res[k])[at]), bits(np.asarray(win[k])[full])), (tag, W, first, k)
        assert win["n_used"] == res["n_used"] and win["n_rejected"] == res["n_rejected"], (tag, W, first)
        seen.update(int(b) for b in at)
    return seen


# ---- 1. the scan is the disjoint check at every position ----

@pytest.mark.parametrize("cfg", ["p1", "p3", "chi-square"])
@pytest.mark.parametrize("Nx", [2, 65, 700])
def test_the_scan_is_the_disjoint_check_at_every_position(accel_mod, Nx, cfg):
    """scan=(1, 2, 7, 64) cut to the widths that fit, 37 samples two of which are rejected; for every W and every first =
    1 ... W the disjoint check on the same chain: no tolerance.  At W = 1 the per-bin check as well (not at p = 3: module
    docstring)."""
    w, y0, P35 = c2_chain(Nx, 35)
    P = with_rejected(w, P35, [0, 20])
    y, like, p, sigma = data_of(w, y0, cfg)
    widths = widths_for(Nx, like, p, (1, 2, 7, 64))
    assert widths[:2] == (1, 2)
    with open_case(accel_mod, w, y, cfg) as acc:
        res, _, _, pred = run(acc, [P], 8, scan=widths, predictive=True)
        for k, W in enumerate(widths):
            tag = f"disjoint Nx={Nx} {cfg} W={W}"
            check_totals(tag, res[k], 35, 2, Nx, W)
            seen = compare_with_windows(tag, acc, [P], res[k], Nx, W, range(1, W + 1), 8)
            assert seen == set(range(Nx - W + 1)), (tag, "positions no disjoint window reached", sorted(set(range(Nx - W + 1)) - seen)[:5])
        if cfg != "p3":
            for k in KEYS:
                assert np.array_equal(bits(res[0][k]), bits(pred[k])), (Nx, cfg, "W = 1 against the per-bin check", k)
            assert res[0]["pos_min_log_sf"] == pred["bin_min_log_sf"] and res[0]["pos_min_log_cdf"] == pred["bin_min_log_cdf"]
            assert np.array_equal(bits(float(res[0]["min_log_sf"])), bits(float(pred["min_log_sf"])))


# ---- 2. tile edges and halo ----

def test_tile_edges_and_halo(accel_mod):
    """5000 bins: three tiles of 2048 positions for every width of scan=(7, 100, 512).  W = 100 against all 100 values of
    first; W = 7 and 512 against first = 1, 3, W - 1, W and the values that put a window start on each tile's first position,
    on its last position and W - 1 positions before its end."""
    Nx = 5000
    w, y0, P35 = c2_chain(Nx, 35)
    P = with_rejected(w, P35, [0, 20])
    y = edited_chi(y0)
    widths = (7, 100, 512)
    with open_case(accel_mod, w, y, "p1") as acc:
        res, _, _, _ = run(acc, [P], 16, scan=widths)
        for k, W in enumerate(widths):
            n_pos = Nx - W + 1
            assert -(-n_pos // TILE) >= 3
            check_totals(f"tiles W={W}", res[k], 35, 2, Nx, W)
            if W == 100:
                seen = compare_with_windows("tiles", acc, [P], res[k], Nx, W, range(1, W + 1), 16)
                assert seen == set(range(n_pos))
                continue
            edges = set()
            for t0 in range(0, n_pos, TILE):
                t1 = min(t0 + TILE, n_pos) - 1                                  # the tile's last position
                edges.update((t0, t1, t1 - (W - 1)))
            firsts = {1, 3, W - 1, W} | {first_for(b, W) for b in edges}
            seen = compare_with_windows("tiles", acc, [P], res[k], Nx, W, sorted(firsts), 16)
            assert edges <= seen, (W, sorted(edges - seen))


# ---- 3. the list does not matter ----

@pytest.mark.parametrize("cfg", ["p1", "p3", "chi-square"])
def test_the_list_does_not_matter(accel_mod, cfg):
    """scan=(3, 7, 64) equals scan=3, scan=7 and scan=64 alone, bit for bit, arrays and totals."""
    w, y0, P0 = c2_chain(129, 70)
    P = with_rejected(w, P0, [0, 33, 70])
    y = data_of(w, y0, cfg)[0]
    with open_case(accel_mod, w, y, cfg) as acc:
        together = run(acc, [P], 16, scan=(3, 7, 64))[0]
        assert together[0]["n_used"] == 70 and together[0]["n_rejected"] == 3
        for k, W in enumerate((3, 7, 64)):
            alone = run(acc, [P], 16, scan=W)[0]
            assert len(alone) == 1 and same_scan(alone[0], together[k]), (cfg, W)
        pair = run(acc, [P], 5, scan=(7, 64))[0]
        assert same_scan(pair[0], together[1]) and same_scan(pair[1], together[2]), cfg


# ---- 4. block size and push split ----

@pytest.mark.parametrize("cfg", ["p1", "p3", "chi-square"])
def test_block_size_and_push_split_cannot_change_a_bit(accel_mod, cfg):
    """block_chains 1, 3, 64 and the default, four different splits into pushes: identical bits in every array and total of
    every width; the fold, per-bin and windowed results are those of objects without the scan; the order of the three enables
    changes nothing."""
    w, y0, P0 = c2_chain(129, 70)
    P = with_rejected(w, P0, [0, 33, 70])
    y = data_of(w, y0, cfg)[0]
    widths = (2, 7, 20)
    with open_case(accel_mod, w, y, cfg) as acc:
        first, fold, win, pred = run(acc, [P], 1, scan=widths, window=(7, 3), predictive=True)
        assert first[0]["n_used"] == 70 and first[0]["n_rejected"] == 3
        for B in (3, 64, 0):
            res, f, wi, pr = run(acc, [P], B, scan=widths, window=(7, 3), predictive=True)
            assert same_scans(res, first) and same(f, fold) and same_win(wi, win) and same_pred(pr, pred), ("block_chains", B)
        for cuts in ((1,), (9, 10), (24, 48, 72), tuple(range(1, len(P)))):
            res, f, _, _ = run(acc, np.split(P, cuts), 7, scan=widths)           # (the other checks off: the scan keeps its bits)
            assert same_scans(res, first) and same(f, fold), ("pushes", cuts[:3])
        with capi.Summary(acc, 7, predictive=True, window=(7, 3)) as s:          # the scan off
            s.push(P)
            assert same(s.result(), fold), "the fold results differ with the scan on"
            assert same_pred(s.predictive_result(), pred), "the per-bin check's results differ with the scan on"
            assert same_win(s.window_result(), win), "the windowed check's results differ with the scan on"
        enables = dict(p=lambda s: s.predictive_enable(), w=lambda s: s.window_enable(7, 3), s=lambda s: s.scan_enable(widths))
        for order in itertools.permutations("pws"):
            with capi.Summary(acc, 7) as s:
                for name in order:
                    enables[name](s)
                s.push(P)
                assert same_scans([s.scan_result(k) for k in range(3)], first), order
                assert same_pred(s.predictive_result(), pred) and same_win(s.window_result(), win) and same(s.result(), fold), order


def test_a_chunk_edge_inside_a_block(accel_mod):
    """9000 samples of a 65-bin grid in blocks of 5000 -- chunks of 4096 and 904 samples, then 4000 -- and in blocks of 64: the
    same bits, rejected samples on both sides of the chunk edge."""
    w = synth.workload_c2(Nx=65)
    y = edited_chi(spectrum_for(w))
    P = with_rejected(w, synth.chain_params(w, 8996), [0, 4095, 4096, 8996])
    assert len(P) == 9000
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        small, fold, _, _ = run(acc, [P], 64, scan=(7, 20))
        big, fold_big, _, _ = run(acc, [P], 5000, scan=(7, 20))
    assert small[0]["n_used"] == 8996 and small[0]["n_rejected"] == 4
    assert same_scans(big, small) and same(fold_big, fold)


# ---- 5. other modes and reset ----

def test_other_modes_and_reset_leave_the_state_alone(accel_mod):
    """A quantile pass, a LOO pass and an ESS pass over the same rows on the same object: the scan's results keep their bits
    and can be read inside every mode; scan_enable inside ESS mode is refused; reset keeps the setting and a second pass gives
    the same bits."""
    w, y0, P = c2_chain(129, 70)
    y = edited_chi(y0)
    extra = synth.chain_params(w, 5, seed=4242)

    def results(s):
        return [s.scan_result(k) for k in range(2)]

    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc, 16, scan=(7, 20)) as s:
            s.push(P)
            first = results(s)
            regs = s.scan_regions(1, 0, -0.5)
            assert same_scans(results(s), first), "a second result"
            s.quantiles_begin((0.16, 0.5, 0.84))
            s.push(P)
            assert same_scans(results(s), first), "inside quantile mode, a pass pushed"
            s.quantiles_step()
            s.quantiles_end()
            assert same_scans(results(s), first), "after a quantile pass"
            s.loo_begin()
            s.push(P)
            assert same_scans(results(s), first), "inside LOO mode, a pass pushed"
            s.loo_result()
            s.loo_end()
            assert same_scans(results(s), first), "after a LOO pass"
            s.ess_begin()
            s.push(P)
            assert same_scans(results(s), first) and s.scan_regions(1, 0, -0.5) == regs, "inside ESS mode, a pass pushed"
            s.ess_result()
            s.ess_end()
            assert same_scans(results(s), first), "after an ESS pass"
            s.push(extra)
            after, after_fold = results(s), s.result()
            s.reset()
            r0 = s.scan_result(1)
            assert r0["n_used"] == 0 and r0["n_positions"] == 110 and all(np.all(np.isnan(r0[k])) for k in KEYS)
            assert np.isnan(r0["min_log_sf"]) and r0["pos_min_log_sf"] == -1 and r0["pos_min_log_cdf"] == -1 and s.scan_regions(1) == []
            with pytest.raises(accel_mod.AccelError):
                s.scan_enable((7, 20))                                           # the setting is still on
            s.push(P[:33])
            s.push(P[33:])
            assert same_scans(results(s), first), "a second pass after a reset"
        both, both_fold, _, _ = run(acc, [P, extra], 16, scan=(7, 20))
        assert same_scans(after, both) and same(after_fold, both_fold), "a summary that never entered a mode differs"
        with capi.Summary(acc, 16) as s:                                         # and the modes' results do not depend on the scan
            s.push(P)
            ess_off = s.ess(P)
            s.ess_begin()
            with pytest.raises(accel_mod.AccelError) as e:
                s.scan_enable(7)                                                 # inside ESS mode
            assert e.value.code == capi.E_INVALID
            s.ess_end()
        with capi.Summary(acc, 16, scan=(7, 20)) as s:
            s.push(P)
            ess_on = s.ess(P)
        assert all(np.array_equal(bits(np.asarray(ess_on[k], dtype=np.float64)), bits(np.asarray(ess_off[k], dtype=np.float64)))
                   for k in ("ess_M", "tau_M", "mcse_M", "rhat_M", "ess_l", "r_eff"))


# ---- 6. against the reference ----

CASES = [(2, 1), (7, 37), (65, 200), (700, 37)]


@pytest.mark.parametrize("cfg", ["p1", "p3", "chi-square"])
@pytest.mark.parametrize("Nx,S", CASES)
def test_against_the_reference(accel_mod, Nx, S, cfg):
    """scan=(2, 3, 7, 64) cut to the widths that fit, on the GPU's own rows, with rejected samples among them; totals and
    regions recomputed from the library's own arrays."""
    w, y0, P0 = c2_chain(Nx, S)
    n_bad = 0 if S == 1 else 3
    P = with_rejected(w, P0, [0, S // 2, S]) if n_bad else P0
    y, like, p, sigma = data_of(w, y0, cfg)
    widths = widths_for(Nx, like, p, (2, 3, 7, 64))
    misses = []
    with open_case(accel_mod, w, y, cfg) as acc:
        rows = accepted(acc, P, n_bad)
        with capi.Summary(acc, 16, scan=widths) as s:
            s.push(P)
            for k, W in enumerate(widths):
                res = s.scan_result(k)
                tag = f"gpu-rows Nx={Nx} S={S} {cfg} W={W}"
                collect(check_reference, misses, tag, res, rows, y, np.arange(S), 2.0 ** -50, (1,), True, W, like, p, sigma, n_rejected=n_bad)
                check_regions(tag, s, k, res, Nx)
    print("WORST gpu-rows", WORST.get("gpu-rows"))
    assert not misses, misses


@pytest.mark.parametrize("name,p,W", [("p64-W8", 64, 8), ("p1-W512", 1, 512)])
def test_the_largest_shape(accel_mod, name, p, W):
    """Shape 512 exactly, from p = 64 over 8 bins and from p = 1 over 512: 700 bins, 37 samples."""
    misses = []
    w, y0, P = c2_chain(700, 37)
    y = edited_chi(y0)
    with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=float(p)) as acc:
        rows = accepted(acc, P, 0)
        res = run(acc, [P], 16, scan=W)[0][0]
        collect(check_reference, misses, f"shape-512 {name}", res, rows, y, np.arange(37), 2.0 ** -50, (1,), True, W, 0, p)
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
        res = run(acc, [P], scan=(7, 64, 100))[0]
        for k, W in enumerate((7, 64, 100)):
            collect(check_reference, misses, f"oracle {name} W={W}", res[k], M, y, row_groups(P), 1e-12, (1, 2, 3, 4, 5), False, W, like, p, sigma)
    print("WORST oracle", WORST.get("oracle"))
    assert not misses, misses


# ---- 7. refusals ----

def test_refusals_and_state(accel_mod):
    w, y0, P = c2_chain(65, 9)
    y = edited_chi(y0)
    T = np.ones(len(P))
    E = capi.E_INVALID
    lib = accel_mod.load_library()

    def refused(fn, *a, **k):
        with pytest.raises(accel_mod.AccelError) as e:
            fn(*a, **k)
        assert e.value.code == E

    with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=3.0) as acc:
        with capi.Summary(acc) as s:
            refused(s.scan_enable, ())                                           # n_widths = 0
            refused(s.scan_enable, tuple(range(1, 10)))                          # nine widths
            assert lib.tamcmc_summary_scan_enable(s._s, 2, None) == E            # a NULL list
            refused(s.scan_enable, 0)
            refused(s.scan_enable, -1)
            refused(s.scan_enable, 513)
            refused(s.scan_enable, (7, 66))                                      # above Nx
            refused(s.scan_enable, (7, 7))                                       # not strictly ascending
            refused(s.scan_enable, (8, 7))
            refused(s.scan_enable, (7, 0))
            refused(s.scan_enable, (7, 171))                                     # p W = 513 (and above Nx)
            refused(s.scan_result)                                               # not enabled
            refused(s.scan_regions)
            refused(s.scan_kernel_time)
            refused(capi.Summary, acc, 0, scan=(7, 7))
            s.scan_enable((7, 65))                                               # the object is as it was: the enable goes through
            s.push(P)
            check_totals("after the refusals W=7", s.scan_result(0), 9, 0, 65, 7)
            check_totals("after the refusals W=65", s.scan_result(1), 9, 0, 65, 65)
    with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=64.0) as acc:
        with capi.Summary(acc) as s:
            refused(s.scan_enable, (2, 9))                                       # p W = 576
            s.scan_enable((2, 8))                                                # p W = 512
    for p in (0.0, 0.9, 513.0):                                                  # chi(2,2p) with p < 1, or p alone past the shape
        with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=p) as acc:
            with capi.Summary(acc) as s:
                refused(s.scan_enable, 1)
    with accel_mod.Accel(2, w["plength"], w["x"], y, sigma_y=sigma_of(65), likelihood_case=1, likelihood_p=0.0) as acc:
        with capi.Summary(acc, scan=65) as s:                                    # chi_square does not look at p
            s.push(P)
            assert s.scan_result()["n_used"] == 9 and s.scan_result()["n_positions"] == 1
    acc = accel_mod.Accel(2, w["plength"], w["x"], y)
    s = capi.Summary(acc, 4)
    s.push(P[:3])
    refused(s.scan_enable, 7)                                                    # after a push
    s.quantiles_begin((0.5,))
    refused(s.scan_enable, 7)                                                    # in quantile mode
    s.quantiles_end()
    s.loo_begin()
    refused(s.scan_enable, 7)                                                    # in LOO mode
    s.reset()
    acc.begin(P, T)                                                              # a batch in flight
    refused(s.scan_enable, 7)
    acc.end()
    acc.arm(len(P))                                                              # a batch armed
    refused(s.scan_enable, 7)
    acc.disarm()
    s.scan_enable((7, 20))                                                       # after a reset: allowed
    refused(s.scan_enable, (7, 20))                                              # twice
    refused(s.scan_enable, 8)
    r0 = s.scan_result(0)                                                        # n = 0: everything is NaN
    assert r0["n_used"] == 0 and r0["n_rejected"] == 0 and r0["n_positions"] == 59 and all(np.all(np.isnan(r0[k])) for k in KEYS)
    assert np.isnan(r0["min_log_sf"]) and np.isnan(r0["min_log_cdf"]) and r0["pos_min_log_sf"] == -1 and r0["pos_min_log_cdf"] == -1
    assert s.scan_regions(0) == [] and s.scan_regions(1, 1, -1e-3) == []
    s.push(P)
    full = [s.scan_result(0), s.scan_result(1)]
    check_totals("refusals", full[0], 9, 0, 65, 7)
    refused(s.scan_result, 2)                                                    # k out of range
    refused(s.scan_result, -1)
    refused(s.scan_regions, 2)
    refused(s.scan_regions, -1)
    refused(s.scan_regions, 0, 2)                                                # which outside 0 ... 1
    refused(s.scan_regions, 0, -1)
    refused(s.scan_regions, 0, 0, 0.0)                                           # log_below >= 0
    refused(s.scan_regions, 0, 0, 1.5)
    refused(s.scan_regions, 0, 0, float("inf"))
    # max_regions smaller than the count: the count is still returned, and the first records are filled
    for line in np.sort(full[0]["log_sf"][np.isfinite(full[0]["log_sf"])])[::-1]:  # the highest line with two or more regions
        want = regions(full[0]["log_sf"], 7, 65, float(line), full[0]["mean_resid"]) if line < 0 else []
        if len(want) >= 2:
            break
    line = float(line)
    assert len(want) >= 2 and s.scan_regions(0, 0, line) == want
    buf = (capi.SummaryScanRegion * 3)()
    for r in buf:
        r.pos_first = -77
    n = capi.C.c_int32(-1)
    assert lib.tamcmc_summary_scan_regions(s._s, 0, 0, line, 1, buf, capi.C.byref(n)) == 0 and n.value == len(want)
    assert {k: (getattr(buf[0], k)) for k in capi.Summary.SCAN_REGION} == want[0] and buf[1].pos_first == -77
    assert lib.tamcmc_summary_scan_regions(s._s, 0, 0, line, 0, None, capi.C.byref(n)) == 0 and n.value == len(want)
    assert lib.tamcmc_summary_scan_regions(s._s, 0, 0, line, 1, None, capi.C.byref(n)) == E     # room promised, none given
    assert lib.tamcmc_summary_scan_regions(s._s, 0, 0, line, -1, buf, capi.C.byref(n)) == E
    assert lib.tamcmc_summary_scan_regions(s._s, 0, 0, line, 0, None, None) == E
    # NULL arrays and totals are accepted
    assert lib.tamcmc_summary_scan_result(s._s, 1, None, None, None, None, None) == 0
    only = np.empty(46)
    assert lib.tamcmc_summary_scan_result(s._s, 1, None, None, None, capi._dptr(only), None) == 0
    assert np.array_equal(bits(only), bits(full[1]["log_sf"]))
    acc.begin(P, T)
    refused(s.scan_result)                                                       # a batch in flight
    refused(s.scan_regions)
    acc.end()
    assert same_scans([s.scan_result(0), s.scan_result(1)], full), "a refused call touched the state"
    s.profile(True)                                                              # the getter: one event pair per block
    s.reset()
    s.push(P)
    ms_f, n_f = s.kernel_time()
    ms_s, n_s = s.scan_kernel_time()
    s.profile(False)
    assert n_f == 3 and n_s == 3 and ms_f > 0.0 and ms_s > 0.0
    assert same_scans([s.scan_result(0), s.scan_result(1)], full), "with the timers on"
    refused(acc.close)                                                           # a live summary holds the context
    s.close()
    acc.close()


# ---- 8. what it is for ----

PLANTED = dict(seed=2, first_bin=350, bins=20)


def test_a_feature_the_disjoint_windows_cut(accel_mod):
    """700 bins of y = M e with exponential e, M the model at the generating parameters; in bins 350 ... 369 y = 2 M instead.
    The disjoint windows of W = 20, first = 0 cut the feature at bin 360.  On the reference alone: neither the disjoint
    windows nor the single bins cross the Bonferroni line log(0.01 20 / 700) = -8.16, the scan has its minimum at position
    350, and its positions below the line form one run inside 331 ... 369.  Then the library, in one pass."""
    Nx, W = 700, 20
    w = synth.workload_c2(Nx=Nx)
    M0 = true_model(w)
    y = M0 * np.random.default_rng(PLANTED["seed"]).exponential(size=Nx)
    b0, b1 = PLANTED["first_bin"], PLANTED["first_bin"] + PLANTED["bins"]
    y[b0:b1] = 2.0 * M0[b0:b1]
    P = synth.chain_params(w, 100, scale=0.05)
    _, rst, M = pyorc().generate_batch(2, w["plength"], w["x"], y, P, np.ones(100), want_models=True)
    assert np.all(rst == 0)
    line = default_line(W, Nx)
    ref_w, ref_b, ref_s = window_reference(M, y, W), predictive_reference(M, y), scan_reference(M, y, W)
    runs = regions(ref_s["log_sf"], W, Nx)
    print(f"PLANTED line {line:.4g}; disjoint windows: best log_sf {float(ref_w['log_sf'].min()):.4g} (window {int(np.argmin(ref_w['log_sf']))}); "
          f"per bin: best {float(ref_b['log_sf'].min()):.4g} (bin {int(np.argmin(ref_b['log_sf']))}); scan: {float(ref_s['log_sf'].min()):.6g} at "
          f"position {int(np.argmin(ref_s['log_sf']))}, runs below the line {[(r['pos_first'], r['pos_last']) for r in runs]}")
    assert not np.any(ref_w["log_sf"] < line), "set-up error: choose another seed"
    assert not np.any(ref_b["log_sf"] < line), "set-up error: choose another seed"
    assert int(np.argmin(ref_s["log_sf"])) == b0, "set-up error: choose another seed"
    assert len(runs) == 1 and 331 <= runs[0]["pos_first"] <= runs[0]["pos_last"] <= 369, "set-up error: choose another seed"
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc, scan=(10, 20, 40), window=W, predictive=True) as s:
            s.push(P)
            res, found, win = s.scan_result(1), s.scan_regions(1), s.window_result()
    assert res["W"] == W and res["pos_min_log_sf"] == b0
    assert abs(res["min_log_sf"] - float(ref_s["log_sf"][b0])) < 1e-9 * abs(res["min_log_sf"])
    assert len(found) == 1
    r = found[0]
    assert r["pos_first"] <= b0 <= r["pos_last"] and r["pos_min"] == b0 and r["min_log"] == res["min_log_sf"]
    assert 331 <= r["bin_first"] and r["bin_last"] <= 388 and r["bin_first"] <= b0 and r["bin_last"] >= b1 - 1
    assert win["min_log_sf"] > line


# ---- 9. at length ----

def test_at_length(accel_mod):
    """70 001 samples of a 65-bin grid, scan=(7,), in blocks of 64 and in one block of 70 001 -- 18 chunks --: the same bits,
    and the n 2^-52 accumulation of the two running sums within the bound (the reference at every sixth position and at both
    ends: module docstring)."""
    S = 70001
    w = synth.workload_c2(Nx=65)
    y = edited_chi(spectrum_for(w))
    P = synth.chain_params(w, S)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        rows = accepted(acc, P, 0)
        res, fold, _, _ = run(acc, [P], 64, scan=(7,))
        one, fold1, _, _ = run(acc, [P], S, scan=(7,))
    assert same_scans(one, res) and same(fold1, fold)
    positions = sorted(set(range(0, 59, 6)) | {58})
    check_reference("at-length", res[0], rows, y, np.arange(S), 2.0 ** -50, (1,), True, 7, positions=positions)
