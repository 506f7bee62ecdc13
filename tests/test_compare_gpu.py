"""The comparison of fits on the GPU (tamcmc_compare_*, include/tamcmc_accel_compare.h; tamcmc_compare.hip) against the
independent long-double restatement of tests/compare_reference.py.

1. variates     variates(r) against the long-double reference from the same uniforms, within the bound tests/test_scan_null_gpu.py
                uses for the chi(2,2p) p = 1 variate (10 x 1.5 x 2^-52 e: the same -log u).
2. bootstrap    N in {1, 2, 63, 64, 65, T - 1, T, T + 1, 2 T + 1} (T the bootstrap tile), K in {2, 3, 8}, R in {1, 2, 5}, excluded units
                first, last, on a tile edge and a whole tile of them.  Bit for bit: z does not depend on scratch_bytes (chunks of
                1, 2 and 3 replicates), on the split of R over calls (5 = 2 + 3 = 1 + 1 + 3) or on first_replicate.  Against long
                double: z recomputed from the library's own variates and from the reference's stays within 10 x its first-order
                sensitivity to a relative 2^-50 change of every e_i and D_k,i; the worst ratio is printed (pytest -s).
3. symmetry     a duplicated fit has z_1 == z_2 and equal weights from all three methods; identical fits give z = 0, weights
                1 / K, elpd_diff = se_diff = 0.
4. counting     diff equals the long-double totals; prob, interval and the pseudo-BMA(+) weights equal the header's rules applied
                to the library's own z.
5. moments      the fixed case of the issue: E z = elpd_diff and Var z = N' S / (N' + 1) within 6 standard errors.
6. stacking     g recomputed in long double from the returned w: max g - 1 <= tol + 10 x the sensitivity of g; for K = 2
                f* - f(w) <= gap with f* by bisection; independent of scratch_bytes and of the cadence of the host's looks; a fit
                0.01 worse in every unit ends below 1e-6; max_iter = 3 returns converged = 0 with the true gap.
7. refusals     on a live object, and with N' = 0.
8. planted      2000 bins, a chain about the truth against the same chain with one mode's height taken to nearly zero:
                Summary.loo and window_loo(W = 20) for both, Compare.from_loo: elpd_diff positive by many se_diff, every weight
                method gives the true fit more than 0.99, the units of largest d lie in the removed mode's truncation window."""
import numpy as np
import pytest

import compare_reference as CR
from summary_support import true_model
from support import bits
from tamcmc_amd import capi, synth

pytestmark = pytest.mark.gpu

LD = np.longdouble
T = capi.COMPARE_TILE
ST = capi.COMPARE_STACK_TILE
E_INVALID = capi.E_INVALID


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def make_case(K, N, seed=1, exclude=True):
    """elpd (K, N) and pareto_k: a common part and fit-wise scatter with heavy tails; excluded units (NaN, +inf, -inf in
    different fits) first, last, on either side of the first tile edge, and the whole second tile where there is one."""
    rng = np.random.default_rng(1000 * K + N + seed)
    elpd = rng.normal(-3.0, 1.0, N)[None, :] + 0.3 * rng.standard_t(5, (K, N)) + 0.02 * np.arange(K)[:, None]
    kh = rng.uniform(-0.2, 1.0, (K, N))
    if exclude and N >= 63:
        bad = [0, N - 1, 31] + ([T - 1, T] if N > T else []) + (list(range(T, 2 * T)) if N > 2 * T else [])
        for j, i in enumerate(bad):
            elpd[j % K, i] = (np.nan, np.inf, -np.inf)[j % 3]
    return elpd, kh


def per_replicate_bytes(K, N):
    tiles = (N + T - 1) // T
    return tiles * K * 8 + (K - 1) * 8


def all_z(cmp):
    return np.stack([cmp.z(k) for k in range(cmp.K)], axis=1)


# ---- 1. variates ----

def test_variates_against_long_double(accel_mod):
    N = 3001
    elpd = np.zeros((2, N))
    elpd[1, 5] = np.nan                                                       # (an excluded unit has its variate all the same)
    worst = 0.0
    for seed, first, reps in ((3, 0, (0, 1, 5)), (0x9E3779B97F4A7C15, 1000, (1,)), (17, (1 << 33) - 3, (0, 1, 2, 3))):
        with accel_mod.Compare(elpd, seed=seed, first_replicate=first) as cmp:
            for r in reps:
                got = cmp.variates(r)
                want, sens = CR.variates(N, seed, first + r)
                assert np.all(np.isfinite(got)) and np.all(got > 0) and np.all(sens > 0)
                ratio = float(np.max(np.abs(got.astype(LD) - want) / (10.0 * sens)))
                worst = max(worst, ratio)
                print(f"RATIO compare variates seed={seed:#x} replicate={first + r}: {ratio:.3g}")
    assert worst <= 1.0, worst


# ---- 2. bootstrap: bit for bit, and against long double ----

SIZES = (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)
WORST = {}


@pytest.mark.parametrize("K", (2, 3, 8))
@pytest.mark.parametrize("N", SIZES)
def test_bootstrap_bits_and_long_double(accel_mod, N, K):
    elpd, kh = make_case(K, N)
    seed, R = 77 + N, 5
    per = per_replicate_bytes(K, N)
    with accel_mod.Compare(elpd, kh, seed=seed) as cmp:
        assert cmp.n_included == int(CR.included(elpd).sum()) and cmp.n_excluded == N - cmp.n_included and cmp.n_included >= 1
        assert cmp.bootstrap(R) == R
        z = all_z(cmp)
        e_lib = [cmp.variates(r) for r in range(R)]
        assert z.shape == (R, K) and np.all(z[:, 0] == 0) and np.all(np.isfinite(z))
    # chunks of 1, 2 and 3 replicates; R = 1, 2, 5 over calls: 5 = 2 + 3 = 1 + 1 + 3
    for chunk in (1, 2, 3):
        with accel_mod.Compare(elpd, seed=seed) as cmp:
            cmp.bootstrap(R, scratch_bytes=chunk * per)
            assert same_bits(all_z(cmp), z), ("chunk", chunk)
    for split, scratch in (((2, 3), 0), ((1, 1, 3), 0), ((1, 1, 3), 2 * per)):
        with accel_mod.Compare(elpd, seed=seed) as cmp:
            done = 0
            for n in split:
                done += n
                assert cmp.bootstrap(n, scratch_bytes=scratch) == done
                assert same_bits(all_z(cmp), z[:done]), ("split", split, done)
    with accel_mod.Compare(elpd, seed=seed, first_replicate=3) as cmp:
        cmp.bootstrap(2)
        assert same_bits(all_z(cmp), z[3:]) and same_bits(cmp.variates(1), e_lib[4])
    with accel_mod.Compare(elpd, seed=seed + 1) as cmp:
        cmp.bootstrap(1)
        assert N == 1 or not np.array_equal(all_z(cmp)[0], z[0])               # (one unit: z = D whatever the variate)
    # long double, from the library's variates and from the reference's
    worst = 0.0
    for r in range(R):
        for e in (e_lib[r], CR.variates(N, seed, r)[0]):
            want, sens = CR.z_ld(e, elpd)
            err = np.abs(z[r, 1:].astype(LD) - want)
            assert np.all(err <= 10.0 * sens), (N, K, r, err, sens)
            worst = max(worst, float(np.max(err[sens > 0] / (10.0 * sens[sens > 0]))) if np.any(sens > 0) else 0.0)
    WORST[(N, K)] = worst
    print(f"RATIO compare z N={N} K={K}: worst {worst:.3g} of 10 x sensitivity (all so far {max(WORST.values()):.3g})")


# ---- 3. symmetry ----

def test_duplicated_and_identical_fits(accel_mod):
    base, _ = make_case(2, 2 * T + 1, seed=9)
    dup = np.stack([base[0], base[1], base[1]])
    with accel_mod.Compare(dup, seed=5) as cmp:
        cmp.bootstrap(7)
        assert same_bits(cmp.z(1), cmp.z(2)) and cmp.prob(1, 2) == (0, 7, 7) and cmp.interval(1, 2, 0.5) == 0.0
        st = cmp.stacking(1e-8, 5000)
        for method in ("pseudo_bma", "pseudo_bma_plus", "stacking"):
            w = cmp.weights(method)
            assert same_bits(w[1], w[2]) and abs(w.sum() - 1.0) < 1e-10, (method, w)
        assert same_bits(st["w"], cmp.weights("stacking")) and st["iterations"] >= 1
        d = cmp.diff(1, 2)
        assert d["elpd_diff"] == 0.0 and d["se_diff"] == 0.0 and d["n_better"] == 0 and d["n_worse"] == 0
    for K in (2, 3, 8):
        same = np.tile(base[0], (K, 1))
        with accel_mod.Compare(same, seed=5) as cmp:
            cmp.bootstrap(3)
            assert np.all(all_z(cmp) == 0.0)
            st = cmp.stacking(0.0, 50)
            assert st["iterations"] == 1 and st["converged"] == 1 and st["gap"] == 0.0 and st["f"] == 0.0
            for method in ("pseudo_bma", "pseudo_bma_plus", "stacking"):
                assert np.all(cmp.weights(method) == 1.0 / K), (K, method)
            d = cmp.diff(K - 1, 0)
            assert d["elpd_diff"] == 0.0 and d["se_diff"] == 0.0 and d["n_included"] == cmp.n_included


# ---- 4. counting ----

def test_totals_and_counting_rules(accel_mod):
    K, N, R, s = 3, 501, 200, 0.5
    elpd, kh = make_case(K, N, seed=4)
    kh[0, 7], kh[1, 7], kh[2, 9], kh[0, 11] = np.nan, np.inf, np.nan, 0.7
    with accel_mod.Compare(elpd, kh, scale=s, seed=8) as cmp:
        for a in range(K):
            for b in range(K):
                got, want = cmp.diff(a, b), CR.pair_totals(elpd, kh, a, b)
                for key in ("n_included", "n_excluded", "n_better", "n_worse", "n_k_high"):
                    assert got[key] == want[key], (a, b, key)
                with np.errstate(invalid="ignore"):
                    dab = elpd[a] - elpd[b]
                room = 2.0 ** -60 * float(np.abs(dab[np.isfinite(dab)]).sum())
                for key in ("elpd_diff", "se_diff", "diff_k_high"):
                    assert abs(got[key] - want[key]) <= 4 * 2.0 ** -52 * abs(want[key]) + room, (a, b, key, got[key], want[key])
        with accel_mod.Compare(elpd, None, scale=s) as plain:
            d = plain.diff(1, 0)
            assert d["n_k_high"] == -1 and np.isnan(d["diff_k_high"]) and d["elpd_diff"] == cmp.diff(1, 0)["elpd_diff"]
        cmp.bootstrap(R)
        z = all_z(cmp)
        for a in range(K):
            for b in range(K):
                assert cmp.prob(a, b) == CR.prob(z[:, a], z[:, b]) + (R,)
                for q in (0.0, 0.05, 0.5, 0.95, 0.999, 1.0):
                    assert cmp.interval(a, b, q) == CR.interval(z[:, a], z[:, b], q), (a, b, q)
        want = np.asarray(CR.bma_plus(z, s), dtype=np.float64)
        got = cmp.weights("pseudo_bma_plus")
        assert np.all(np.abs(got - want) <= 1e-14) and abs(got.sum() - 1.0) < 1e-14
        diffs = [0.0] + [cmp.diff(k, 0)["elpd_diff"] for k in range(1, K)]
        want = np.asarray(CR.softmax(s * np.array(diffs)), dtype=np.float64)
        assert np.all(np.abs(cmp.weights("pseudo_bma") - want) <= 1e-14)


# ---- 5. moments ----

def test_bootstrap_moments(accel_mod):
    elpd, R, seed = CR.moments_case()
    with accel_mod.Compare(elpd, seed=seed) as cmp:
        cmp.bootstrap(R)
        z = cmp.z(1)
        assert cmp.diff(1, 0)["elpd_diff"] == float(elpd[1].astype(LD).sum())
    t_mean, t_var = CR.moments_check(z, elpd[1])
    print(f"MOMENTS library: mean {t_mean:+.3f} se, variance {t_var:+.3f} se")
    assert abs(t_mean) <= 6.0 and abs(t_var) <= 6.0


# ---- 6. stacking ----

def check_stacking(tag, elpd, s, st, tol):
    """The returned state against long double: the true gap at the returned w, the reported gap and f."""
    P = CR.stack_P(elpd, s)
    g, sens, f = CR.stack_g(st["w"], P)
    gap = float(np.max(g) - 1)
    slack = 10.0 * float(np.max(sens))
    f_slack = 10.0 * 2.0 ** -50 * (1.0 + float(np.abs(np.log((np.asarray(st["w"], dtype=LD)[:, None] * P).sum(axis=0))).mean()))
    print(f"STACKING {tag}: iterations {st['iterations']} converged {st['converged']} gap {st['gap']:.3e} (long double {gap:.3e}, "
          f"slack {slack:.1e}) f {st['f']:.6g} w {st['w']}")
    assert abs(st["gap"] - gap) <= slack and abs(st["f"] - float(f)) <= f_slack, (tag, st, gap, float(f))
    assert abs(float(np.sum(st["w"].astype(LD))) - 1.0) <= 1e-12 * max(st["iterations"], 1) and np.all(st["w"] >= 0)
    if st["converged"]:
        assert gap <= tol + slack, (tag, gap, tol, slack)
    return P, gap, f


@pytest.mark.parametrize("K", (2, 3, 8))
@pytest.mark.parametrize("N", (1, 65, ST + 1, 2 * ST + 1))
def test_stacking_against_long_double(accel_mod, N, K):
    elpd, _ = make_case(K, N, seed=3)
    if N > ST:
        elpd[1, ST - 1:ST + 1] = np.nan                                        # the stacking tile's edge
    tol, s, most = 1e-8, 1.0, 5000
    with accel_mod.Compare(elpd, scale=s) as cmp:
        st = cmp.stacking(tol, most)
        assert st["table"] == 1 and 1 <= st["iterations"] <= most and (st["converged"] == 1 or st["iterations"] == most)
        P, gap, f = check_stacking(f"N={N} K={K}", elpd, s, st, tol)
        if K == 2:
            fstar = CR.stack_optimum_2(P)
            assert -1e-15 <= fstar - f <= gap, (float(fstar), float(f), gap)
        # no bit depends on the table of P or on how often the host looks
        for scratch, cadence in ((1, None), (0, 1), (1, 3), (0, 4096)):
            other = cmp.stacking(tol, most, scratch_bytes=scratch, cadence=cadence)
            assert other["table"] == (0 if scratch else 1)
            assert same_bits(other["w"], st["w"]) and same_bits([other["gap"], other["f"]], [st["gap"], st["f"]]), (scratch, cadence)
            assert (other["iterations"], other["converged"]) == (st["iterations"], st["converged"])
        # max_iter = 3: not converged (unless it was within three), and the gap is that of the returned w
        few = cmp.stacking(tol, 3)
        if st["iterations"] > 3:
            assert few["iterations"] == 3 and few["converged"] == 0 and few["gap"] > tol
        check_stacking(f"N={N} K={K} max_iter=3", elpd, s, few, tol)


def test_stacking_drops_a_dominated_fit(accel_mod):
    base, _ = make_case(2, 3001, seed=6)
    for K, worse in ((2, 1), (3, 2)):
        elpd = np.stack([base[k] for k in range(K - 1)] + [base[0] - 0.01])
        with accel_mod.Compare(elpd) as cmp:
            st = cmp.stacking(1e-9, 100000)
            check_stacking(f"dominated K={K}", elpd, 1.0, st, 1e-9)
            assert st["converged"] == 1 and st["w"][worse] < 1e-6, st
            few = cmp.stacking(1e-9, 3)
            assert few["iterations"] == 3 and few["converged"] == 0 and few["gap"] > 1e-9
            check_stacking(f"dominated K={K} max_iter=3", elpd, 1.0, few, 1e-9)
            assert same_bits(cmp.weights("stacking"), few["w"])


def test_stacking_scale(accel_mod):
    """chi_square's convention: scale 0.5 is the stacking of half the values at scale 1."""
    elpd, _ = make_case(3, 700, seed=2)
    with accel_mod.Compare(elpd, scale=0.5) as a, accel_mod.Compare(0.5 * elpd, scale=1.0) as b:
        sa, sb = a.stacking(1e-8, 5000), b.stacking(1e-8, 5000)
        check_stacking("scale 0.5", elpd, 0.5, sa, 1e-8)
        assert sa["iterations"] == sb["iterations"] and np.all(np.abs(sa["w"] - sb["w"]) <= 1e-12)


# ---- 7. refusals ----

def test_refusals_on_a_live_object(accel_mod):
    lib = accel_mod.load_library()
    elpd, kh = make_case(3, 100, seed=1, exclude=False)
    w = np.empty(8)
    with accel_mod.Compare(elpd, kh) as cmp:
        def refused(fn, *a, **k):
            try:
                fn(*a, **k)
            except accel_mod.AccelError as e:
                return e.code == E_INVALID
            return False

        for a, b in ((-1, 0), (0, 3), (3, 3)):
            assert refused(cmp.diff, a, b)
        assert refused(cmp.weights, "pseudo_bma_plus") and refused(cmp.weights, "stacking") and refused(cmp.weights, 3)
        assert refused(cmp.prob, 1, 0) and refused(cmp.interval, 1, 0, 0.5)
        assert refused(cmp.bootstrap, 0) and refused(cmp.bootstrap, -1) and refused(cmp.bootstrap, 5, scratch_bytes=-1)
        assert refused(cmp.bootstrap, (1 << 24) + 1)
        assert cmp.bootstrap(2) == 2 and refused(cmp.bootstrap, (1 << 24) - 1) and cmp.replicates == 2
        assert refused(cmp.z, 3) and refused(cmp.z, -1) and refused(cmp.prob, 0, 3)
        for q in (-0.01, 1.01, float("nan")):
            assert refused(cmp.interval, 1, 0, q)
        for tol, it, scratch in ((-1e-9, 10, 0), (float("nan"), 10, 0), (float("inf"), 10, 0), (1e-8, 0, 0), (1e-8, (1 << 24) + 1, 0), (1e-8, 10, -1)):
            assert refused(cmp.stacking, tol, it, scratch)
        assert refused(cmp.stacking, 1e-8, 10, cadence=0) and refused(cmp.stacking, 1e-8, 10, cadence=4097)
        assert refused(cmp.variates, -1) and refused(cmp.kernel_time, 2)
        assert lib.tamcmc_compare_weights(cmp._h, 0, None) == E_INVALID and lib.tamcmc_compare_stacking(cmp._h, 1e-8, 10, 0, None, None) == E_INVALID
        assert cmp.weights("pseudo_bma").shape == (3,)
    # no included unit: NaN totals, bootstrap and stacking refused
    none = np.array([[1.0, np.nan, 3.0], [np.inf, 2.0, -np.inf]])
    with accel_mod.Compare(none) as cmp:
        d = cmp.diff(1, 0)
        assert (cmp.n_included, cmp.n_excluded, d["n_included"], d["n_excluded"]) == (0, 3, 0, 3)
        assert np.isnan(d["elpd_diff"]) and np.isnan(d["se_diff"]) and np.isnan(d["diff_k_high"]) and d["n_better"] == 0
        for fn, args in ((cmp.bootstrap, (3,)), (cmp.stacking, (1e-8, 10)), (cmp.weights, ("pseudo_bma",))):
            try:
                fn(*args)
            except accel_mod.AccelError as e:
                assert e.code == E_INVALID
            else:
                raise AssertionError("taken with no included unit")
        assert cmp.variates(0).shape == (3,)


def test_profile_counts_launches(accel_mod):
    elpd, _ = make_case(2, 2 * T + 1, seed=1)
    with accel_mod.Compare(elpd) as cmp:
        cmp.profile(True)
        cmp.bootstrap(5, scratch_bytes=2 * per_replicate_bytes(2, 2 * T + 1))
        ms, n = cmp.kernel_time(0)
        assert n == 3 and ms > 0.0
        st = cmp.stacking(1e-9, 40, cadence=8)
        ms, n = cmp.kernel_time(1)
        assert n == 1 + (min(st["iterations"], 40) + 7) // 8 and ms > 0.0
        cmp.profile(False)
        assert cmp.kernel_time(0) == (0.0, 0)


# ---- 8. planted case, end to end ----

def test_planted_missing_mode(accel_mod):
    """2000 bins around the l = 2 mode at 2313.13 muHz (truncation at 3 widths), its height 20 times the catalogue's.  Fit A:
    100 rows scattered about the truth; fit B: the same rows with Height_l[0] at 1e-6, which removes that mode (the l = 0 and
    l = 1 modes of the same order lie outside the grid)."""
    Nx, W = 2000, 20
    w = synth.workload_c2(Nx=Nx, trunc_c=3.0)
    w["params_true"][0] *= 20.0
    y = synth.make_spectrum(true_model(w), seed=17)
    PA = synth.chain_params(w, 100, scale=0.05)
    PB = PA.copy()
    PB[:, 0] = 1e-6
    loo, lwo = [], []
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        for P in (PA, PB):
            with capi.Summary(acc) as s:
                s.push(P)
                loo.append(s.loo(P))
                lwo.append(s.window_loo(P, W))
        with capi.ModeTable(acc) as mt:
            cols = mt.columns()
            row, status = mt.derive(w["params_true"][None, :])
    assert status[0] == 0
    names = np.array([capi.ModeTable.KINDS[k] for k in cols["kind"]])
    mine = np.flatnonzero((names == "freq") & (cols["l"] == 2) & (np.abs(row[0] - 2313.12988) < 1e-6))
    assert mine.size == 1
    mult = cols["mult"][mine[0]]
    lo = int(row[0][(names == "window_lo") & (cols["mult"] == mult)][0])      # [lo, hi) in bins
    hi = int(row[0][(names == "window_hi") & (cols["mult"] == mult)][0])
    assert 0 < lo < hi <= Nx                                                 # (bins below lo lie outside the window)
    for tag, res, first, last in (("bins", loo, np.arange(Nx), np.arange(Nx)), ("windows", lwo, lwo[0]["first_bin"], lwo[0]["last_bin"])):
        with accel_mod.Compare.from_loo(*res, seed=1) as cmp:
            assert cmp.K == 2 and cmp.N == (Nx if tag == "bins" else Nx // W) and cmp.n_excluded == 0
            d = cmp.diff(0, 1)
            cmp.bootstrap(2000)
            st = cmp.stacking(1e-9, 100000)
            wts = {m: cmp.weights(m) for m in ("pseudo_bma", "pseudo_bma_plus", "stacking")}
            gt, eq, R = cmp.prob(0, 1)
            key = "elpd_loo" if tag == "bins" else "elpd_lwo"
            di = res[0][key] - res[1][key]
            top = np.argsort(-np.abs(di), kind="stable")[:20 if tag == "bins" else 3]
            print(f"PLANTED {tag}: elpd_diff {d['elpd_diff']:.6g} se_diff {d['se_diff']:.6g} ({d['elpd_diff'] / d['se_diff']:.3g} se) n_k_high {d['n_k_high']} "
                  f"diff_k_high {d['diff_k_high']:.4g} prob {gt}/{R} interval [{cmp.interval(0, 1, 0.05):.6g}, {cmp.interval(0, 1, 0.95):.6g}] "
                  f"weights of A {[float(v[0]) for v in wts.values()]} stacking {st['iterations']} iterations, top units {top.min()}..{top.max()}, "
                  f"window bins {lo}..{hi - 1}")
            assert d["elpd_diff"] > 5.0 * d["se_diff"] > 0 and d["n_included"] == cmp.N
            assert gt == R and eq == 0 and cmp.interval(0, 1, 0.05) > 0
            for m, v in wts.items():
                assert v[0] > 0.99 and abs(v.sum() - 1.0) < 1e-9, (tag, m, v)
            assert np.all(last[top] >= lo) and np.all(first[top] < hi), (tag, top)
