"""Monte-Carlo null of the scan on the GPU (tamcmc_scan_null_*, include/tamcmc_accel.h; tamcmc_scan_null.hip) against the
independent numpy restatement of tests/scan_null_reference.py.

1. variates     variates(r) against the long-double reference from the same uniforms, within 10 x the sensitivity derived in
                the reference file; the worst ratio is printed (pytest -s) before it is asserted.
2. extremes     from the device's own variates, float64 sliding sums in ascending order with argmax / argmin taking the first
                position give ext_sum and pos bit for bit, both sides, over the grids and widths at which the kernel takes
                another path: one tile, a tile and a bin, the halo ending in and past the last tile, one position, K = 1 and 8.
3. min_log      against scipy's gamma.logsf / logcdf and norm with scale sqrt(1/2), within the bar tamcmc_window.h states for
                the shape, relative to max(1, |value|).
4. independence replicate r has the same bits in runs of 1, 7 and 50, across run calls split any way, whichever other widths
                are in the list, and in an object created at first_replicate = r.
4b. long grid   131 073 bins, eight widths: 65 tiles, and replicate chunks of 4032 set by the 64 MiB of partials, not by the cap of
                4096; variates, extremes and split independence across that chunk edge.
5. distribution Kolmogorov distance to the exact law below 1.63 / sqrt(R), R = 2000, seed 3, in three cases.
6. calibration  line and pvalue equal the counting rule restated in numpy on the returned min_log, exactly; joint <= per-width
                <= the library's default line at Nx = 5000, widths (10, 20, 40), p = 1, R = 1000, seed 3.
7. with a chain a planted run of 20 bins at least 3 below the joint line is the one region of scan_regions(log_below =
                null.line(...)), with p_joint = 1 / (R + 1); a ScanNull alive on the device changes no bit of a summary."""
import numpy as np
import pytest

import scan_null_reference as R
from summary_support import same, same_pred, same_scans, same_win, true_model
from support import bits
from tamcmc_amd import capi, synth

pytestmark = pytest.mark.gpu

def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def null_results(null):
    return [[null.result(k, which) for which in (0, 1)] for k in range(len(null.widths))]


def same_results(a, b):
    """two lists over widths of (side 0, side 1) result dicts, bit for bit"""
    return len(a) == len(b) and all(same_bits(x[s][key], y[s][key]) and np.array_equal(x[s]["pos"], y[s]["pos"])
                                    for x, y in zip(a, b) for s in (0, 1) for key in ("ext_sum", "min_log"))


# ---- 1. variates ----

@pytest.mark.parametrize("like,p", [(0, 1), (0, 2), (0, 3), (0, 64), (1, 1)])
def test_variates_against_long_double(accel_mod, like, p):
    Nx = 3001
    worst = 0.0
    for seed, first, reps in ((3, 0, (0, 5)), (0x9E3779B97F4A7C15, 1000, (1,)), (17, (1 << 32) - 2, (0, 1, 2))):
        with accel_mod.ScanNull(like, p, Nx, (1,) if like == 0 and p == 64 else (1, 8), seed, first_replicate=first) as null:
            for r in reps:
                got = null.variates(r)
                want, sens = R.variates(like, p, Nx, seed, first + r)
                assert np.all(np.isfinite(got)) and np.all(sens > 0)
                ratio = float(np.max(np.abs(got.astype(R.LD) - want) / (10.0 * sens)))
                worst = max(worst, ratio)
                print(f"RATIO scan-null variates like={like} p={p} seed={seed:#x} replicate={first + r}: {ratio:.3g}")
    assert worst <= 1.0, (like, p, worst)


def test_variates_cross_the_counter_word(accel_mod):
    """first_replicate = 2^32 - 2 with three replicates: the third has replicate words (0, 1).  The same replicates reached
    from another first_replicate are the same bits, and distinct from each other."""
    first = (1 << 32) - 2
    with accel_mod.ScanNull(0, 1, 257, (1, 5), 17, first_replicate=first) as a, \
            accel_mod.ScanNull(0, 1, 257, (1, 5), 17, first_replicate=first + 2) as b:
        q = [a.variates(r) for r in range(3)]
        assert same_bits(q[2], b.variates(0))
        assert not np.array_equal(q[0], q[1]) and not np.array_equal(q[1], q[2]) and not np.array_equal(q[0], q[2])
        a.run(3)
        b.run(1)
        for k in (0, 1):
            for which in (0, 1):
                ra, rb = a.result(k, which), b.result(k, which)
                assert same_bits(ra["ext_sum"][2], rb["ext_sum"][0]) and ra["pos"][2] == rb["pos"][0]
                for r in range(3):
                    want = R.extremes(q[r], a.widths[k])
                    assert (ra["ext_sum"][r], ra["pos"][r]) == want[2 * which:2 * which + 2], (k, which, r)


# ---- 2. extremes, exact ----

WIDE = (1, 2, 3, 8, 64, 256, 511, 512)
GRIDS = (2, 3, 511, 512, 513, 2047, 2048, 2049, 2048 + 511, 2048 + 512, 4097)
EXACT = [(0, 1, Nx, WIDE) for Nx in GRIDS] + [(1, 1, Nx, WIDE) for Nx in GRIDS] + \
        [(0, 1, Nx, (W,)) for W in (1, 2, 511, 512) for Nx in sorted({W, W + 1, 2049, 2560, 2048 + W - 1, 2048 + W})] + \
        [(1, 1, Nx, (W,)) for W in (1, 512) for Nx in (W, W + 1, 2048 + W)] + \
        [(0, 64, Nx, (1, 8)) for Nx in (8, 9, 2055, 2056)] + [(0, 2, 4097, (1, 2, 256)), (0, 3, 2049, (2, 170)), (0, 512, 2049, (1,))]


@pytest.mark.parametrize("like,p,Nx,want", EXACT)
def test_extremes_are_the_sliding_sums_of_the_variates(accel_mod, like, p, Nx, want):
    widths = tuple(W for W in want if W <= Nx)
    assert widths
    reps = 3
    with accel_mod.ScanNull(like, p, Nx, widths, 11) as null:
        assert null.run(reps) == reps
        q = [null.variates(r) for r in range(reps)]
        res = null_results(null)
    for k, W in enumerate(widths):
        for r in range(reps):
            smax, amax, smin, amin = R.extremes(q[r], W)
            assert same_bits(res[k][0]["ext_sum"][r], smax) and res[k][0]["pos"][r] == amax, (Nx, W, r, "max")
            assert same_bits(res[k][1]["ext_sum"][r], smin) and res[k][1]["pos"][r] == amin, (Nx, W, r, "min")


def test_positions_are_in_range(accel_mod):
    """(The tie rule itself is checked on the CPU, tests/cpp/scan_null_core_check.cpp: continuous variates do not tie.)"""
    with accel_mod.ScanNull(1, 1, 5000, (1, 7, 40), 5) as null:
        null.run(4)
        for k, W in enumerate(null.widths):
            hi, lo = null.result(k, 0), null.result(k, 1)
            assert np.all((hi["pos"] >= 0) & (hi["pos"] <= 5000 - W)) and np.all((lo["pos"] >= 0) & (lo["pos"] <= 5000 - W))
            assert np.all(hi["ext_sum"] > lo["ext_sum"])


# ---- 3. min_log ----

# shape -> bar (tamcmc_window.h): the power of two at or above twice the worst error measured against long double
BARS = {1: 2.0 ** -51, 2: 2.0 ** -49, 3: 2.0 ** -49, 25: 2.0 ** -47, 64: 2.0 ** -46, 256: 2.0 ** -44, 511: 2.0 ** -43, 512: 2.0 ** -43}
GAUSS_BAR = 2.0 ** -50


@pytest.mark.parametrize("like,p,widths", [(0, 1, (1, 2, 3, 25, 64, 256, 511, 512)), (0, 8, (8, 32, 64)), (1, 1, (1, 2, 7, 512))])
def test_min_log_against_scipy(accel_mod, like, p, widths):
    from scipy import stats
    with accel_mod.ScanNull(like, p, 3000, widths, 23) as null:
        null.run(40)
        res = null_results(null)
    for k, W in enumerate(widths):
        for which in (0, 1):
            S, got = res[k][which]["ext_sum"], res[k][which]["min_log"]
            if like == 0:
                a = p * W
                want = (stats.gamma.logsf if which == 0 else stats.gamma.logcdf)(p * S, a)
                bar = BARS[a]
            else:
                d = stats.norm(scale=np.sqrt(0.5))
                want = (d.logsf if which == 0 else d.logcdf)(S / np.sqrt(W))
                bar = GAUSS_BAR
            err = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
            print(f"MINLOG like={like} p={p} W={W} which={which}: error {err:.3g}, bar {bar:.3g}, values {want.min():.4g} ... {want.max():.4g}")
            assert np.all(got < 0) and err <= bar, (like, p, W, which, err, bar)


# ---- 4. bit independence ----

@pytest.mark.parametrize("like,p", [(0, 1), (0, 3), (1, 1)])
def test_a_replicate_depends_on_nothing_else(accel_mod, like, p):
    Nx, widths, seed = 2600, (1, 10, 40, 170), 29

    def results(n_runs, widths=widths, first=0):
        with accel_mod.ScanNull(like, p, Nx, widths, seed, first_replicate=first) as null:
            for n in n_runs:
                null.run(n)
            assert null.replicates == sum(n_runs)
            return null_results(null)

    def head(res, n, lo=0):
        return [[{key: v[lo:lo + n] for key, v in side.items()} for side in w] for w in res]

    full = results([50])
    assert same_results(head(full, 1), results([1]))
    assert same_results(head(full, 7), results([7]))
    assert same_results(full, results([1, 7, 30, 12]))
    assert same_results(full, results([49, 1]))
    # whichever other widths are in the list
    for sub in ((10,), (1, 170), (10, 40), (2, 10, 11, 40, 41, 168, 169, 170)):
        part = results([50], widths=sub)
        for k, W in enumerate(sub):
            if W in widths:
                assert same_results([full[widths.index(W)]], [part[k]]), (sub, W)
    # an object created at first_replicate = r
    for r in (1, 49):
        assert same_results(head(full, 1, lo=r), results([1], first=r)), r
    # and another seed is another spectrum
    with accel_mod.ScanNull(like, p, Nx, widths, seed + 1) as other:
        other.run(1)
        assert not same_bits(other.result(0, 0)["ext_sum"], full[0][0]["ext_sum"][:1])


# ---- 4b. a long grid: the chunk set by the memory of the partials ----

LONG_NX, LONG_WIDTHS, LONG_R = 131073, (1, 10, 20, 40, 64, 128, 256, 512), 4100


def long_chunk():
    """tmn_chunk (tamcmc_scan_null.h) restated: 64 MiB of partials at 2 K tiles (value, position) pairs of 16 bytes a
    replicate, at most 2^30 threads a launch of 256-thread workgroups, at most 4096."""
    K, tiles = len(LONG_WIDTHS), -(-(LONG_NX - LONG_WIDTHS[0] + 1) // 2048)
    return K * tiles, max(1, min((64 << 20) // (2 * K * tiles * 16), (1 << 30) // (tiles * 256), 4096))


@pytest.mark.parametrize("like", [0, 1], ids=["chi22p", "chi-square"])
def test_a_long_grid_in_chunks_set_by_memory(accel_mod, like):
    """131 073 bins with a narrowest width of 1 are 65 tiles; with eight widths K tiles = 520 > 512, so the memory rule and
    not the cap of 4096 sets the chunk: floor(2^21 / 520) = 4032 replicates.  One run of 4100 is a chunk of 4032 and one of 68.
    The replicates on both sides of that edge (and of 4033, where the edge would be with one pair less in the rule) have the
    reference's variates within the suite's bound and the extremes of the library's own variates bit for bit; the same seed
    run as the two chunks by hand, and as 41 runs of 100, gives the same bits in every replicate."""
    kt, C = long_chunk()
    assert kt == 520 and C == 4032 and 0 < LONG_R - C < C
    reps = sorted({0, C - 1, C, C + 1, 4033, LONG_R - 1})
    with accel_mod.ScanNull(like, 1, LONG_NX, LONG_WIDTHS, 31) as null:
        assert null.run(LONG_R) == LONG_R
        full = null_results(null)
        worst = 0.0
        for r in reps:
            q = null.variates(r)
            want, sens = R.variates(like, 1, LONG_NX, 31, r)
            assert np.all(np.isfinite(q)) and np.all(sens > 0)
            ratio = float(np.max(np.abs(q.astype(R.LD) - want) / (10.0 * sens)))
            worst = max(worst, ratio)
            print(f"RATIO scan-null long grid variates like={like} replicate={r}: {ratio:.3g}")
            for k, W in enumerate(LONG_WIDTHS):
                smax, amax, smin, amin = R.extremes(q, W)
                assert same_bits(full[k][0]["ext_sum"][r], smax) and full[k][0]["pos"][r] == amax, (W, r, "max")
                assert same_bits(full[k][1]["ext_sum"][r], smin) and full[k][1]["pos"][r] == amin, (W, r, "min")
        assert worst <= 1.0, (like, worst)
    for runs in ([C, LONG_R - C], [100] * 41):
        with accel_mod.ScanNull(like, 1, LONG_NX, LONG_WIDTHS, 31) as null:
            for n in runs:
                null.run(n)
            assert null.replicates == LONG_R
            assert same_results(full, null_results(null)), runs[:2]


# ---- 5. distribution ----

KS_BAR = 1.63 / np.sqrt(2000.0)


def test_distribution_of_the_maximum_of_exponentials(accel_mod):
    """p = 1, W = 1, Nx = 1000: -min_log is the largest of 1000 exponentials, CDF (1 - e^-t)^Nx.  (Reference alone: 0.0159.)"""
    with accel_mod.ScanNull(0, 1, 1000, (1,), 3) as null:
        null.run(2000)
        t = -null.result(0, 0)["min_log"]
    D = R.ks_distance(t, lambda x: (-np.expm1(-x)) ** 1000)
    print(f"KS max of exponentials: {D:.4f} (bar {KS_BAR:.4f})")
    assert D < KS_BAR


def test_distribution_of_a_gamma_sum(accel_mod):
    """p = 3, Nx = W = 8: 3 S is Gamma(24).  (Reference alone: 0.0145.)"""
    from scipy import stats
    with accel_mod.ScanNull(0, 3, 8, (8,), 3) as null:
        null.run(2000)
        hi, lo = null.result(0, 0), null.result(0, 1)
    assert same_bits(hi["ext_sum"], lo["ext_sum"]) and not hi["pos"].any() and not lo["pos"].any()     # one position
    D = R.ks_distance(3.0 * hi["ext_sum"], stats.gamma(24).cdf)
    print(f"KS gamma sum: {D:.4f} (bar {KS_BAR:.4f})")
    assert D < KS_BAR


def test_distribution_of_a_gaussian_sum(accel_mod):
    """chi_square, Nx = W = 8: S / sqrt(8) is N(0, 1/2).  (Reference alone: 0.0159.)"""
    from scipy import stats
    with accel_mod.ScanNull(1, 1, 8, (8,), 3) as null:
        null.run(2000)
        S = null.result(0, 0)["ext_sum"]
    D = R.ks_distance(S / np.sqrt(8.0), stats.norm(scale=np.sqrt(0.5)).cdf)
    print(f"KS gaussian sum: {D:.4f} (bar {KS_BAR:.4f})")
    assert D < KS_BAR


# ---- 6. calibration ----

@pytest.fixture(scope="module")
def calibrated(accel_mod):
    """Nx = 5000, widths (10, 20, 40), p = 1, R = 1000, seed 3: the open object and m[side] = (R, K) min_log.  Computed once."""
    with accel_mod.ScanNull(0, 1, 5000, (10, 20, 40), 3) as null:
        null.run(1000)
        m = [np.stack([null.result(k, which)["min_log"] for k in range(3)], axis=1) for which in (0, 1)]
        for a in m:
            a.setflags(write=False)
        yield null, m


def test_line_and_pvalue_are_the_counting_rule(accel_mod, calibrated):
    null, m = calibrated
    for which in (0, 1):
        for k in range(3):
            for alpha in (0.01, 0.001, 0.05, 0.5, 0.999):
                for joint in (False, True):
                    assert null.line(k, which, alpha, joint) == R.line(m[which], k, alpha, joint), (which, k, alpha, joint)
            assert null.line(k, which, 0.01, True) <= null.line(k, which, 0.01, False)
            for alpha in (0.0, 0.0009, 1.0, -0.1, float("nan")):
                with pytest.raises(accel_mod.AccelError) as e:
                    null.line(k, which, alpha)
                assert e.value.code == capi.E_INVALID
            col = m[which][:, k]
            for v in (col[0], col[17], float(col.min()), float(col.max()), float(col.min()) - 3.0, 0.0, float(np.median(col)) + 1e-12,
                      null.line(k, which, 0.01, True)):
                assert null.pvalue(k, which, v) == R.pvalue(m[which], k, v), (which, k, v)
    assert null.pvalue(0, 0, -1e9) == (1 / 1001, 1 / 1001)
    for bad in (lambda: null.line(3), lambda: null.line(-1), lambda: null.line(0, 2), lambda: null.pvalue(3, 0, -5.0),
                lambda: null.pvalue(0, -1, -5.0), lambda: null.pvalue(0, 0, float("nan")), lambda: null.result(3, 0), lambda: null.result(0, 2)):
        with pytest.raises(accel_mod.AccelError) as e:
            bad()
        assert e.value.code == capi.E_INVALID


def test_the_default_line_is_too_high(accel_mod, calibrated):
    """Each of the per-width and the joint 1 % line of the excess side lies at or below log(0.01 W / Nx).  (Reference alone:
    -12.71 / -11.74 / -11.48 per width, -13.95 / -12.49 / -12.52 jointly, against -10.82 / -10.13 / -9.43.)"""
    null, _ = calibrated
    for k, W in enumerate((10, 20, 40)):
        default = float(np.log(0.01 * W / 5000.0))
        per, joint = null.line(k, 0, 0.01, False), null.line(k, 0, 0.01, True)
        print(f"LINES W={W}: per width {per:.2f}, joint {joint:.2f}, default {default:.2f}")
        assert joint <= per <= default


def test_refusals_of_an_object_without_replicates(accel_mod):
    with accel_mod.ScanNull(0, 1, 100, (5,), 3) as null:
        assert null.replicates == 0 and null.result(0, 0)["min_log"].size == 0
        for bad in (lambda: null.line(0), lambda: null.pvalue(0, 0, -3.0), lambda: null.run(0), lambda: null.run(-1),
                    lambda: null.run((1 << 24) + 1), lambda: null.variates(-1)):
            with pytest.raises(accel_mod.AccelError) as e:
                bad()
            assert e.value.code == capi.E_INVALID
        null.profile(True)
        null.run(99)                                                      # floor(0.01 * 100) = 1: the smallest R with a 1 % line
        ms, chunks = null.kernel_time()
        assert ms > 0 and chunks == 1
        assert null.line(0, 0, 0.01, False) == float(null.result(0, 0)["min_log"].min())
        null.profile(False)
        null.run(5000)                                                    # two chunks of at most 4096
        assert null.replicates == 5099 and null.kernel_time() == (0.0, 0)
        split = null_results(null)
    with accel_mod.ScanNull(0, 1, 100, (5,), 3) as again:
        again.run(5099)
        assert same_results(split, null_results(again))


# ---- 7. with a chain ----

def test_a_planted_run_is_the_one_region_below_the_joint_line(accel_mod):
    """700 bins of y = M e with exponential e, M the model at the generating parameters; in 20 bins y = ratio M, the ratio
    chosen on the CPU from gamma.logsf so that the window over the run lies 6 below the joint 1 % line of width 20 (at least
    3 once the chain's rows stand in for M).  The one region of scan_regions(log_below = the joint line) is that run, and its
    p_joint is 1 / (R + 1): no replicate of the null is that extreme."""
    from scipy import optimize, stats
    Nx, widths, b0, nb, Rn = 700, (10, 20, 40), 350, 20, 500
    w = synth.workload_c2(Nx=Nx)
    M0 = true_model(w)
    y = M0 * np.random.default_rng(2).exponential(size=Nx)
    P = synth.chain_params(w, 100, scale=0.05)
    with accel_mod.ScanNull(0, 1, Nx, widths, 3) as null:
        null.run(Rn)
        lines = [null.line(k, 0, 0.01, True) for k in range(3)]
        ratio = optimize.brentq(lambda t: stats.gamma.logsf(nb * t, nb) - (lines[1] - 6.0), 1.0, 50.0)
        y[b0:b0 + nb] = ratio * M0[b0:b0 + nb]
        with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
            with capi.Summary(acc, scan=widths) as s:
                s.push(P)
                res = s.scan_result(1)
                found = [s.scan_regions(k, 0, log_below=lines[k]) for k in range(3)]
        print(f"PLANTED ratio {ratio:.4g}, joint lines {lines}, scan minimum {res['min_log_sf']:.4f} at {res['pos_min_log_sf']}, regions {found[1]}")
        assert res["min_log_sf"] <= lines[1] - 3.0
        assert len(found[1]) == 1
        r = found[1][0]
        assert r["pos_first"] <= b0 <= r["pos_last"] and abs(r["pos_min"] - b0) <= 2 and r["min_log"] == res["min_log_sf"]
        assert b0 - nb < r["bin_first"] and r["bin_last"] < b0 + 2 * nb
        assert null.pvalue(1, 0, r["min_log"]) == (1 / (Rn + 1), 1 / (Rn + 1))
        # the other widths see the same feature and nothing else
        for k in (0, 2):
            assert all(b0 - widths[k] < q["bin_first"] and q["bin_last"] < b0 + nb + widths[k] for q in found[k]), (k, found[k])


def test_a_null_on_the_device_changes_no_bit_of_a_summary(accel_mod):
    Nx = 700
    w = synth.workload_c2(Nx=Nx)
    y = synth.make_spectrum(true_model(w), seed=17)
    P = synth.chain_params(w, 37)

    def summary():
        with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
            with capi.Summary(acc, 16, predictive=True, window=20, scan=(10, 20, 40)) as s:
                s.push(P[:20])
                mid = [s.scan_result(k) for k in range(3)]
                s.push(P[20:])
                return s.result(), s.predictive_result(), s.window_result(), [s.scan_result(k) for k in range(3)], mid

    alone = summary()
    with accel_mod.ScanNull(0, 1, Nx, (10, 20, 40), 3) as null:
        null.run(10)
        before = null_results(null)
        beside = summary()
        null.run(10)
        after = null_results(null)
    assert same(alone[0], beside[0]) and same_pred(alone[1], beside[1]) and same_win(alone[2], beside[2])
    assert same_scans(alone[3], beside[3]) and same_scans(alone[4], beside[4])
    assert same_results(before, [[{key: v[:10] for key, v in side.items()} for side in wd] for wd in after])
