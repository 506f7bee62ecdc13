"""The extreme-value columns of tests/columncases.py have the properties they are named for, and the numpy references the GPU
suite compares the column kernels with (modetable_reference.fold, the sort behind the quantiles, moderank_reference,
modediag_reference, modepdf_reference) run over every set and agree with a brute-force statement of the same definition.
No GPU and no library."""
import math

import numpy as np
import pytest

import columncases as CC
import ess_reference as ER
import modediag_reference as DR
import modepdf_reference as PR
import moderank_reference as RR
import modetable_reference as MR
from support import LD, bits

SMALL = (64, 257)
CASES = [(name, n) for name in CC.SETS for n in CC.sizes(name)]
QS = np.array([0.0, 1e-9, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0])


def key_int(v):
    return int(RR.key(np.float64(v)))


def span_bits(v):
    k = RR.key(v)
    return (int(k.max()) - int(k.min())).bit_length()


@pytest.mark.parametrize("name,n", CASES)
def test_sets_are_deterministic_and_free_of_nan(name, n):
    v = CC.column(name, n)
    assert v.dtype == np.float64 and v.shape == (n,) and not np.any(np.isnan(v))
    assert np.array_equal(bits(v), bits(CC.column(name, n)))
    if n >= 64:
        assert not np.array_equal(bits(v), bits(CC.column(name, n, seed=1))) or name in ("zeros-alt", "ties-equal", "ties-but_one")


def test_key_spans():
    """span64 (with or without the infinities) spans 64 key bits -- eight 8-bit digits, the u >= 64 side of tmq_match; the
    neighbours differ in the last 9 bits at most; +0 and -0 are one key."""
    for n in CC.sizes("span64"):
        assert span_bits(CC.column("span64", n)) == 64 and span_bits(CC.column("span64-inf", n)) == 64
        assert span_bits(CC.column("scaled", n)) >= 62
        v = CC.column("span64-inf", n)
        assert np.isneginf(v.min()) and np.isposinf(v.max()) and np.isfinite(CC.column("span64", n)).all()
        assert CC.column("span64", n).min() == -CC.DBL_MAX and CC.column("span64", n).max() == CC.DBL_MAX
    for n in CC.sizes("neighbours"):
        v = np.unique(CC.column("neighbours", n))
        assert v.size == min(n, 300) and 1 <= span_bits(v) <= 9
        assert np.array_equal(np.diff(RR.key(v).astype(np.int64)), np.ones(v.size - 1, dtype=np.int64))       # consecutive doubles
    assert span_bits(CC.column("zeros-alt", 64)) == 0 and key_int(0.0) == key_int(-0.0)
    d = CC.column("denormals", 257)
    assert np.any(d == CC.DENORM) and np.any(d == -CC.DENORM) and np.any(d == CC.DBL_MIN) and np.any(np.signbit(d) & (d == 0))
    assert np.abs(CC.column("denormals-smallest", 257)).max() == 2 * CC.DENORM


def test_zero_signs_and_ties():
    for n in CC.sizes("zeros-alt"):
        v = CC.column("zeros-alt", n)
        assert np.all(v == 0.0) and np.signbit(v).sum() == n // 2
    for n in CC.sizes("zeros-among"):
        v = CC.column("zeros-among", n)
        z = v == 0.0
        assert z.sum() == len(range(0, n, 3)) and (n < 4 or (np.signbit(v[z]).any() and not np.signbit(v[z]).all()))
        assert n < 64 or (np.any(v < 0) and np.any(v > 0))
    for n in CC.sizes("ties-halves"):
        assert np.unique(CC.column("ties-equal", n)).size == 1
        u, c = np.unique(CC.column("ties-but_one", n), return_counts=True)
        assert sorted(c) == [1, n - 1]
        u, c = np.unique(CC.column("ties-halves", n), return_counts=True)
        assert sorted(c) == [n // 2, n - n // 2]
        u, c = np.unique(CC.column("ties-twice", n), return_counts=True)
        assert np.all(c[:n // 2] == 2) and u.size == (n + 1) // 2


def test_infinities_and_overflow():
    for n in CC.sizes("infs-both"):
        for name, npos, nneg in (("infs-plus", 1, 0), ("infs-minus", 0, 1), ("infs-both", 1, 1)):
            v = CC.column(name, n)
            assert np.isposinf(v).sum() == npos and np.isneginf(v).sum() == nneg and np.isfinite(v).sum() == n - npos - nneg
    for n in CC.sizes("huge"):
        v = CC.column("huge", n)
        f = MR.fold(v[:, None])
        assert np.all(np.isfinite(v)) and np.isfinite(f["mean"][0]) and np.isposinf(f["sd"][0])          # M2 overflows, the mean does not
        with np.errstate(over="ignore"):
            assert np.isposinf(np.sum((v - f["mean"][0]) ** 2))


def test_histogram_scale_overflows():
    """n_bins / (hi - lo) overflows for every n_bins on denormals-smallest and from 9 classes on over the whole denormals set;
    then v == lo is class 0 (0 * inf is a NaN) and every other value the last class.  Around 110.2 no span of doubles is
    short enough: the neighbours' scale stays finite and single ulps of (v - lo) * s decide the class."""
    for name, bins_over, bins_fine in (("denormals-smallest", (1, 2, 64, 4096), ()), ("denormals", (64, 4096), (1, 2, 8))):
        for n in (64, 257):
            v = CC.column(name, n)
            lo, hi = v.min(), v.max()
            with np.errstate(over="ignore"):
                for b in bins_over:
                    assert np.isinf(np.float64(b) / (hi - lo))
                    c = PR.classes(v, lo, hi, b)
                    assert np.all(c[v == lo] == 0) and np.all(c[v != lo] == b - 1)
                for b in bins_fine:
                    assert np.isfinite(np.float64(b) / (hi - lo))
    v = CC.column("neighbours", 257)
    assert np.isfinite(4096.0 / (v.max() - v.min())) and np.unique(PR.classes(v, v.min(), v.max(), 4096)).size > 100


def brute_class(v, lo, hi, bins):
    """tmp_class one value at a time in Python floats."""
    if v < lo:
        return -1
    if v > hi:
        return -2
    if not hi > lo:
        return 0
    try:
        s = bins / (hi - lo)
    except ZeroDivisionError:
        s = math.inf
    u = (v - lo) * s
    if u != u:
        return 0
    return int(min(math.floor(u), bins - 1)) if u != math.inf else bins - 1


def scale(bins, lo, hi):
    with np.errstate(over="ignore"):
        return float(np.float64(bins) / (np.float64(hi) - np.float64(lo)))


@pytest.mark.parametrize("name", CC.SETS)
def test_references_against_brute_force(name):
    for n in [m for m in SMALL if m >= CC.MIN_N.get(name, 1)]:
        v = CC.column(name, n)
        tag = (name, n)
        # quantiles: the order statistic by counting
        s = PR.sorted_column(v)
        assert np.array_equal(bits(s), bits(RR.sorted_values(v))) and not np.any(np.signbit(s[s == 0])), tag
        keys = [key_int(x) for x in v]
        for q in QS:
            k = int(min(max(math.ceil(q * n) - 1, 0), n - 1))
            kk = key_int(s[k])
            assert sum(x < kk for x in keys) <= k < sum(x <= kk for x in keys), (tag, q)
        # ranks: #{<} + #{<=} + 1 by counting
        r2 = RR.rank2(v)
        assert r2.tolist() == [sum(x < y for x in keys) + sum(x <= y for x in keys) + 1 for y in keys], tag
        assert int(r2.sum()) == n * (n + 1), tag
        # histogram classes one value at a time, default and explicit range
        lo, hi = float(v.min()), float(v.max())
        ranges = [(lo, hi)] if PR.range_ok(lo, hi) else []
        fin = v[np.isfinite(v)]
        ranges.append((float(np.median(fin)), float(fin.max())))
        for (a, b) in ranges:
            for nb in (1, 64, 4096):
                c = PR.classes(v, a, b, nb)
                want = []
                for x in v:
                    if b > a and math.isinf(scale(nb, a, b)):
                        want.append(-1 if x < a else -2 if x > b else 0 if x == a else nb - 1)
                    else:
                        want.append(brute_class(float(x), a, b, nb))
                assert c.tolist() == want, (tag, a, b, nb)
        h = PR.hist(v[:, None], 64)
        assert h["status"][0] == (0 if PR.range_ok(lo, hi) else PR.RANGE), tag
        if h["status"][0] == 0:
            assert h["counts"].sum() == n and h["below"][0] == 0 and h["above"][0] == 0, tag
        else:
            assert h["counts"].sum() == 0, tag
        # the shortest interval: every window, the first shortest, a NaN width last
        masses = (1.0 / n, 0.5, 0.95, 1.0)
        got = PR.hpd(v[:, None], masses)
        for m, mass in enumerate(masses):
            k = max(1, min(n, int(math.ceil(np.float64(mass) * np.float64(n)))))
            best, at = None, 0
            for i in range(n - k + 1):
                with np.errstate(invalid="ignore", over="ignore"):
                    wdt = s[i + k - 1] - s[i]
                if not np.isnan(wdt) and (best is None or wdt < best):
                    best, at = wdt, i
            assert got["k"][m] == k and got["start"][m, 0] == at, (tag, mass)
            assert bits(got["lo"][m, 0]) == bits(s[at]) and bits(got["hi"][m, 0]) == bits(s[at + k - 1]), (tag, mass)


@pytest.mark.parametrize("name", CC.SETS)
def test_references_run_on_every_set(name):
    """fold, the centred lag products, the covariance, the correlation, the finish and the pair density on two planted columns
    beside a constant one: nothing raises, and the finite sets agree with long double."""
    for n in [m for m in SMALL if m >= CC.MIN_N.get(name, 1)]:
        other = "ties-twice" if name != "ties-twice" else "neighbours"
        rows = np.stack([CC.column(name, n), CC.column(other, n, seed=3), np.full(n, 0.15)], axis=1)
        f = MR.fold(rows)
        assert bits(f["min"][0]) == bits(rows[np.argmin(rows[:, 0]), 0]) or rows[:, 0].min() == 0.0
        assert f["min"][0] == rows[:, 0].min() and f["max"][0] == rows[:, 0].max() and f["sd"][2] == 0.0 and f["mean"][2] == 0.15
        finite = bool(np.all(np.isfinite(rows)) and np.isfinite(f["sd"]).all())
        if finite:
            c = rows.astype(LD)
            # (+ one denormal step per sample: below DBL_MIN the recurrence rounds to multiples of 5e-324, not to 2^-52 relative)
            assert np.all(np.abs(f["mean"].astype(LD) - c.mean(axis=0)) <= n * (2.0 ** -52 * np.abs(c).mean(axis=0) + LD(CC.DENORM))), (name, n)
        else:
            assert name.startswith("infs") or name in ("huge", "span64", "span64-inf"), name
        L = ER.lag_limit(0, n)
        with np.errstate(all="ignore"):
            d, e = DR.centred(rows, f["mean"])
            A, bound = DR.lag(d, e, L)
            S, sb = DR.cov_sums(d, e)
            r, rb = DR.corr(S, sb)
            A64 = np.asarray(A).astype(np.float64)
            tau, ess, cut = ER.finish(A64, n)
        assert A.shape == (L + 1, 3) and S.shape == (3, 3) and r.shape == (3, 3) and cut.shape == (3,)
        assert np.isnan(float(r[0, 2])) and np.isnan(float(r[2, 2])), (name, n)               # the constant column
        if finite:
            assert float(r[1, 1]) == 1.0, (name, n)
            if S[0, 0] > 0:                # (long double: the denormals' sum of squares, 1e-640, is a zero in double alone)
                assert abs(float(r[0, 1])) <= 1.0 + 1e-6, (name, n)
            else:
                assert np.isnan(float(r[0, 1])), (name, n)
        p = PR.hist2d(rows, [(0, 1), (0, 0), (1, 2)], 8, mass=(0.5, 0.95))
        ok = PR.range_ok(rows[:, 0].min(), rows[:, 0].max())
        assert p["status"].tolist() == [0 if ok else PR.RANGE, 0 if ok else PR.RANGE, 0], (name, n)
        assert p["counts"][2].sum() == n and (not ok or (p["counts"][0].sum() == n and np.trace(p["counts"][1]) == n)), (name, n)


def test_planting():
    """plant() changes the frequency entries alone; the layouts have 13 and 22 columns with the planted columns where the
    module says."""
    for w, nc in ((CC.one_mode(), 13), (CC.two_modes(), 22)):
        cols = MR.layout(11, w["plength"])
        assert len(cols) == nc and w["params_true"].size == int(w["plength"].sum())
        assert [int(c) for c in MR.first_columns(cols)] == w["freq_cols"]
        assert [int(cols["param_index"][c]) for c in w["freq_cols"]] == w["freq_index"]
        assert all(cols["kind"][c] == MR.K["nu_m"] for c in w["nu_cols"])
        vs = [CC.column("span64-inf", 64, seed=k) for k in range(len(w["freq_index"]))]
        P = CC.plant(w, *vs)
        keep = np.ones(P.shape[1], dtype=bool)
        keep[w["freq_index"]] = False
        assert np.array_equal(bits(P[:, keep]), bits(np.tile(w["params_true"][keep], (64, 1))))
        for idx, v in zip(w["freq_index"], vs):
            assert np.array_equal(bits(P[:, idx]), bits(v))
