"""Extreme column values through every column kernel of the mode table: the fold, the table's quantile kernel, the lag and
covariance kernels (modediag), the sort, transform and mean kernels (moderank), the histogram, HPD and pair kernels (modepdf).

The columns are those of tests/columncases.py -- +-0, denormals, a key span of 64 bits with and without +-inf, consecutive
doubles, single infinities, values whose squares overflow, ties -- planted in the frequency of the single l = 0 mode of the
13-column local layout (the freq column equals the params entry bit for bit, nu_m repeats it, the truncation window clamps a
mode outside the grid: every planted row has status 0, asserted), and two different sets in the two l = 0 modes of a 22-column
layout for pairs, covariance and correlation.  Every other column is constant or a window edge (an integer step function of
the frequency).  n = 1, 2, 64, 257, 4097, 8193 where the set allows: one wave, the quantile kernel's stride, the push block,
the sort tile.

Per set and size, on the library's own derived rows:
  1  result(): mean, sd, min, max equal the float64 restatement of the fold in push order bit for bit (NaN for NaN) -- so min
     and max are the exact extremes, a zero extreme carrying the sign of the zero pushed first; on the sets of normal range
     also within the statistics bounds of the mode-table suite.
  2  quantiles: inverted_cdf ranks, the order statistic bit for bit, a zero as +0.
  3  ess / acov / cov / corr: the finish on the library's own lag products and the totals everywhere; on the sets of normal
     range the long-double bounds of the modediag suite (modediag_support); on infs, huge and the unscaled span64 (sums
     that overflow) and on the denormals (products that underflow: A_0 = 0, counted in n_constant) the NaN / +-inf / zero
     pattern of the float64 restatement; corr is the restatement of tmd_corr on the library's own cov bit for bit.
  4  rank_series / rank_diag as the moderank suite checks them (moderank_support); and a law that needs no reference: a
     strictly increasing map that sends the column's ends to +-inf or +-DBL_MAX leaves rank2, the z series, the I05 / I95
     indicator series and everything computed from them the same bits.
  5  hist: the class rule on the default range, an explicit one, the overflowing scale, n_bins 1, 64, 4096; status RANGE and
     all-zero counts for a default range that holds an infinity.
  6  hpd: k, start, lo, hi at masses 1 / n, 0.5, 0.95, 1 (from n = 4, the sort kernel's condition; refused below).
  7  hist2d: counts, outside, levels, status for pairs of sets and a column with itself, n_bins 1, 2, 128.
  8  every result is independent of the push split (at once, blocks of 29), max_samples (n, n + 37), the selection order
     (rank_diag, hist and hpd on every column reversed and on a permuted subset; cov and the pairs permuted) and the scratch
     size (one column per chunk, two).
test_zz_report prints the worst ratios."""
import numpy as np
import pytest

import columncases as CC
import ess_reference as ER
import modediag_support as DS
import modepdf_reference as PR
import moderank_reference as RR
import moderank_support as RS
import modetable_reference as MR
from modetable_support import QS, check_statistics, open_acc, ranks_of
from support import bits

pytestmark = pytest.mark.gpu

RANK_WORST = {"z": 0.0, "lag": 0.0, "rhat": 0.0}
NORMAL_RANGE = ("zeros-alt", "zeros-among", "neighbours", "ties-equal", "ties-but_one", "ties-halves", "ties-twice", "scaled")
UNDERFLOW = ("denormals", "denormals-smallest")                           # every product of two centred values is a zero
FINITE_SUMS = NORMAL_RANGE + UNDERFLOW                                    # no sum of products overflows
BINS = (1, 64, 4096)
WORST = {"lag": 0.0, "cov": 0.0, "rhat": 0.0, "corr": 0.0}
K = MR.K
CASES = [(name, n) for name in CC.SETS for n in CC.sizes(name)]


def nan_eq(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def same(want, got, tag, keys):
    for k in keys:
        a, b = np.asarray(want[k]), np.asarray(got[k])
        assert a.shape == b.shape, (tag, k)
        assert nan_eq(a, b) if a.dtype == np.float64 else np.array_equal(a, b), (tag, k)


def planted_rows(mt, w, P, columns):
    """derive() of the planted rows: status 0 everywhere, the planted bits in the freq and nu_m columns, every other column
    the base row's but the window edges, which are integers with 0 <= lo < hi <= Nx."""
    base, st0 = mt.derive(w["params_true"][None, :])
    rows, st = mt.derive(P)
    assert st0[0] == 0 and np.all(st == 0), np.flatnonzero(st)
    cols = mt.columns()
    window = np.isin(cols["kind"], [K["window_lo"], K["window_hi"]])
    want = CC.expected_rows(w, base[0], *columns)
    assert np.array_equal(bits(rows[:, ~window]), bits(want[:, ~window]))
    for c0 in w["freq_cols"]:
        lo, hi = rows[:, c0 + 5], rows[:, c0 + 6]
        assert np.all(lo == np.floor(lo)) and np.all(hi == np.floor(hi)) and np.all((0 <= lo) & (lo < hi) & (hi <= w["x"].size))
    return rows


def tmd_corr(cov):
    """The header's correlation on a covariance matrix, float64: NaN where either variance is 0 or not finite, 1.0 on the
    diagonal, cov_ij / (sqrt(cov_ii) sqrt(cov_jj)) clamped to [-1, 1] elsewhere."""
    var = np.diag(cov)
    ok = (var > 0.0) & (var <= np.finfo(np.float64).max)
    with np.errstate(all="ignore"):
        s = np.sqrt(var)
        r = cov / (s[:, None] * s[None, :])
    r = np.where(r > 1.0, 1.0, np.where(r < -1.0, -1.0, r))
    r[np.diag_indices_from(r)] = 1.0
    r[~ok, :] = np.nan
    r[:, ~ok] = np.nan
    return r


def pattern(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


def check_result(tag, name, res, rows):
    """Check 1."""
    n = len(rows)
    want = MR.fold(rows)
    for k in ("mean", "sd", "min", "max"):
        assert nan_eq(res[k], want[k]), (tag, k, np.flatnonzero(bits(res[k]) != bits(want[k])))
    assert np.array_equal(res["min"], rows.min(axis=0)) and np.array_equal(res["max"], rows.max(axis=0)), tag
    first_zero = rows[np.argmax(rows == 0.0, axis=0), np.arange(rows.shape[1])]              # (the first zero of the column, if any)
    for k, ext in (("min", rows.min(axis=0)), ("max", rows.max(axis=0))):
        z = ext == 0.0
        assert np.array_equal(np.signbit(res[k][z]), np.signbit(first_zero[z])), (tag, k, "the sign of the zero pushed first")
    assert res["n_used"] == n and res["n_rejected"] == 0, tag
    if name in NORMAL_RANGE:
        # (a zero extreme's sign is pinned above; numpy's own min of +0 and -0 is either)
        check_statistics(tag, dict(res, min=res["min"] + 0.0, max=res["max"] + 0.0), rows + 0.0)


def check_quantiles(tag, mt, rows):
    """Check 2."""
    n = len(rows)
    q = mt.quantiles(QS)
    assert np.array_equal(q["ranks"], ranks_of(QS, n)), tag
    want = np.sort(rows + 0.0, axis=0)[q["ranks"]]
    assert np.array_equal(bits(q["values"]), bits(want)), (tag, np.argwhere(bits(q["values"]) != bits(want))[:4])
    assert not np.any(np.signbit(q["values"][q["values"] == 0.0])), tag
    return q


def fma_sums(rows, mean, L):
    """Steps 1 and 3 of the header and its covariance sums with the overflow behaviour of the fused multiply-add they are
    stated with: (A (L + 1, n_cols), S (n_cols, n_cols)) in float64, each accumulator advanced in ascending t by
    round(d_t d_{t-k} + A) -- the product exact (long double holds it), so that an accumulator that has overflowed to an
    infinity keeps it whatever the sign of the later finite products, where a product rounded to an infinity first would
    give inf - inf.  For the NaN / +-inf / zero pattern; the finite values are not the library's bits."""
    LD = np.longdouble
    with np.errstate(all="ignore"):
        d = (rows - mean).astype(LD)
        n, nc = d.shape
        A, S = np.zeros((L + 1, nc)), np.zeros((nc, nc))
        for t in range(n):
            k = np.arange(min(t, L) + 1)
            A[k] = (d[t][None, :] * d[t - k] + A[k].astype(LD)).astype(np.float64)
            S = (d[t][:, None] * d[t][None, :] + S.astype(LD)).astype(np.float64)
    return A, S


def float64_diag_pattern(rows, mean, L):
    A, S = fma_sums(rows, mean, L)
    return pattern(A), pattern(S)


def check_finish(tag, r, L, n):
    """The finish on the library's own lag products (ess_reference.finish) and the totals from the arrays, as the modediag
    suite has them; A_0 zero or not finite: tau = ess = mcse = NaN, cut = 0."""
    A = r["acov"]
    tau, ess, cut = ER.finish(A, n)
    floor = 1.0 / np.log10(float(n))
    assert np.array_equal(cut, r["cut"]), tag
    for got, want in ((r["tau"], tau), (r["ess"], ess)):
        on_floor = np.abs(tau - floor) <= 4 * DS.U * floor
        with np.errstate(invalid="ignore"):
            ok = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)) | (on_floor & (np.abs(got - want) <= 4 * DS.U * np.abs(want)))
        assert np.all(ok), (tag, np.flatnonzero(~ok))
    dead = ~(np.isfinite(A[0]) & (A[0] > 0.0))
    for k in ("ess", "tau", "mcse"):
        assert np.all(np.isnan(r[k][dead])), (tag, k)
    assert np.all(r["cut"][dead] == 0) and r["n_constant"] == np.sum(A[0] == 0.0), tag
    want_t = DS.DR.totals(r["ess"], r["rhat"], r["cut"], A[0], L, n)
    for k in DS.TOTALS:
        assert r[k] == want_t[k] or (isinstance(want_t[k], float) and np.isnan(want_t[k]) and np.isnan(r[k])), (tag, k, r[k], want_t[k])
    return dead


def check_diag(tag, name, mt, rows, res, max_lag):
    """Check 3."""
    n, nc = rows.shape
    L = ER.lag_limit(max_lag, n)
    r = mt.ess(max_lag)
    r["acov"], r["cov"], r["corr"] = mt.acov(), mt.cov(), mt.corr()
    assert nan_eq(r["corr"], tmd_corr(r["cov"])), (tag, "corr is tmd_corr of cov")
    assert np.array_equal(bits(r["cov"]), bits(r["cov"].T)) and np.array_equal(bits(np.diag(r["cov"])), bits(r["acov"][0] / np.float64(n - 1))), tag
    dead = check_finish(tag, r, L, n)
    const = rows.min(axis=0) == rows.max(axis=0)
    assert np.all(r["acov"][:, const] == 0.0) and np.all(np.isnan(r["rhat"][const])) and np.all(dead[const]), tag
    assert np.all(np.isnan(r["corr"][dead, :])) and np.all(np.isnan(r["corr"][:, dead])), tag
    want_rhat = float64_rhat(rows, res["mean"])
    if name in NORMAL_RANGE:
        DS.check_against_references(tag, r, rows, res, L, worst=WORST)
        # a half of equal values beside another (ties-but_one: the odd value sits between the halves) has W = 0: NaN
        assert np.array_equal(np.isnan(r["rhat"]), np.isnan(want_rhat)), (tag, "rhat", r["rhat"], want_rhat)
        live = np.isfinite(want_rhat)
        if live.any():
            # R-hat does not change with a shift, and the long-double reference needs one here: consecutive doubles at 110.2 lie
            # 2^-52 apart, a long-double mean of 4096 of them is good to 2^-64 of 110.2 -- 1e-8 of their spread.  The first row
            # is subtracted in long double (exact for values within a factor 2^11 of each other)
            shifted = rows[:, live].astype(np.longdouble) - rows[0, live].astype(np.longdouble)
            DS.check_rhat(tag, r["rhat"][live], shifted, worst=WORST)
        return
    # infs, huge, span64: sums that overflow; denormals: products that underflow.  The NaN / +-inf / zero pattern of the float64
    # restatement, in every column (the window edges beside the planted column are finite and live)
    pA, pS = float64_diag_pattern(rows, res["mean"], L)
    assert np.array_equal(pattern(r["acov"]), pA), (tag, "acov")
    assert np.array_equal(pattern(r["cov"]), pS), (tag, "cov")
    planted = ~const & ~np.isin(mt.columns()["kind"], [K["window_lo"], K["window_hi"]])
    assert planted.sum() == 2 and np.all(dead[planted]), tag
    if name in UNDERFLOW:
        assert np.all(r["acov"][:, planted] == 0.0) and np.all(r["cov"][planted] == 0.0), tag
    else:
        assert np.all(pA[0][planted] != 0), tag
    assert np.array_equal(pattern(r["rhat"]), pattern(want_rhat)), (tag, "rhat", r["rhat"], want_rhat)
    fin = np.isfinite(want_rhat)
    assert np.all(np.abs(r["rhat"][fin] - want_rhat[fin]) <= 8 * (n // 2) * 2.0 ** -52 * want_rhat[fin]), tag


def float64_rhat(rows, mean):
    """Step 5 of the header in float64: Welford over the centred halves, W, Bn, sqrt(((h - 1) / h W + Bn) / W); W = 0: NaN."""
    n = len(rows)
    h = n // 2
    with np.errstate(all="ignore"):
        d = rows - mean
        m, s2 = [], []
        for half in (d[:h], d[n - h:]):
            f = MR.fold(half)
            m.append(f["mean"])
            s2.append(f["sd"] * f["sd"])
        Wv = (s2[0] + s2[1]) / 2.0
        mb = (m[0] + m[1]) / 2.0
        Bn = (m[0] - mb) ** 2 + (m[1] - mb) ** 2
        out = np.sqrt(((h - 1.0) / h * Wv + Bn) / Wv)
    return np.where(Wv == 0.0, np.nan, out)


def check_rank(tag, mt, rows, q, max_lag, columns):
    """Check 4 against the references.  Returns the rank_diag snapshot."""
    n, nc = rows.shape
    L = ER.lag_limit(max_lag, n)
    rng = np.random.default_rng(n)
    q2 = mt.quantiles([0.05, 0.95])["values"]
    r = RS.snapshot(mt, max_lag)
    series_of = {int(c): RS.check_column(tag, mt, int(c), rows[:, c], n, q2, rng, worst=RANK_WORST) for c in columns}
    RS.check_results(tag, r, n, L, series_of, worst=RANK_WORST)
    const = rows.min(axis=0) == rows.max(axis=0)
    with np.errstate(all="ignore"):
        tied = np.array([RR.rank2(rows[:, c]).min() == RR.rank2(rows[:, c]).max() for c in range(nc)])      # +-0 alone: one rank
    assert np.all(tied[const]) and r["n_constant"] == tied.sum(), tag
    return r


def check_hist(tag, name, mt, res, rows, col):
    """Check 5."""
    n = len(rows)
    v = rows[:, col]
    fin = v[np.isfinite(v)]
    for bins in BINS:
        got = mt.hist(bins)
        want = PR.hist(rows, bins)
        assert np.array_equal(want["range"], np.stack([res["min"], res["max"]], axis=1)), (tag, bins)
        want["range"] = np.stack([res["min"], res["max"]], axis=1)          # result()'s own: a zero with the sign the fold kept
        same(want, got, (tag, bins), ("counts", "below", "above", "range", "status"))
        ok = got["status"] == 0
        assert np.all(got["counts"][ok].sum(axis=1) == n) and np.all(got["counts"][~ok] == 0), (tag, bins)
        assert (got["status"][col] == PR.RANGE) == (not PR.range_ok(v.min(), v.max())), (tag, bins)     # an infinity, or hi - lo one
        # explicit ranges on the planted column: one that cuts both tails of the finite values, and min ... max of them
        explicit = ((np.quantile(fin, 0.25, method="inverted_cdf"), np.quantile(fin, 0.75, method="inverted_cdf")), (fin.min(), fin.max())) if fin.size else ()
        for lo, hi in explicit:
            if not PR.range_ok(lo, hi):
                continue
            g = mt.hist(bins, [col], [lo], [hi])
            same(PR.hist(v[:, None], bins, [lo], [hi]), g, (tag, bins, lo, hi), ("counts", "below", "above", "range", "status"))
            assert g["counts"].sum() + g["below"][0] + g["above"][0] == n, (tag, bins)
        if name.startswith("denormals") and bins >= 64 and n >= 64:
            lo, hi = v.min(), v.max()
            with np.errstate(over="ignore"):
                assert np.isinf(np.float64(bins) / (hi - lo))
            c = got["counts"][col]
            assert c[0] == np.sum(v == lo) and c[bins - 1] == np.sum(v != lo) and c[1:bins - 1].sum() == 0, (tag, bins, "the overflowing scale")


def selections(w, nc):
    """Check 8's selections: every column in reverse order, and a permuted subset that holds the planted column, its nu_m
    copy, a window edge and constant columns."""
    col = w["freq_cols"][0]
    return [np.arange(nc - 1, -1, -1).astype(np.int32), np.array([w["nu_cols"][0], 0, col + 6, col, 5, col + 5], dtype=np.int32)]


def check_rank_selection(tag, mt, r, max_lag, sels, scratch):
    """Check 8 for rank_diag: a selection returns the columns of the whole table's result, in the selection's order, bit for
    bit -- the arrays, the cuts and the four series' lag products."""
    for sel in sels:
        sub = RS.snapshot(mt, max_lag, sel, scratch)
        assert np.array_equal(sub["cols"], sel), tag
        for k in RR.OUT:
            assert nan_eq(sub[k], r[k][sel]), (tag, "selection", k, sel)
        assert np.array_equal(sub["cut"], r["cut"][:, sel]), (tag, "selection", sel)
        for s in RR.SERIES:
            assert np.array_equal(bits(sub["acov_" + s]), bits(r["acov_" + s][:, sel])), (tag, "selection", s, sel)
        assert sub["n_used"] == r["n_used"] and sub["lag"] == r["lag"], tag


def check_hist_selection(tag, mt, rows, sels):
    """Check 8 for hist: a permuted selection, on the default range and on explicit ranges (per column the quartiles of its
    finite values, which cut both tails of a column that moves and are lo = hi on a constant one)."""
    keys = ("counts", "below", "above", "range", "status")
    for sel in sels:
        for bins in BINS:
            whole, got = mt.hist(bins), mt.hist(bins, sel)
            assert np.array_equal(got["cols"], sel), tag
            same({k: whole[k][sel] for k in keys}, got, (tag, bins, "selection"), keys)
            V = rows[:, sel]
            if not np.all(np.isfinite(V).any(axis=0)):
                continue                                    # (n = 2 with -inf and +inf: no finite value to take a range from)
            lo = np.array([np.quantile(c[np.isfinite(c)], 0.25, method="inverted_cdf") for c in V.T])
            hi = np.array([np.quantile(c[np.isfinite(c)], 0.75, method="inverted_cdf") for c in V.T])
            if all(PR.range_ok(a, b) for a, b in zip(lo, hi)):
                same(PR.hist(V, bins, lo, hi), mt.hist(bins, sel, lo, hi), (tag, bins, "selection, explicit"), keys)


def check_hpd(tag, mt, rows):
    """Check 6, and check 8's scratch sizes and selection order for it."""
    n, nc = rows.shape
    masses = np.array([1.0 / n, 0.5, 0.95, 1.0])
    keys = ("k", "start", "lo", "hi")
    got = mt.hpd(masses)
    same(PR.hpd(rows, masses), got, tag, keys)
    P2 = 2
    while P2 < n:
        P2 *= 2
    per = 8 * P2 + 4 + 24 * masses.size
    same(got, mt.hpd(masses, None, 64 + per), (tag, "one column per chunk"), keys)
    same(got, mt.hpd(masses, None, 64 + 2 * per + 5), (tag, "two columns per chunk"), keys)
    rev = np.arange(nc - 1, -1, -1).astype(np.int32)
    same({k: got[k][:, rev] for k in keys[1:]}, mt.hpd(masses, rev, 64 + 3 * per), (tag, "reversed"), keys[1:])
    return got


def everything(mt, n, max_lag):
    """What check 8 compares between two tables."""
    out = {"result": mt.result(), "quantiles": mt.quantiles(QS), "hist": mt.hist(64)}
    if n >= 2:
        out["cov"] = {"cov": mt.cov(), "corr": mt.corr()}
    if n >= 4:
        out["ess"] = mt.ess(max_lag)
        out["ess"]["acov"] = mt.acov()
        out["rank"] = RS.snapshot(mt, max_lag)
        out["hpd"] = mt.hpd([1.0 / n, 0.5, 0.95, 1.0])
    return out


def same_everything(a, b, tag):
    assert a.keys() == b.keys(), tag
    for part in a:
        same(a[part], b[part], (tag, part), a[part].keys())


@pytest.mark.parametrize("name,n", CASES)
def test_column_kernels(accel_mod, name, n):
    w = CC.one_mode()
    v = CC.column(name, n)
    P = CC.plant(w, v)
    tag = (name, n)
    max_lag = 0 if n <= 257 else 31
    col = w["freq_cols"][0]
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, n) as mt, accel_mod.ModeTable(acc, n + 37) as mt2:
        rows = planted_rows(mt, w, P, [v])
        assert np.all(mt.push(P) == 0)
        res = mt.result()
        check_result(tag, name, res, rows)
        q = check_quantiles(tag, mt, rows)
        check_hist(tag, name, mt, res, rows, col)
        check_hist_selection(tag, mt, rows, selections(w, rows.shape[1]))
        if n >= 4:
            check_hpd(tag, mt, rows)
        else:
            with pytest.raises(accel_mod.AccelError) as e:       # the sort kernel's condition: n >= 4
                mt.hpd([0.5])
            assert e.value.code == accel_mod.capi.E_INVALID
        if n >= 2:
            cov = mt.cov()
            assert nan_eq(mt.corr(), tmd_corr(cov)) and np.array_equal(bits(cov), bits(cov.T)), tag
        if n >= 4:
            check_diag(tag, name, mt, rows, res, max_lag)
            assert np.isfinite(RR.median(v)), tag              # (the folded series needs a median: every set has one from n = 4)
            r = check_rank(tag, mt, rows, q, max_lag, sorted({0, col, col + 5, w["nu_cols"][0]}))
            per = accel_mod.capi.moderank_col_bytes(n, ER.lag_limit(max_lag, n))
            RS.same(RS.snapshot(mt, max_lag, None, per), r, (tag, "one column per chunk"))
            RS.same(RS.snapshot(mt, max_lag, None, 2 * per + 7), r, (tag, "two columns per chunk"))
            check_rank_selection(tag, mt, r, max_lag, selections(w, rows.shape[1]), 3 * per)
        # check 8: blocks of 29 into max_samples = n + 37
        for k0 in range(0, n, 29):
            assert np.all(mt2.push(P[k0:k0 + 29]) == 0)
        same_everything(everything(mt2, n, max_lag), everything(mt, n, max_lag), tag)


def increasing_map(v):
    """Strictly increasing on the distinct values of v: the smallest goes to -inf (-DBL_MAX if it is -inf already, which is then
    decreasing nowhere: the next value is finite), the largest to +inf, the rest stay."""
    g = v.copy()
    lo, hi = v.min(), v.max()
    g[v == lo] = -np.inf if np.isfinite(lo) else -CC.DBL_MAX
    g[v == hi] = np.inf if np.isfinite(hi) else CC.DBL_MAX
    return g


LAW = [("zeros-among", 257), ("neighbours", 4097), ("ties-twice", 64), ("scaled", 8193), ("denormals", 257), ("ties-halves", 64)]


@pytest.mark.parametrize("name,n", LAW)
def test_ranks_do_not_see_a_monotone_map(accel_mod, name, n):
    """Check 4's law: the two l = 0 modes carry v and g(v), g strictly increasing with the ends sent to +-inf."""
    w = CC.two_modes()
    v = CC.column(name, n)
    g = increasing_map(v)
    assert not np.array_equal(bits(v), bits(g)) and np.array_equal(RR.rank2(v), RR.rank2(g))
    a, b = w["freq_cols"]
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, n) as mt:
        planted_rows(mt, w, CC.plant(w, v, g), [v, g])
        mt.push(CC.plant(w, v, g))
        sa, sb = mt.rank_series(a), mt.rank_series(b)
        assert np.array_equal(sa["rank2"], sb["rank2"]) and np.array_equal(sa["rank2"], RR.rank2(v)), (name, n)
        for s in (0, 2, 3):                                   # z, I05, I95 (zfold depends on the values: |v - median|)
            assert np.array_equal(bits(sa["series"][s]), bits(sb["series"][s])), (name, n, RR.SERIES[s])
            assert bits(sa["mean"][s]) == bits(sb["mean"][s]), (name, n, RR.SERIES[s])
        r = RS.snapshot(mt, 0, [a, b])
        for k in ("ess_bulk", "tau_bulk", "rhat_bulk", "ess_q05", "ess_q95", "ess_tail"):
            assert nan_eq(r[k][0], r[k][1]), (name, n, k)
        assert np.array_equal(r["cut"][[0, 2, 3], 0], r["cut"][[0, 2, 3], 1]), (name, n)
        for s in ("z", "i05", "i95"):
            assert np.array_equal(bits(r["acov_" + s][:, 0]), bits(r["acov_" + s][:, 1])), (name, n, s)
        assert not np.any(np.isnan(r["ess_bulk"])) or name == "ties-equal"
    # -0 and +0 tie: one rank
    z = RR.rank2(CC.column("zeros-alt", 64))
    assert z.min() == z.max() == 65


PAIRS = [("span64", "neighbours"), ("infs-both", "ties-twice"), ("span64-inf", "zeros-among"), ("huge", "ties-halves"),
         ("denormals", "scaled"), ("zeros-alt", "ties-equal")]


@pytest.mark.parametrize("first,second", PAIRS)
@pytest.mark.parametrize("n", [64, 4097])
def test_pairs(accel_mod, first, second, n):
    """Check 7, and the covariance and correlation of two planted columns."""
    w = CC.two_modes()
    va, vb = CC.column(first, n), CC.column(second, n, seed=1)
    P = CC.plant(w, va, vb)
    a, b = w["freq_cols"]
    tag = (first, second, n)
    pairs = [[a, b], [b, a], [a, a], [b, b], [a, w["nu_cols"][1]], [0, a]]
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, n) as mt, accel_mod.ModeTable(acc, n + 37) as mt2:
        rows = planted_rows(mt, w, P, [va, vb])
        mt.push(P)
        for k0 in range(0, n, 29):
            mt2.push(P[k0:k0 + 29])
        keys = ("counts", "outside", "level", "status")
        for bins in (1, 2, 128):
            got = mt.hist2d(pairs, bins, mass=(0.5, 0.95))
            same(PR.hist2d(rows, pairs, bins, mass=(0.5, 0.95)), got, (tag, bins), keys)
            same(got, mt2.hist2d(pairs, bins, mass=(0.5, 0.95)), (tag, bins, "blocks"), keys)
            ok = got["status"] == 0
            assert np.all(got["counts"][ok].sum(axis=(1, 2)) + got["outside"][ok] == n) and np.all(got["counts"][~ok] == 0), (tag, bins)
            inf_a, inf_b = not PR.range_ok(va.min(), va.max()), not PR.range_ok(vb.min(), vb.max())
            assert list(got["status"]) == [int(inf_a or inf_b)] * 2 + [int(inf_a), int(inf_b), int(inf_a or inf_b), int(inf_a)], (tag, bins)
            if not inf_a:
                assert np.trace(got["counts"][2]) == n, (tag, bins, "a column with itself")
            # an explicit range over the finite values of both
            fa, fb = va[np.isfinite(va)], vb[np.isfinite(vb)]
            lo, hi = [fa.min(), fb.min()], [fa.max(), fb.max()]
            if PR.range_ok(lo[0], hi[0]) and PR.range_ok(lo[1], hi[1]):
                g = mt.hist2d([[a, b]], bins, lo, hi, mass=(0.5,))
                same(PR.hist2d(rows, [[a, b]], bins, lo, hi, mass=(0.5,)), g, (tag, bins, "explicit"), keys)
        res = mt.result()
        cov, corr = mt.cov([a, b, 0]), mt.corr([a, b, 0])
        assert nan_eq(corr, tmd_corr(cov)) and np.array_equal(bits(cov), bits(cov.T)), tag
        assert nan_eq(mt2.cov([a, b, 0]), cov) and nan_eq(mt.cov([0, b, a]), cov[::-1, ::-1]), tag
        sel = rows[:, [a, b, 0]]
        if first in FINITE_SUMS and second in FINITE_SUMS:
            d, e = DS.DR.centred(sel, res["mean"][[a, b, 0]])
            Sq, sb = DS.DR.cov_sums(d, e)
            sb = sb + DS.U * np.abs(Sq).astype(np.float64)
            serr = np.abs(cov.astype(np.longdouble) * (n - 1) - Sq).astype(np.float64)
            assert np.all(serr <= 10 * sb), (tag, serr, sb)
            if np.any(sb > 0):
                WORST["cov"] = max(WORST["cov"], float(np.max(serr[sb > 0] / sb[sb > 0])))
        else:
            _, pS = float64_diag_pattern(sel, res["mean"][[a, b, 0]], 0)
            with np.errstate(all="ignore"):
                assert np.array_equal(pattern(cov), pS), (tag, cov, pS)
            assert np.isnan(corr[0, 1]) and np.isnan(corr[0, 0]) and np.all(np.isnan(corr[2])), (tag, corr)


def test_zz_report():
    """Not a check: the line DESIGN.md quotes (run after the cases of this module)."""
    print("mode columns, worst error / bound: lag products %.3g, covariance sums %.3g (of 10), correlation %.3g, R-hat %.3g (of 1); "
          "ranks: z %.3g, lag products %.3g (of 10), R-hat %.3g" % (WORST["lag"], WORST["cov"], WORST["corr"], WORST["rhat"],
                                                                   RANK_WORST["z"], RANK_WORST["lag"], RANK_WORST["rhat"]))
