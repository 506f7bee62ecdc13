"""The mode table's rank-normalised diagnostics on the GPU (tamcmc_moderank_*, include/tamcmc_accel.h; ModeTable.rank_diag /
rank_acov / rank_series).

Rows as in tests/test_modediag_gpu.py: AR(1) parameters around params_true, a NaN row and skipped rows interleaved; the
series under test are the library's own derive rows.  Layouts `one` (13 columns), `mid` (70), `c2` (277) of that file.

Sizes on the 13-column layout, L the default: 4, 5, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, and n - 1, n, n + 1 at every
threshold of the new kernels:
  * the number of slots P = the smallest power of two >= n, which sets the sorting network's pass count: n = 8, 16, 32, 128,
    256, 512, 4096 (64, 1024, 2048 are in the list above);
  * the sort kernel's tile and LDS-resident limit TM_MR_TILE = 8192: n = 8192 is the last column sorted entirely in LDS,
    8193 the first with a wide stage on the key buffer in device memory;
  * two and three wide stages: n = 16 384 and 32 768 (+- 1); 70 001 (once, L = 255) has four.
  The kernels have no 32-bit-key path (every column sorts 64-bit keys), so there is no such switch to straddle.
n = 1100 on the 70- and 277-column layouts with L in {1, 255, 1023}.  Tie cases: every row twice, one row fifty times, all rows
equal at n = 64.

Checks.  (1) exact: rank2 and rank2_fold against moderank_reference on the library's rows and its own f_t, their sums,
med / Q05 / Q95 against the sorted-row formula and ModeTable.quantiles, f_t, the indicators, the Welford means, and ess_tail,
rhat, cut, totals from the returned arrays.  (2) every bit the same for rows pushed at once, in blocks, one at a time;
max_samples n or n + 37; scratch for all columns, for exactly one, for two; all columns or a permuted subset; a repeated call;
after _ess / _cov calls; after further pushes against a fresh object; result, quantiles, ess and acov keep their bytes.
(3) |z - z_mp| <= 10 2^-50 q / phi(z_mp) + 4 2^-52 |z_mp| (every distinct rank2 for n <= 2049; 2000 drawn ones and both
extremes above), antisymmetry and +0 at rank2 = n + 1 bit for bit.  (4) lag products of the four series within 10 x
modediag_reference.lag's bound on the library's own series and means; ess_reference.finish on the library's own rank_acov
gives cut, tau, ess (4 ulp on the floor); R-hat within 8 h 2^-52 of the long-double formula on the library's centred series.
(5) planted sequences, (6) refusals.  test_zz_report prints the worst ratios.

Measured on the MI355X (this file's cases): see test_zz_report's line in README.md."""
import math

import numpy as np
import pytest

import ess_reference as ER
import modetable_reference as MR
import moderank_reference as RR
import workloads as W
from moderank_support import WORST, check_column, check_results, nan_eq, same, snapshot
from support import bits
from tamcmc_amd import synth

pytestmark = pytest.mark.gpu

QS = np.array([0.05, 0.95])


def one_mode():
    """id 11 (local) with a single l = 0 mode: heights, frequencies, 6 splitting entries, widths, white noise, inclination,
    trunc_c, do_amp -- 13 columns."""
    Nx = 1500
    x = synth.grid(Nx, 94.30, 40.0 / Nx)
    p = np.array([12.0, 110.2, 0.4, 0.0, 0.0, math.sqrt(0.4) * 0.5, math.sqrt(0.4) * math.sqrt(0.75), 0.0, 0.15, 0.8, 60.0, 20.0, 0.0])
    relax = np.array([1, 1, 0, 0, 0, 1, 1, 0, 1, 1, 0, 0, 0], dtype=np.int32)
    pl = np.array([1, 0, 1, 0, 0, 0, 6, 1, 1, 1, 2], dtype=np.int32)
    w = dict(model_case=11, plength=pl, params_true=p, x=x, index_to_relax=np.flatnonzero(relax).astype(np.int32), relax=relax)
    assert len(MR.layout(11, pl)) == 13
    return w


def layout(name):
    if name == "one":
        return one_mode()
    w = W.layout(2, lmax=1, Nmax=3) if name == "mid" else W.layout(2, 2, Nmax=7)
    assert len(MR.layout(2, w["plength"])) == {"mid": 70, "c2": 277}[name]
    return w


def ar1_params(w, n, seed, scale=0.002):
    """n params rows, relaxed parameter j an AR(1) sequence of its own around the true value"""
    idx = w["index_to_relax"]
    P = np.tile(w["params_true"], (n, 1))
    for j, k in enumerate(idx):
        P[:, k] *= 1.0 + ER.ar1(0.95 * j / max(len(idx) - 1, 1), n, scale, seed * 1000 + j)
    return P


def open_acc(accel_mod, w):
    return accel_mod.Accel(w["model_case"], w["plength"], w["x"], np.ones(w["x"].size))


def with_rejects(P, n_bad=3):
    """The rows with a NaN row and skipped rows interleaved: (rows, skip); the accepted rows are P, in order."""
    n = len(P)
    at = sorted({min(n, 1), n // 2, n})[:n_bad]                # positions in the accepted sequence before which a row goes in
    out, skip = [], []
    prev = 0
    for j, a in enumerate(at):
        out.append(P[prev:a]); skip.append(np.zeros(a - prev, dtype=np.int32))
        bad = P[-1].copy()                                     # a healthy row that must not enter: named by skip
        if j == 1:
            bad[0] = np.nan                                    # the NaN row (a height): status TAMCMC_CHAIN_NAN, no skip entry
        skip.append(np.full(1, int(j != 1), dtype=np.int32))
        out.append(bad[None, :])
        prev = a
    out.append(P[prev:]); skip.append(np.zeros(n - prev, dtype=np.int32))
    return np.concatenate(out), np.concatenate(skip)


def run_case(accel_mod, name, n, max_lag, P=None, n_series=None):
    w = layout(name)
    if P is None:
        P = ar1_params(w, n, seed=n + max_lag)
    Pin, skip = with_rejects(P)
    L = ER.lag_limit(max_lag, n)
    tag = (name, n, L)
    rng = np.random.default_rng(n)
    per = accel_mod.capi.moderank_col_bytes(n, L)
    with open_acc(accel_mod, w) as acc:
        with accel_mod.ModeTable(acc, n) as mt, accel_mod.ModeTable(acc, n + 37) as mt2:
            rows, st = mt.derive(P)
            assert np.all(st == 0), tag
            mt.push(Pin, skip=skip)
            nc = rows.shape[1]
            res, q, cl = mt.result(), mt.quantiles(QS)["values"], mt.ess(max_lag)
            cl_acov = mt.acov()
            assert res["n_used"] == n, tag
            with pytest.raises(accel_mod.AccelError):
                mt.rank_acov(0)                                  # no _diag call yet
            r = snapshot(mt, max_lag)
            # the table's and the classic diagnostics' results are untouched
            res2 = mt.result()
            for k in res:
                assert np.array_equal(bits(res[k]), bits(res2[k])) if isinstance(res[k], np.ndarray) else res[k] == res2[k], (tag, k)
            assert np.array_equal(bits(q), bits(mt.quantiles(QS)["values"])) and np.array_equal(bits(cl_acov), bits(mt.acov())), tag
            cl2 = mt.ess(max_lag)
            same(cl2, cl, (tag, "the classic diagnostics"))
            mt.cov([0, 1])
            same(snapshot(mt, max_lag), r, (tag, "repeated call, after _ess and _cov"))
            # checks 1, 3, 4 against the references
            const = np.flatnonzero(rows.min(axis=0) == rows.max(axis=0))
            pickc = np.arange(nc) if n_series is None or n_series >= nc else np.unique(np.concatenate([const[:2], rng.permutation(nc)[:n_series]]))
            series_of = {int(c): check_column(tag, mt, int(c), rows[:, c], n, q, rng) for c in pickc}
            assert const.size >= 1 and r["n_constant"] == const.size, tag
            check_results(tag, r, n, L, series_of)
            # (2) scratch for one column, for two (a partial last chunk when n_sel is odd); a permuted subset
            same(snapshot(mt, max_lag, None, per), r, (tag, "one column per chunk"))
            same(snapshot(mt, max_lag, None, 2 * per + 7), r, (tag, "two columns per chunk"))
            sel = rng.permutation(nc)[:max(1, min(nc - 1, 41))].astype(np.int32)
            sub = snapshot(mt, max_lag, sel, 3 * per)
            assert np.array_equal(sub["cols"], sel), tag
            for k in RR.OUT:
                assert nan_eq(sub[k], r[k][sel]), (tag, "subset", k)
            assert np.array_equal(sub["cut"], r["cut"][:, sel]), tag
            for s in RR.SERIES:
                assert np.array_equal(bits(sub["acov_" + s]), bits(r["acov_" + s][:, sel])), (tag, "subset", s)
            # in blocks into max_samples = n + 37; one at a time where that is short
            for k0 in range(0, len(Pin), 29):
                mt2.push(Pin[k0:k0 + 29], skip=skip[k0:k0 + 29])
            same(snapshot(mt2, max_lag), r, (tag, "blocks, max_samples = n + 37"))
            if n <= 1100:
                mt2.reset()
                with pytest.raises(accel_mod.AccelError):
                    mt2.rank_acov(0)
                for k0 in range(len(Pin)):
                    mt2.push(Pin[k0:k0 + 1], skip=skip[k0:k0 + 1])
                same(snapshot(mt2, max_lag), r, (tag, "one at a time"))
        if n >= 8:
            with accel_mod.ModeTable(acc, n) as mt3:
                mt3.push(P[:n // 2])
                assert mt3.rank_diag(max_lag)["n_used"] == n // 2
                mt3.rank_acov(1)
                mt3.push(P[n // 2:])
                with pytest.raises(accel_mod.AccelError) as e:
                    mt3.rank_acov(1)
                assert e.value.code == accel_mod.capi.E_INVALID
                same(snapshot(mt3, max_lag), r, (tag, "after further pushes"))


BASE = (4, 5, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049)
EDGES = tuple(p + d for p in (8, 16, 32, 128, 256, 512, 4096) for d in (-1, 0, 1))
WIDE = tuple(p + d for p in (8192, 16384, 32768) for d in (-1, 0, 1))


@pytest.mark.parametrize("n", BASE + EDGES)
def test_sizes(accel_mod, n):
    run_case(accel_mod, "one", n, 0)


@pytest.mark.parametrize("n", WIDE)
def test_sizes_past_the_tile(accel_mod, n):
    """One, two and three wide stages of the sort kernel; the long-double lag products on three columns."""
    run_case(accel_mod, "one", n, 0, n_series=3)


@pytest.mark.parametrize("name,max_lag", [(nm, L) for nm in ("mid", "c2") for L in (1, 255, 1023)])
def test_layouts(accel_mod, name, max_lag):
    run_case(accel_mod, name, 1100, max_lag, n_series=10)


def test_long_chain(accel_mod):
    """n = 70 001, L = 255 on the 13-column layout: 131 072 slots, four wide stages."""
    run_case(accel_mod, "one", 70001, 255, n_series=3)


@pytest.mark.parametrize("kind", ["twice", "fifty", "equal"])
def test_ties(accel_mod, kind):
    w = layout("one")
    if kind == "twice":
        P = np.repeat(ar1_params(w, 150, seed=5), 2, axis=0)
    elif kind == "fifty":
        P = ar1_params(w, 300, seed=6)
        P = np.concatenate([P[:100], np.repeat(P[100:101], 50, axis=0), P[101:]])
    else:
        P = np.repeat(ar1_params(w, 1, seed=7), 64, axis=0)
    n = len(P)
    if kind != "equal":
        run_case(accel_mod, "one", n, 0, P=P)
        return
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, n) as mt:
        rows, _ = mt.derive(P)
        mt.push(P)
        q = mt.quantiles(QS)["values"]
        r = snapshot(mt, 0)
        rng = np.random.default_rng(1)
        series_of = {c: check_column((kind, n), mt, c, rows[:, c], n, q, rng) for c in range(mt.n_cols)}
        check_results((kind, n), r, n, ER.lag_limit(0, n), series_of)
        assert r["n_constant"] == mt.n_cols and r["col_max_rhat"] == -1 and np.isnan(r["min_ess_bulk"]) and np.isnan(r["min_ess_tail"])
        for k in RR.OUT:
            assert np.all(np.isnan(r[k])), k
        for s in series_of.values():
            assert np.all(bits(s["series"][:2]) == 0) and np.all(s["series"][2:] == 1.0)


def planted(accel_mod, seq, scale=0.001):
    """seq (n values) on the frequency parameter of the 13-column layout's mode, held to checks 1-4; (rank_diag, classic ess, column)"""
    n = len(seq)
    w = layout("one")
    cols = MR.layout(11, w["plength"])
    c = int(np.flatnonzero(cols["param_index"] >= 0)[0])
    k = int(cols["param_index"][c])
    P = np.tile(w["params_true"], (n, 1))
    P[:, k] += scale * np.asarray(seq)
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, n) as mt:
        rows, st = mt.derive(P)
        mt.push(P)
        res, q = mt.result(), mt.quantiles(QS)["values"]
        assert res["n_rejected"] == 0 and np.all(st == 0) and np.array_equal(bits(rows[:, c]), bits(P[:, k]))
        r, cl = snapshot(mt, 255), mt.ess(255)
        rng = np.random.default_rng(2)
        series_of = {cc: check_column(("planted", n), mt, cc, rows[:, cc], n, q, rng) for cc in (c, 0)}
        check_results(("planted", n), r, n, 255, series_of)
    return r, cl, c


def test_planted_scale_change(accel_mod):
    """N(0, 1) whose second half is three times as wide: the classic diagnostics pass it, the folded R-hat and the tail ESS do not."""
    n = 4000
    x = np.random.default_rng(1).standard_normal(n)
    x[n // 2:] *= 3.0
    r, cl, c = planted(accel_mod, x)
    print(f"scale change: classic ess {cl['ess'][c]:.1f} rhat {cl['rhat'][c]:.4f}; rhat_fold {r['rhat_fold'][c]:.4f}, ess_tail {r['ess_tail'][c]:.1f}")
    assert cl["rhat"][c] < 1.01 and r["rhat_fold"][c] > 1.1 and r["ess_tail"][c] < 0.2 * cl["ess"][c]


def test_planted_cauchy_shift(accel_mod):
    """iid Cauchy (clipped at +-1000 scale units) whose second half is shifted by one scale unit."""
    n = 4000
    x = np.clip(np.random.default_rng(1).standard_cauchy(n), -1000.0, 1000.0)
    x[n // 2:] += 1.0
    r, cl, c = planted(accel_mod, x)
    print(f"Cauchy shift: classic ess {cl['ess'][c]:.1f} rhat {cl['rhat'][c]:.4f}; rhat_bulk {r['rhat_bulk'][c]:.4f}, ess_bulk {r['ess_bulk'][c]:.1f}")
    assert cl["rhat"][c] < 1.01 and r["rhat_bulk"][c] > 1.03 and r["ess_bulk"][c] < 0.2 * cl["ess"][c]


def test_planted_ar1_control(accel_mod):
    """Gaussian AR(1), phi = 0.8: the bulk ESS agrees with the classic one."""
    r, cl, c = planted(accel_mod, ER.ar1(0.8, 4000, 1.0, seed=1))
    print(f"AR(1) control: classic ess {cl['ess'][c]:.1f}, ess_bulk {r['ess_bulk'][c]:.1f}")
    assert abs(r["ess_bulk"][c] - cl["ess"][c]) <= 0.05 * cl["ess"][c]


def test_refusals(accel_mod):
    """The refusals of the header on a live object; a refused call changes nothing."""
    E = accel_mod.capi.E_INVALID
    w = layout("one")
    P = ar1_params(w, 12, seed=5)

    def refused(fn, *a):
        with pytest.raises(accel_mod.AccelError) as e:
            fn(*a)
        assert e.value.code == E, (fn, a)

    with open_acc(accel_mod, w) as acc:
        with accel_mod.ModeTable(acc, 0) as mt:                  # statistics only: no table to work on
            mt.push(P)
            refused(mt.rank_diag); refused(mt.rank_acov, 0); refused(mt.rank_series, 0)
            assert mt.rank_kernel_time() == (0.0, 0)
        with accel_mod.ModeTable(acc, 12) as mt:
            refused(mt.rank_diag)                                  # no row
            mt.push(P[:3])
            refused(mt.rank_diag); refused(mt.rank_series, 0)      # n = 3 < 4
            mt.push(P[3:])
            refused(mt.rank_acov, 0)                               # no _diag yet
            base = snapshot(mt, 0)
            per12 = accel_mod.capi.moderank_col_bytes(12, base["lag"])
            for bad in (-1, 1024, 5000):
                refused(mt.rank_diag, bad)
            for bad in ([], [13], [-1], [0, 0], [1, 2, 1], list(range(13)) + [0]):
                refused(mt.rank_diag, 0, bad)
            refused(mt.rank_diag, 0, None, -1)
            refused(mt.rank_acov, 4); refused(mt.rank_acov, -1); refused(mt.rank_series, 13); refused(mt.rank_series, -1)
            assert acc._lib.tamcmc_moderank_acov(mt._mt, 0, None) == E
            assert acc._lib.tamcmc_moderank_diag(mt._mt, 0, 14, None, 0, None, None, None) == E
            # a batch in flight, then a batch armed, on the table's context: every entry point is refused
            T = np.ones(len(P))
            for enter, leave in ((lambda: acc.begin(P, T), acc.end), (lambda: acc.arm(len(P)), acc.disarm)):
                enter()
                refused(mt.rank_diag); refused(mt.rank_diag, 0, [0, 1], per12)
                refused(mt.rank_acov, 0); refused(mt.rank_series, 0); refused(mt.rank_kernel_time)
                leave()
            for s, name in enumerate(RR.SERIES):                   # the last result is still there, unchanged
                assert np.array_equal(bits(mt.rank_acov(s)), bits(base["acov_" + name]))
            same(snapshot(mt, 0), base, "after the refusals")
            ms, launches = mt.rank_kernel_time()
            assert ms > 0.0 and launches == 2 * 6                   # 2 snapshots of sort, sort, transform, mean, lag, finish
            mt.reset()
            assert mt.rank_kernel_time() == (0.0, 0)
            refused(mt.rank_acov, 0); refused(mt.rank_diag)


def test_zz_report():
    """Not a check: the line README quotes (run after the cases of this module)."""
    print("moderank worst error / bound: z %.3g (of 1), lag products %.3g (of the 10 allowed), R-hat %.3g (of 1)"
          % (WORST["z"], WORST["lag"], WORST["rhat"]))
