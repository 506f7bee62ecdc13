"""The mode table's diagnostics on the GPU (tamcmc_modediag_*, include/tamcmc_accel.h; ModeTable.ess / acov / cov / corr).

Rows: every relaxed parameter moves as its own AR(1) sequence around params_true (relative scale 0.002, phi from 0 to 0.95
over the parameters), so every sample stays TAMCMC_CHAIN_OK; a few skip entries and one NaN row are interleaved and must not
enter.  The series under test are the library's own derive rows of the accepted samples; the references are the numpy
statements of tests/modediag_reference.py and tests/ess_reference.py.

Layouts: a single l = 0 multiplet (13 columns), id 2 with lmax 1 and 3 orders (70 columns: more than one wave of the finish
kernel, more than two strips of the covariance kernel), the benchmark layout (277 columns, 9 strips, the last one partial).

Sizes: n in {4, 5, 63, 64, 65}; n on either side of the lag kernel's tile TM_MD_TILE = 1024 and of 2 TM_MD_TILE (the
covariance kernel's stage TM_MD_CS = 64 divides both, so these sit on its stage edges too); n = 1024 with L = 1023 = n - 1;
n = 1100 with L in {1, 3, 15, 17, 255, 1023} (one lag block of TM_MD_BLOCK_LAGS = 256 lags, then four; a lane's TM_MD_G = 4
lags cut by L); once n = 70 001 with L = 255 on the 13-column layout.

Checks, per case: (1) every result bit is the same for rows pushed at once into a table of max_samples = n, in blocks into
one of max_samples = n + 37, and one at a time; for a repeated call; for _ess after further pushes against a fresh object;
for cov over a permuted subset against the full matrix.  (2) result and quantiles are unchanged; cov is symmetric, its
diagonal is acov[0] / (n - 1), mcse is sd / sqrt(ess), constant columns give NaN, NaN, cut 0, rhat NaN and are counted.
(3) ess_reference.finish on the library's own acov gives the same cut and tau, ess bit for bit (4 ulp where tau sits on the
floor 1 / log10(n), for the host's log10, as the band-ESS suite allows); the totals recomputed from the arrays.  (4) lag
products and sums of products within 10 x the sensitivity bound of the long-double values, on the library's own rows and
mean (the factor 10 for the reason ess_reference's docstring gives).  (5) R-hat within 8 h 2^-52 relative of the long-double
formula: Welford's M2 of the centred values carries a relative error of order h u per half, and R-hat, a square root of a
ratio of positive sums, does not amplify it.  The worst ratios are printed by test_zz_report."""
import math

import numpy as np
import pytest

import ess_reference as ER
import modediag_reference as DR
import modetable_reference as MR
import workloads as W
from modediag_support import RHAT, U, WORST, check_against_references, check_rhat
from support import LD, bits
from tamcmc_amd import synth

pytestmark = pytest.mark.gpu

QS = np.array([0.0, 0.16, 0.5, 0.84, 1.0])
ARRAYS = ("ess", "tau", "mcse", "rhat", "cut")


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


def collect(mt, L, cols=None):
    r = mt.ess(L)
    r["acov"] = mt.acov()
    r["cov"] = mt.cov(cols)
    r["corr"] = mt.corr(cols)
    return r


def same(a, b, tag):
    assert a.keys() == b.keys(), tag
    for k in a:
        if isinstance(a[k], np.ndarray) and a[k].dtype == np.float64:
            assert np.array_equal(bits(a[k]), bits(b[k])), (tag, k)
        elif isinstance(a[k], float):
            assert bits(a[k]) == bits(b[k]), (tag, k)
        else:
            assert np.array_equal(a[k], b[k]), (tag, k)


CASES = [("one", n, 0) for n in (4, 5, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049)] + [("one", 1024, 1023)] + \
        [("one", 1100, L) for L in (1, 3, 15, 17, 255, 1023)] + \
        [("mid", 5, 0), ("mid", 65, 0), ("mid", 1025, 0), ("mid", 1100, 1023), ("mid", 2049, 17)] + \
        [("c2", 64, 0), ("c2", 1100, 255), ("c2", 2049, 17)]


@pytest.mark.parametrize("name,n,max_lag", CASES)
def test_diagnostics(accel_mod, name, n, max_lag):
    w = layout(name)
    P = ar1_params(w, n, seed=n + max_lag)
    Pin, skip = with_rejects(P)
    L = ER.lag_limit(max_lag, n)
    tag = (name, n, L)
    rng = np.random.default_rng(n)
    with open_acc(accel_mod, w) as acc:
        with accel_mod.ModeTable(acc, n) as mt, accel_mod.ModeTable(acc, n + 37) as mt2:
            rows, st = mt.derive(P)
            assert np.all(st == 0), tag
            st_in = mt.push(Pin, skip=skip)                      # at once
            assert np.array_equal(st_in != 0, np.isnan(Pin[:, 0])), tag
            res = mt.result()
            q = mt.quantiles(QS)["values"]
            assert res["n_used"] == n and res["n_rejected"] == len(Pin) - n, tag
            with pytest.raises(accel_mod.AccelError):
                mt.acov()                                        # no _ess call yet
            r = collect(mt, max_lag)
            # (2) the table's own results are untouched
            res2 = mt.result()
            for k in res:
                assert np.array_equal(bits(res[k]), bits(res2[k])) if isinstance(res[k], np.ndarray) else res[k] == res2[k], (tag, k)
            assert np.array_equal(bits(q), bits(mt.quantiles(QS)["values"])), tag
            same(collect(mt, max_lag), r, (tag, "repeated call"))
            check_against_references(tag, r, rows, res, L)
            # (1) in blocks, with another stride; then one at a time where that is short
            for k0 in range(0, len(Pin), 29):
                mt2.push(Pin[k0:k0 + 29], skip=skip[k0:k0 + 29])
            same(collect(mt2, max_lag), r, (tag, "blocks, max_samples = n + 37"))
            if n <= 1100:
                mt2.reset()
                with pytest.raises(accel_mod.AccelError):
                    mt2.acov()                                   # reset
                for k0 in range(len(Pin)):
                    mt2.push(Pin[k0:k0 + 1], skip=skip[k0:k0 + 1])
                same(collect(mt2, max_lag), r, (tag, "one at a time"))
            # a column subset in any order equals the matching entries of the full matrix
            nc = rows.shape[1]
            sel = rng.permutation(nc)[:max(1, min(nc - 1, 40))].astype(np.int32)
            for fn, full in ((mt.cov, r["cov"]), (mt.corr, r["corr"])):
                assert np.array_equal(bits(fn(sel)), bits(full[np.ix_(sel, sel)])), (tag, "subset")
            assert np.array_equal(bits(mt.cov([nc - 1])), bits(r["cov"][nc - 1:, nc - 1:])), tag
        # _ess after further pushes equals a fresh object holding all rows; acov is refused in between
        if n >= 8:
            with accel_mod.ModeTable(acc, n) as mt3:
                mt3.push(P[:n // 2])
                first = mt3.ess(max_lag)
                assert first["n_used"] == n // 2
                mt3.acov()
                mt3.push(P[n // 2:])
                with pytest.raises(accel_mod.AccelError) as e:
                    mt3.acov()
                assert e.value.code == accel_mod.capi.E_INVALID
                same(collect(mt3, max_lag), r, (tag, "after further pushes"))


@pytest.mark.parametrize("name,n,max_lag", CASES)
def test_rhat_against_long_double(accel_mod, name, n, max_lag):
    """Check 5 on the rows of the case of the same name (run here when that case has not run in this session).

    The library takes the halves' Welford moments of the centred values d_t (R-hat is unchanged by the shift): on the raw
    values the update of the mean rounds at the size of the mean, which on columns whose mean is 500 standard deviations (the
    inclination, the frequencies of these rows) costs M2 a relative mean / sd x 2^-53 whatever h is, and six cases with
    n <= 65 missed the bound by 1.2 x to 49 x."""
    tag = (name, n, ER.lag_limit(max_lag, n))
    if tag not in RHAT:
        w = layout(name)
        P = ar1_params(w, n, seed=n + max_lag)
        with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, n) as mt:
            rows, _ = mt.derive(P)
            mt.push(P)
            RHAT[tag] = (mt.ess(max_lag)["rhat"], rows)
    check_rhat(tag, *RHAT[tag])


def test_long_chain(accel_mod):
    """n = 70 001, L = 255 on the 13-column layout: 69 tiles of the lag kernel, 1094 stages of the covariance kernel."""
    n, w = 70001, layout("one")
    P = ar1_params(w, n, seed=77)
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, n + 37) as mt, accel_mod.ModeTable(acc, n) as mt2:
        rows, st = mt.derive(P)
        assert np.all(st == 0)
        for k0 in range(0, n, 4097):
            mt.push(P[k0:k0 + 4097])
        mt2.push(P)
        r, res = collect(mt, 255), mt.result()
        same(collect(mt2, 255), r, "at once")
        check_against_references(("one", n, 255), r, rows, res, 255)
        check_rhat(("one", n, 255), *RHAT[("one", n, 255)])


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
            for fn, a in ((mt.ess, ()), (mt.acov, ()), (mt.cov, ()), (mt.corr, ([0, 1],))):
                refused(fn, *a)
            assert mt.diag_kernel_time() == (0.0, 0)
        with accel_mod.ModeTable(acc, 12) as mt:
            refused(mt.ess); refused(mt.cov); refused(mt.corr)     # no row
            mt.push(P[:1])
            refused(mt.ess); refused(mt.cov)                       # n = 1
            mt.push(P[1:3])
            refused(mt.ess)                                        # n = 3 < 4
            assert mt.cov().shape == (13, 13)                      # n = 3 >= 2
            mt.push(P[3:])
            base = collect(mt, 0)
            for bad in (-1, 1024, 5000):
                refused(mt.ess, bad)
            for bad in ([], [13], [-1], [0, 0], [1, 2, 1], list(range(13)) + [0]):
                refused(mt.cov, bad); refused(mt.corr, bad)
            assert acc._lib.tamcmc_modediag_cov(mt._mt, 2, None, None) == E and acc._lib.tamcmc_modediag_acov(mt._mt, None) == E
            same(collect(mt, 0), base, "after the refusals")
            ms, launches = mt.diag_kernel_time()
            assert ms > 0.0 and launches == 2 * 4 + 1               # 2 collects of lag, finish, cov, cov; the cov at n = 3
            mt.reset()
            assert mt.diag_kernel_time() == (0.0, 0)
            refused(mt.acov); refused(mt.ess)


def test_known_ess_of_an_ar1_frequency(accel_mod):
    """An AR(1) sequence (phi = 0.8, 4000 samples) planted on one mode frequency: the freq column equals its params entry bit
    for bit, so its lag products are those of the sequence (check 4's bound) and its ESS lies within 15 % of
    n (1 - phi) / (1 + phi)."""
    n, phi = 4000, 0.8
    w = layout("mid")
    cols = MR.layout(2, w["plength"])
    c = int(np.flatnonzero(cols["param_index"] >= 0)[2])
    k = int(cols["param_index"][c])
    P = np.tile(w["params_true"], (n, 1))
    P[:, k] += ER.ar1(phi, n, 0.01, seed=1)
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, n) as mt:
        mt.push(P)
        r, res = mt.ess(255), mt.result()
        A = mt.acov()
    d, e = DR.centred(P[:, k:k + 1], res["mean"][c])
    Aq, bound = DR.lag(d, e, 255)
    err = np.abs(A[:, c].astype(LD) - Aq[:, 0]).astype(np.float64)
    assert np.all(err <= 10 * bound[:, 0])
    expect = n * (1 - phi) / (1 + phi)
    print(f"AR(1) phi 0.8 on a frequency: ess {r['ess'][c]:.1f}, expected {expect:.1f}; the sequence itself {ER.ess_of_sequence(P[:, k], 255)[1]:.1f}")
    assert abs(r["ess"][c] - expect) <= 0.15 * expect
    assert cols["l"][c] == 0 and bits(r["ess"][c + 7]) == bits(r["ess"][c])      # nu_m of an l = 0 mode is its frequency


def test_known_correlation_of_two_frequencies(accel_mod):
    """Two mode frequencies a + z1 and b + 0.6 z1 + 0.8 z2: their correlation is within the propagated bound of the
    long-double value and within 0.05 of 0.6."""
    n = 4000
    w = layout("mid")
    cols = MR.layout(2, w["plength"])
    ci, cj = (int(v) for v in np.flatnonzero(cols["param_index"] >= 0)[[1, 4]])
    ki, kj = int(cols["param_index"][ci]), int(cols["param_index"][cj])
    rng = np.random.default_rng(17)
    z1, z2 = 0.01 * rng.standard_normal(n), 0.01 * rng.standard_normal(n)
    P = np.tile(w["params_true"], (n, 1))
    P[:, ki] += z1
    P[:, kj] += 0.6 * z1 + 0.8 * z2
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, n) as mt:
        mt.push(P)
        res = mt.result()
        corr, cov = mt.corr([ci, cj]), mt.cov([cj, ci])
    d, e = DR.centred(P[:, [ki, kj]], res["mean"][[ci, cj]])
    Sq, sb = DR.cov_sums(d, e)
    rq, rb = DR.corr(Sq, 10 * (sb + U * np.abs(Sq).astype(np.float64)))
    print(f"corr of the two frequencies: {corr[0, 1]:.6f} (long double {float(rq[0, 1]):.6f})")
    assert abs(LD(corr[0, 1]) - rq[0, 1]) <= rb[0, 1] + 8 * U and abs(corr[0, 1] - 0.6) <= 0.05
    assert bits(corr[0, 1]) == bits(corr[1, 0]) and corr[0, 0] == corr[1, 1] == 1.0
    assert bits(cov[0, 1]) == bits(cov[1, 0]) and abs(LD(cov[1, 1]) * (n - 1) - Sq[0, 0]) <= 10 * (sb[0, 0] + U * float(Sq[0, 0]))


def test_known_rhat_of_a_shifted_half(accel_mod):
    """A chain whose second half is shifted by 3 sd in one parameter, the height of the single mode: rhat > 1.5 on the columns
    derived from it (height, amplitude, h_m), < 1.01 on every other column that moves, and n_rhat_high counts them."""
    n, scale = 4000, 0.002
    w = layout("one")
    cols = MR.layout(11, w["plength"])
    P = W.perturbed(w, n, scale=scale, seed=23)                # independent samples
    P[n // 2:, 0] += 3.0 * scale * w["params_true"][0]
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, n) as mt:
        rows, st = mt.derive(P)
        mt.push(P)
        r = mt.ess()
    assert np.all(st == 0)
    derived = np.isin(cols["kind"], [MR.K["height"], MR.K["amplitude"], MR.K["h_m"]])
    moving = rows.min(axis=0) != rows.max(axis=0)
    assert derived.sum() == 3 and np.all(moving[derived]) and (moving & ~derived).sum() >= 3
    print("rhat of the shifted chain: " + " ".join(f"{MR.KINDS[c['kind']]}={v:.4f}" for c, v in zip(cols, r["rhat"])))
    assert np.all(r["rhat"][derived] > 1.5) and np.all(r["rhat"][moving & ~derived] < 1.01) and np.all(np.isnan(r["rhat"][~moving]))
    assert r["n_rhat_high"] == 3 and r["col_max_rhat"] in np.flatnonzero(derived) and r["max_rhat"] == r["rhat"][derived].max()


def test_zz_report():
    """Not a check: the line README quotes (run after the cases of this module)."""
    print("modediag worst error / bound: lag products %.3g (of the 10 allowed), sums of products %.3g (of 10), correlations %.3g (of 1), "
          "R-hat %.3g (of 1)" % (WORST["lag"], WORST["cov"], WORST["corr"], WORST["rhat"]))
