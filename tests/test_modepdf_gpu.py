"""The mode table's marginal histograms, shortest (HPD) intervals and pair densities on the GPU (tamcmc_modepdf_*,
include/tamcmc_accel_pdf.h; ModeTable.hist / hpd / hist2d).

Rows as in tests/test_moderank_gpu.py: AR(1) parameters around params_true, a NaN row and skipped rows interleaved; the
columns under test are the library's own derive rows.  Layouts `one` (13 columns), `mid` (70), `c2` (277), and `g3-5` with
the seismic indices enabled.  Every output is an integer count or an order statistic, so every comparison with
modepdf_reference is for equality, doubles bit for bit.

  hist     n = 1, 2, 255, 256, 257, 4097, 20 000 (below, at and above one sweep of the 512 x 4 loads of a workgroup; several
           sweeps), n_bins = 1, 2, 63, 64, 65, 4096, default ranges and explicit ones that cut both tails; the constant
           splitting column of the l = 0 mode; an integer window-edge column with n_bins = hi - lo; a column planted on a
           dyadic lattice (np.histogram agrees); a seismic index at +-inf (status 1, no count).  (The 13-column layout's
           window spans its whole grid; the window edges that move along the chain are those of the 70- and 277-column ones.)
  hpd      n = 4, 5, 8191, 8192, 8193, 16 385 (both sides of the sort's LDS tile), masses 1 / n, 0.5, 0.68, 0.95, 1; every row
           twice, one row fifty times, all rows equal; the integer columns have many tied widths; the planted one-sided column.
  hist2d   n_bins = 1, 2, 127, 128; 1, 3, 70 pairs; a column with itself, a repeated pair; row and column sums; levels.
  then independence of pushes, max_samples, selection and scratch; the other results keep their bytes; refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import ess_reference as ER
import modepdf_reference as PR
import modetable_reference as MR
import workloads as W
from support import bits
from tamcmc_amd import synth

pytestmark = pytest.mark.gpu

MASSES = (0.5, 0.68, 0.95, 1.0)
BINS = (1, 2, 63, 64, 65, 4096)


def one_mode():
    """id 11 (local) with a single l = 0 mode (tests/test_moderank_gpu.py): 13 columns."""
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
    if name == "g3-5":
        return W.layout(2, lmax=3, Nmax=5)
    w = W.layout(2, lmax=1, Nmax=3) if name == "mid" else W.layout(2, 2, Nmax=7)
    assert len(MR.layout(2, w["plength"])) == {"mid": 70, "c2": 277}[name]
    return w


def ar1_params(w, n, seed, scale=0.002):
    idx = w["index_to_relax"]
    P = np.tile(w["params_true"], (n, 1))
    for j, k in enumerate(idx):
        P[:, k] *= 1.0 + ER.ar1(0.95 * j / max(len(idx) - 1, 1), n, scale, seed * 1000 + j)
    return P


def with_rejects(P):
    """(rows, skip): P with a skipped row in front, a NaN row in the middle and a skipped row at the end."""
    n = len(P)
    bad = P[-1].copy()
    nan = bad.copy()
    nan[0] = np.nan
    rows = np.concatenate([bad[None], P[:n // 2], nan[None], P[n // 2:], bad[None]])
    skip = np.zeros(len(rows), dtype=np.int32)
    skip[0] = skip[-1] = 1
    return rows, skip


def open_acc(accel_mod, w):
    return accel_mod.Accel(w["model_case"], w["plength"], w["x"], np.ones(w["x"].size))


def same(a, b, tag, keys=None):
    for k in (keys or a.keys()):
        if a[k].dtype == np.float64:
            assert np.array_equal(bits(a[k]), bits(b[k])), (tag, k)
        else:
            assert np.array_equal(a[k], b[k]), (tag, k)


def cut_ranges(rows):
    """explicit ranges that cut both tails: the middle half of min ... max (a constant column keeps hi = lo)"""
    mn, mx = rows.min(axis=0), rows.max(axis=0)
    return mn + 0.25 * (mx - mn), mx - 0.25 * (mx - mn)


def check_hist(tag, mt, rows, bins, cols=None, lo=None, hi=None):
    n = len(rows)
    got = mt.hist(bins, cols, lo, hi)
    V = rows if cols is None else rows[:, cols]
    want = PR.hist(V, bins, lo, hi)
    same(want, got, (tag, bins), ("counts", "below", "above", "range", "status"))
    ok = got["status"] == 0
    assert np.all(got["counts"][ok].sum(axis=1) + got["below"][ok] + got["above"][ok] == n), (tag, bins)
    assert np.all(got["counts"][~ok] == 0) and np.all(got["below"][~ok] == 0) and np.all(got["above"][~ok] == 0), (tag, bins)
    return got


def filled(accel_mod, acc, P):
    """a table of len(P) rows holding P, pushed with a NaN row and skipped rows among them"""
    mt = accel_mod.ModeTable(acc, len(P))
    Pin, skip = with_rejects(P)
    st = mt.push(Pin, skip=skip)
    assert mt.result()["n_used"] == len(P) and st[1 + len(P) // 2] != 0
    return mt


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097, 20000])
def test_hist_sizes(accel_mod, n):
    w = layout("one")
    P = ar1_params(w, n, seed=n)
    cols = MR.layout(11, w["plength"])
    with open_acc(accel_mod, w) as acc, filled(accel_mod, acc, P) as mt:
        rows, st = mt.derive(P)
        assert np.all(st == 0)
        res = mt.result()
        lo, hi = cut_ranges(rows)
        const = np.flatnonzero(cols["kind"] == MR.K["splitting"])
        assert np.all(rows[:, const] == rows[0, const])                   # the splitting of the l = 0 mode
        for bins in BINS:
            h = check_hist(("default", n), mt, rows, bins)
            assert np.array_equal(bits(h["range"][:, 0]), bits(res["min"])) and np.array_equal(bits(h["range"][:, 1]), bits(res["max"]))
            assert np.all(h["below"] == 0) and np.all(h["above"] == 0) and np.all(h["status"] == 0)
            assert np.all(h["counts"][const, 0] == n) and h["counts"][const].sum() == n * const.size
            hc = check_hist(("cut", n), mt, rows, bins, None, lo, hi)
            if n >= 255:
                vary = rows.min(axis=0) < rows.max(axis=0)
                assert np.all(hc["below"][vary] > 0) and np.all(hc["above"][vary] > 0)
        assert mt.pdf_kernel_time()[1] == 2 * len(BINS)


@pytest.mark.parametrize("name", ["mid", "c2"])
def test_hist_layouts(accel_mod, name):
    w = layout(name)
    n = 1100
    P = ar1_params(w, n, seed=3)
    with open_acc(accel_mod, w) as acc, filled(accel_mod, acc, P) as mt:
        rows, _ = mt.derive(P)
        lo, hi = cut_ranges(rows)
        for bins in (50, 4096):
            check_hist((name, "default"), mt, rows, bins)
            check_hist((name, "cut"), mt, rows, bins, None, lo, hi)
        sel = np.random.default_rng(1).permutation(rows.shape[1])[:41].astype(np.int32)
        check_hist((name, "subset"), mt, rows, 64, sel, lo[sel], hi[sel])
        # the integer window-edge columns that move along the chain, one class per integer (n_bins = hi - lo)
        edge = moving_edges(w, rows)
        for c in edge[:6]:
            v = rows[:, c]
            nb = int(v.max() - v.min())
            h = check_hist((name, "edge", c), mt, rows, nb, [c])
            want = np.bincount((v - v.min()).astype(np.int64), minlength=nb + 1)
            want[nb - 1] += want[nb]
            assert np.array_equal(h["counts"][0], want[:nb]), (name, c)
        # intervals of every column; on the integer columns many widths tie and the first index wins
        masses = [1.0 / n, 0.5, 0.68, 0.95, 1.0]
        got = mt.hpd(masses)
        same(PR.hpd(rows, masses), got, (name, "hpd"), ("k", "start", "lo", "hi"))
        for c in edge[:6]:
            s = np.sort(rows[:, c])
            k = int(got["k"][2])
            wd = s[k - 1:] - s[:n - k + 1]
            assert np.sum(wd == wd.min()) > 1 and got["start"][2, c] == int(np.flatnonzero(wd == wd.min())[0]), (name, c)


def moving_edges(w, rows):
    """the window_lo / window_hi columns (integers) that take at least 3 and at most 4097 values' span along the chain"""
    cols = MR.layout(w["model_case"], w["plength"])
    edge = np.flatnonzero((cols["kind"] == MR.K["window_lo"]) | (cols["kind"] == MR.K["window_hi"]))
    assert np.all(rows[:, edge] == np.floor(rows[:, edge]))
    span = rows[:, edge].max(axis=0) - rows[:, edge].min(axis=0)
    edge = [int(c) for c, d in zip(edge, span) if 2 <= d <= 4096]
    assert len(edge) >= 1, "a window edge moves along the chain"
    return edge


def planted_freq(accel_mod, values):
    """values on the frequency parameter of the 13-column layout's mode: (acc, mt, column, rows) -- the caller closes both"""
    w = layout("one")
    cols = MR.layout(11, w["plength"])
    c = int(np.flatnonzero(cols["param_index"] >= 0)[0])
    k = int(cols["param_index"][c])
    P = np.tile(w["params_true"], (len(values), 1))
    P[:, k] = values
    acc = open_acc(accel_mod, w)
    mt = accel_mod.ModeTable(acc, len(values))
    rows, st = mt.derive(P)
    mt.push(P)
    assert np.all(st == 0) and np.array_equal(bits(rows[:, c]), bits(P[:, k]))
    return acc, mt, c, rows


def test_hist_dyadic_lattice(accel_mod):
    """Values j / 64 above 110, j = 0 ... 64 all present: every edge of 64 classes over [110, 111] is hit exactly; the counts
    are np.histogram's, for the default range (the same numbers) and the explicit one; 32 and 128 classes as well."""
    rng = np.random.default_rng(4)
    j = np.concatenate([np.arange(65), rng.integers(0, 65, 900)])
    v = 110.0 + rng.permutation(j) / 64.0
    acc, mt, c, rows = planted_freq(accel_mod, v)
    with acc, mt:
        for bins in (32, 64, 128):
            want = np.histogram(v, bins=bins, range=(110.0, 111.0))[0]
            for lo, hi in ((None, None), ([110.0], [111.0])):
                h = check_hist("lattice", mt, rows, bins, [c], lo, hi)
                assert np.array_equal(h["counts"][0], want) and list(h["range"][0]) == [110.0, 111.0]
            assert np.array_equal(bits(mt.hist_edges(h["range"][0], bins)), bits(110.0 + np.arange(bins + 1) / bins))
        h = check_hist("lattice", mt, rows, 16, [c], [110.25], [110.75])
        assert np.array_equal(h["counts"][0], np.histogram(v, bins=16, range=(110.25, 110.75))[0])
        assert h["below"][0] == np.sum(v < 110.25) and h["above"][0] == np.sum(v > 110.75)


def indices_table(accel_mod, acc, w, n, n_inf):
    """a table with the seismic indices enabled; n_inf of its n rows have two equal radial frequencies: some ratio is +-inf"""
    cols = MR.layout(2, w["plength"])
    f0 = cols["param_index"][(cols["kind"] == MR.K["freq"]) & (cols["l"] == 0)]
    P = ar1_params(w, n, seed=9, scale=0.0005)
    for t in range(n_inf):
        P[3 + 2 * t, f0[3]] = P[3 + 2 * t, f0[2]]
    mt = accel_mod.ModeTable(acc, n)
    mt.enable_indices(w["params_true"])
    rows, st = mt.derive(P)
    assert np.all(st == 0)
    mt.push(P)
    return mt, rows


def test_hist_index_at_infinity(accel_mod):
    w = layout("g3-5")
    n = 300
    with open_acc(accel_mod, w) as acc:
        mt, rows = indices_table(accel_mod, acc, w, n, 3)
        with mt:
            inf = np.flatnonzero(np.isinf(rows).any(axis=0))
            nb = len(MR.layout(2, w["plength"]))
            assert inf.size >= 1 and np.all(inf >= nb) and mt.n_cols == rows.shape[1] > nb
            for bins in (1, 50):
                h = check_hist("indices", mt, rows, bins)
                assert np.array_equal(np.flatnonzero(h["status"]), inf) and np.all(h["counts"][inf] == 0)
            # a finite explicit range: the infinite values are below or above it
            fin = np.where(np.isinf(rows), np.nan, rows)
            lo, hi = np.nanmin(fin, axis=0), np.nanmax(fin, axis=0)
            h = check_hist("indices, explicit", mt, rows, 50, None, lo, hi)
            assert np.all(h["status"] == 0) and np.array_equal((h["below"] + h["above"])[inf], np.isinf(rows[:, inf]).sum(axis=0))
            # the index columns behave like any other column: intervals (inf - inf is a NaN width) and pairs
            r = mt.hpd([1.0 / n, 0.5, 1.0], inf)
            same(PR.hpd(rows[:, inf], [1.0 / n, 0.5, 1.0]), r, "indices hpd", ("k", "start", "lo", "hi"))
            assert np.all(np.isinf(r["lo"][2]) | np.isinf(r["hi"][2]))
            pairs = [[int(inf[0]), 0], [nb, nb + 1], [int(inf[0]), int(inf[0])]]
            j = mt.hist2d(pairs, 16, mass=(0.68, 0.95))
            same(PR.hist2d(rows, pairs, 16, mass=(0.68, 0.95)), j, "indices hist2d", ("counts", "outside", "level", "status"))
            assert list(j["status"]) == [1, 0, 1] and j["counts"][0].sum() == 0 and j["counts"][1].sum() == n


def hpd_case(accel_mod, tag, P, extra_mass=()):
    w = layout("one")
    n = len(P)
    masses = np.array((1.0 / n,) + MASSES + tuple(extra_mass))
    with open_acc(accel_mod, w) as acc, filled(accel_mod, acc, P) as mt:
        rows, _ = mt.derive(P)
        res = mt.result()
        got = mt.hpd(masses)
        want = PR.hpd(rows, masses)
        same(want, got, tag, ("k", "start", "lo", "hi"))
        assert got["k"][0] == 1 and got["k"][-1 - len(extra_mass)] == n and np.all(got["start"][0] == 0) and np.all(got["lo"][0] == got["hi"][0])
        full = len(MASSES)                                                  # mass 1: the table's min and max
        assert np.all(got["start"][full] == 0) and np.all(got["lo"][full] == res["min"]) and np.all(got["hi"][full] == res["max"])
        assert not np.any(np.signbit(got["lo"][full][res["min"] == 0.0]))
        # one column per chunk; two and a partial chunk; a reversed selection
        P2 = 2
        while P2 < n:
            P2 *= 2
        per = 8 * P2 + 4 + 24 * masses.size
        same(got, mt.hpd(masses, None, 64 + per), (tag, "one column per chunk"), ("k", "start", "lo", "hi"))
        same(got, mt.hpd(masses, None, 64 + 2 * per + 5), (tag, "two columns per chunk"), ("k", "start", "lo", "hi"))
        rev = np.arange(rows.shape[1] - 1, -1, -1).astype(np.int32)
        r = mt.hpd(masses, rev, 64 + 3 * per)
        same({k: got[k][:, rev] for k in ("start", "lo", "hi")}, r, (tag, "reversed"), ("start", "lo", "hi"))
        return got, rows


@pytest.mark.parametrize("n", [4, 5, 8191, 8192, 8193, 16385])
def test_hpd_sizes(accel_mod, n):
    w = layout("one")
    hpd_case(accel_mod, ("sizes", n), ar1_params(w, n, seed=n))


@pytest.mark.parametrize("kind", ["twice", "fifty", "equal"])
def test_hpd_ties(accel_mod, kind):
    w = layout("one")
    if kind == "twice":
        P = np.repeat(ar1_params(w, 150, seed=5), 2, axis=0)
    elif kind == "fifty":
        P = ar1_params(w, 300, seed=6)
        P = np.concatenate([P[:100], np.repeat(P[100:101], 50, axis=0), P[101:]])
    else:
        P = np.repeat(ar1_params(w, 1, seed=7), 64, axis=0)
    got, rows = hpd_case(accel_mod, kind, P, extra_mass=(49.5 / len(P),))
    if kind == "equal":
        assert np.all(got["start"] == 0) and np.all(got["lo"] == got["hi"]) and np.all(got["lo"] == rows[0] + 0.0)
    if kind == "fifty":                                # a window of fifty fits the fifty equal rows: width 0
        cont = np.array([np.unique(rows[:, c]).size == len(P) - 49 for c in range(rows.shape[1])])     # no other tie in the column
        assert cont.sum() >= 3 and got["k"][-1] == 50
        assert np.all((got["hi"][-1] - got["lo"][-1])[cont] == 0.0) and np.all(got["lo"][-1][cont] == rows[100, cont])


def test_hpd_planted_one_sided(accel_mod):
    """a1 = 0.4 |N(0, 1)| on the splitting of the 70-column layout (a1 = p[s + 3]^2 + p[s + 4]^2 of id 2): a marginal piled
    up against 0.  Its 68 % HPD starts at the column's minimum and is shorter than the 16 - 84 % quantile interval.  (Of a
    finite sample of a half-normal the shortest window starts exactly at the minimum in about 4 draws of 10 and within a few
    order statistics of it otherwise: the density is flat at 0.  Seed 1 is a draw that does, as the numpy restatement shows
    without the library.)"""
    w = layout("mid")
    n = 4000
    s = int(w["plength"][:6].sum())
    a = 0.4 * np.abs(np.random.default_rng(1).standard_normal(n))
    ang = math.atan2(w["params_true"][s + 4], w["params_true"][s + 3])
    P = np.tile(w["params_true"], (n, 1))
    P[:, s + 3], P[:, s + 4] = np.sqrt(a) * math.cos(ang), np.sqrt(a) * math.sin(ang)
    cols = MR.layout(2, w["plength"])
    c = int(np.flatnonzero((cols["kind"] == MR.K["splitting"]) & (cols["l"] == 1))[0])
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, n) as mt:
        rows, st = mt.derive(P)
        mt.push(P)
        v = rows[:, c]
        assert np.all(st == 0) and np.all(np.abs(v - a) <= 16 * 2.0 ** -52 * a)
        r = mt.hpd([0.68], [c])
        same(PR.hpd(v[:, None], [0.68]), r, "planted", ("k", "start", "lo", "hi"))
        q = mt.quantiles([0.16, 0.84])["values"][:, c]
        print(f"one-sided splitting: 68 % HPD [{r['lo'][0, 0]:.6f}, {r['hi'][0, 0]:.6f}] (width {r['hi'][0, 0] - r['lo'][0, 0]:.6f}); "
              f"16 - 84 % quantiles [{q[0]:.6f}, {q[1]:.6f}] (width {q[1] - q[0]:.6f}); min {v.min():.6f}")
        assert r["start"][0, 0] == 0 and r["lo"][0, 0] == v.min() == mt.result()["min"][c]
        assert r["hi"][0, 0] - r["lo"][0, 0] < q[1] - q[0] and q[0] > r["lo"][0, 0]
        h = mt.hist(20, [c])                           # the marginal falls away from its first class
        assert h["counts"][0, 0] > 2 * h["counts"][0, 10] > 0 and h["below"][0] == 0


@pytest.mark.parametrize("bins", [1, 2, 127, 128])
def test_hist2d(accel_mod, bins):
    w = layout("mid")
    n = 1100
    P = ar1_params(w, n, seed=11)
    mass = (0.68, 0.95)
    with open_acc(accel_mod, w) as acc, filled(accel_mod, acc, P) as mt:
        rows, _ = mt.derive(P)
        nc = rows.shape[1]
        lo1, hi1 = cut_ranges(rows)
        many = np.stack([np.arange(nc), (7 * np.arange(nc) + 3) % nc], axis=1)
        for pairs in ([[5, 6]], [[4, 4], [6, 5], [6, 5]], many):
            pairs = np.asarray(pairs, dtype=np.int32)
            got = mt.hist2d(pairs, bins, mass=mass)
            same(PR.hist2d(rows, pairs, bins, mass=mass), got, (bins, len(pairs)), ("counts", "outside", "level", "status"))
            assert np.all(got["outside"] == 0) and np.all(got["counts"].sum(axis=(1, 2)) == n) and np.all(got["level"][0] >= got["level"][1])
            # row and column sums: the 1-D counts over the same (default) ranges
            h = mt.hist(bins)["counts"]
            assert np.array_equal(got["counts"].sum(axis=2), h[pairs[:, 0]]) and np.array_equal(got["counts"].sum(axis=1), h[pairs[:, 1]])
            lo, hi = np.stack([lo1[pairs[:, 0]], lo1[pairs[:, 1]]], axis=1), np.stack([hi1[pairs[:, 0]], hi1[pairs[:, 1]]], axis=1)
            cut = mt.hist2d(pairs, bins, lo, hi, mass)
            same(PR.hist2d(rows, pairs, bins, lo, hi, mass), cut, (bins, len(pairs), "cut"), ("counts", "outside", "level", "status"))
            assert np.all(cut["counts"].sum(axis=(1, 2)) + cut["outside"] == n) and np.all(cut["level"][0] >= cut["level"][1])
            for p, (a, b) in enumerate(pairs):         # sums against the 1-D classes of the samples inside both ranges
                ca, cb = PR.classes(rows[:, a], lo[p, 0], hi[p, 0], bins), PR.classes(rows[:, b], lo[p, 1], hi[p, 1], bins)
                ins = (ca >= 0) & (cb >= 0)
                assert np.array_equal(cut["counts"][p].sum(axis=1), np.bincount(ca[ins], minlength=bins))
                assert np.array_equal(cut["counts"][p].sum(axis=0), np.bincount(cb[ins], minlength=bins))
            if len(pairs) == 3:
                # a column with itself: the diagonal only, hist of that column at the same range; the repeated pair twice
                d = got["counts"][0]
                assert np.array_equal(d, np.diag(np.diag(d))) and np.array_equal(np.diag(d), h[4])
                dc = cut["counts"][0]
                hc = mt.hist(bins, [4], [lo1[4]], [hi1[4]])
                assert np.array_equal(dc, np.diag(hc["counts"][0])) and cut["outside"][0] == hc["below"][0] + hc["above"][0]
                assert np.array_equal(got["counts"][1], got["counts"][2]) and np.array_equal(cut["counts"][1], cut["counts"][2])
                assert np.array_equal(mt.hist2d([[5, 6]], bins)["counts"][0], got["counts"][1].T)
        assert mt.hist2d([[0, 1]], bins)["level"].shape == (0, 1)


def snapshot(mt, rows):
    nc = rows.shape[1]
    lo, hi = cut_ranges(rows)
    pairs = np.stack([np.arange(nc), (5 * np.arange(nc) + 1) % nc], axis=1)
    out = {}
    for tag, r in (("h", mt.hist(50)), ("hc", mt.hist(64, None, lo, hi)), ("p", mt.hpd([0.5, 0.68, 0.95])), ("j", mt.hist2d(pairs, 32, mass=(0.68, 0.95)))):
        out.update({tag + "_" + k: v for k, v in r.items()})
    return out


def test_independence(accel_mod):
    """One push, pushes of 1 and of 7 rows, two values of max_samples, rejected and skipped rows or none; a selection
    reversed and a subset."""
    w = layout("one")
    n = 300
    P = ar1_params(w, n, seed=21)
    Pin, skip = with_rejects(P)
    with open_acc(accel_mod, w) as acc:
        with accel_mod.ModeTable(acc, n) as clean:
            rows, _ = clean.derive(P)
            clean.push(P)
            base = snapshot(clean, rows)
            lo, hi = cut_ranges(rows)
            sel = np.array([11, 3, 7, 0, 12], dtype=np.int32)
            for name, r, ref, cut in (("hist", clean.hist(64, sel, lo[sel], hi[sel]), "hc", lambda a: a[sel]),
                                      ("hist reversed", clean.hist(50, np.arange(12, -1, -1)), "h", lambda a: a[::-1]),
                                      ("hpd", clean.hpd([0.5, 0.68, 0.95], sel), "p", lambda a: a[:, sel])):
                for k in ("counts", "below", "above", "range", "status") if ref != "p" else ("start", "lo", "hi"):
                    a, b = r[k], cut(base[ref + "_" + k])
                    assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), (name, k)
        for step, ms in ((len(Pin), n), (7, n + 37), (1, n)):
            with accel_mod.ModeTable(acc, ms) as mt:
                for k0 in range(0, len(Pin), step):
                    mt.push(Pin[k0:k0 + step], skip=skip[k0:k0 + step])
                assert mt.result()["n_used"] == n and mt.result()["n_rejected"] == 3
                same(base, snapshot(mt, rows), ("pushes of", step, ms))


@pytest.mark.parametrize("name", ["one", "g3-5"])
def test_nothing_else_moves(accel_mod, name):
    w = layout(name)
    n = 400
    with open_acc(accel_mod, w) as acc:
        if name == "one":
            mt = filled(accel_mod, acc, ar1_params(w, n, seed=31))
            rows, _ = mt.derive(ar1_params(w, n, seed=31))
        else:
            mt, rows = indices_table(accel_mod, acc, w, n, 0)
        with mt:
            def others():
                out = {"q": mt.quantiles([0.16, 0.5, 0.84])["values"]}
                out.update({"res_" + k: np.asarray(v) for k, v in mt.result().items()})
                out.update({"ess_" + k: np.asarray(v) for k, v in mt.ess(0).items()})
                out["acov"] = mt.acov()
                return out
            before = others()
            rank = mt.rank_diag(0)
            racov = [mt.rank_acov(s) for s in range(4)]
            t0 = (mt.kernel_time(), mt.diag_kernel_time(), mt.rank_kernel_time())
            assert mt.pdf_kernel_time() == (0.0, 0)
            pdf = snapshot(mt, rows)
            ms, launches = mt.pdf_kernel_time()
            assert ms > 0.0 and launches == 2 + 2 + 1                        # hist, hist, (sort, hpd), pair
            assert t0 == (mt.kernel_time(), mt.diag_kernel_time(), mt.rank_kernel_time())
            for s in range(4):                                               # not refused, and the same bytes
                assert np.array_equal(bits(mt.rank_acov(s)), bits(racov[s]))
            assert np.array_equal(bits(mt.acov()), bits(before["acov"]))
            after = others()
            for k in before:
                a, b = before[k], after[k]
                assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), k
            rank2 = mt.rank_diag(0)
            for k in rank:
                a, b = np.asarray(rank[k]), np.asarray(rank2[k])
                assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), k
            same(pdf, snapshot(mt, rows), "after the other calls")
            if name != "one":
                assert not np.any(pdf["h_status"]) and pdf["h_counts"].shape[0] == mt.n_cols > len(MR.layout(2, w["plength"]))
                same(PR.hist(rows, 50), {k[2:]: v for k, v in pdf.items() if k.startswith("h_")}, "indices", ("counts", "below", "above", "range", "status"))
                same(PR.hpd(rows, [0.5, 0.68, 0.95]), {k[2:]: v for k, v in pdf.items() if k.startswith("p_")}, "indices", ("k", "start", "lo", "hi"))
            mt.reset()
            assert mt.pdf_kernel_time() == (0.0, 0)


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
            refused(mt.hist, 10); refused(mt.hpd, [0.5]); refused(mt.hist2d, [[0, 1]], 8)
            assert mt.pdf_kernel_time() == (0.0, 0)
        with accel_mod.ModeTable(acc, 12) as mt:
            refused(mt.hist, 10); refused(mt.hist2d, [[0, 1]], 8); refused(mt.hpd, [0.5])        # no row
            mt.push(P[:3])
            mt.hist(10); mt.hist2d([[0, 1]], 8)
            refused(mt.hpd, [0.5])                                                              # n = 3 < 4
            mt.push(P[3:])
            rows, _ = mt.derive(P)
            base = snapshot(mt, rows)
            for bad in (0, 4097, -1):
                refused(mt.hist, bad)
            for bad in (0, 129, -1):
                refused(mt.hist2d, [[0, 1]], bad)
            for bad in ([], [13], [-1], [0, 0], [1, 2, 1], list(range(13)) + [0]):
                refused(mt.hist, 10, bad); refused(mt.hpd, [0.5], bad)
            for bad in ([0.0], [1.0000001], [np.nan], [-0.5], [0.5, 0.0], [], [0.1] * 9):
                refused(mt.hpd, bad)
                if len(bad) and len(bad) < 9:
                    refused(mt.hist2d, [[0, 1]], 8, None, None, bad)
            refused(mt.hist2d, [[0, 1]], 8, None, None, [0.1] * 9)
            refused(mt.hpd, [0.5], None, -1)
            for lo, hi in (([1.0], [0.5]), ([0.0], [np.inf]), ([-np.inf], [0.0]), ([np.nan], [1.0]), ([-1.7e308], [1.7e308])):
                refused(mt.hist, 10, [0], lo, hi)
                refused(mt.hist2d, [[0, 1]], 8, [[0.0, lo[0]]], [[1.0, hi[0]]])
            for bad in ([[0, 13]], [[-1, 0]], np.zeros((0, 2), dtype=np.int32), np.zeros((1025, 2), dtype=np.int32)):
                refused(mt.hist2d, bad, 8)
            lib, one = acc._lib, np.zeros(64)
            assert lib.tamcmc_modepdf_hist(mt._mt, 4, 1, None, one.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None, None, None) == E
            assert lib.tamcmc_modepdf_hist(mt._mt, 4, 1, None, None, None, None, None, None, None, None) == E       # NULL counts
            assert lib.tamcmc_modepdf_hpd(mt._mt, 1, one.ctypes.data_as(C.POINTER(C.c_double)), 1, None, 0, None, None, None, None) == E
            assert lib.tamcmc_modepdf_hist2d(mt._mt, 4, 1, None, None, None, 0, None, None, None, None, None) == E
            # a batch in flight, then a batch armed, on the table's context: every entry point is refused
            T = np.ones(len(P))
            for enter, leave in ((lambda: acc.begin(P, T), acc.end), (lambda: acc.arm(len(P)), acc.disarm)):
                enter()
                refused(mt.hist, 10); refused(mt.hpd, [0.5]); refused(mt.hist2d, [[0, 1]], 8); refused(mt.pdf_kernel_time)
                leave()
            same(base, snapshot(mt, rows), "after the refusals")
