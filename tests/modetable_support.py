"""What the mode-table suites on the GPU share (tests/test_modetable_gpu.py, tests/test_modetable_special_gpu.py): opening a
context, the identities the columns of a table row obey among themselves, the reconstruction check against the oracle, the
statistics and quantile checks, and the bit-for-bit comparison of two results.  Importing this module needs no GPU."""
import numpy as np

import modetable_reference as MR
from support import LD, bits, pyorc

ULP = 2.0 ** -52
QS = np.array([0.0, 1e-9, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0])
K = MR.K


def open_acc(accel_mod, w, y=None):
    return accel_mod.Accel(w["model_case"], w["plength"], w["x"], np.ones(w["x"].size) if y is None else y)


def ranks_of(q, n):
    """tmq_rank of tamcmc_quantile.h: numpy's inverted_cdf"""
    return np.clip(np.ceil(np.asarray(q) * float(n)) - 1, 0, n - 1).astype(np.int64)


def ulps(a, b):
    ka, kb = (np.where(v < 0, -(v & 0x7FFFFFFFFFFFFFFF), v) for v in (np.asarray(a, dtype=np.float64).view(np.int64),
                                                                      np.asarray(b, dtype=np.float64).view(np.int64)))
    return np.abs(ka - kb)


def check_identities(w, cols, P, rows):
    """Item 2 of the suite, on every row.  Returns the largest distance of `amplitude` from numpy's value, in ulps."""
    mid, pl, x = w["model_case"], [int(v) for v in w["plength"]], w["x"]
    variant = MR.variant_of(mid)
    cfg = sum(pl[:10])
    first = MR.first_columns(cols)
    worst_amp = 0
    for p, r in zip(P, rows):
        has = cols["param_index"] >= 0
        assert np.array_equal(bits(r[has]), bits(p[cols["param_index"][has]])), "freq is not the params entry"
        trunc_c, do_amp = p[cfg], p[cfg + 1] != 0.0
        eta, a3 = LD(r[K["eta"]]), LD(r[K["a3"]])
        a1 = [r[c0 + 4] for c0 in first if cols["l"][c0] >= 1][:1]
        for c0 in first:
            l, n = int(cols["l"][c0]), int(cols["order"][c0])
            nc = 2 * l + 1
            f, G, height, amp, fs, lo, hi = r[c0:c0 + 7]
            nu, h = r[c0 + 7:c0 + 7 + nc], r[c0 + 7 + nc:c0 + 7 + 2 * nc]
            assert list(cols["kind"][c0 + 7:c0 + 7 + 2 * nc]) == [K["nu_m"]] * nc + [K["h_m"]] * nc
            s = 0.0
            for v in h:
                s = s + v
            assert bits(s) == bits(height), "height is not the in-order sum of h_m"
            worst_amp = max(worst_amp, int(ulps(amp, np.sqrt((np.pi * height) * G))))
            if l == 0:
                assert bits(nu[0]) == bits(f) and bits(fs) == bits(0.0)
                if do_amp:
                    assert abs(LD(np.pi) * LD(height) * LD(G) - LD(abs(p[n]))) <= 4 * ULP * abs(p[n]), "l = 0 amplitude form"
            else:
                for k in range(nc):
                    m = k - l
                    t = [LD(f), LD(f) * eta * LD(MR.q_lm(l, m)), m * LD(fs), LD(MR.c_lm(l, m, variant)) * a3]
                    assert abs(LD(nu[k]) - sum(t)) <= 4 * ULP * sum(abs(v) for v in t), (l, m)
            if variant != 1:
                # the window splitting is the chain's a1: the splitting column of any l >= 1 multiplet.  A layout without
                # one (lmax = 0) is checked against both sides of the window's a1 = 1 branch.
                cand = a1 if a1 else [0.5, 2.0]
                wins = [pyorc().truncation_window(x, f, s_win, G, l, trunc_c) for s_win in cand]
                assert (0, int(lo), int(hi)) in wins, (l, n, lo, hi, wins)
    return worst_amp


def check_case(accel_mod, w, P, oracle_rows=True):
    """Reconstruction (item 1) and identities (item 2) of the rows P of workload w.  Returns (worst ratio, amplitude ulps)."""
    mid, pl, x = w["model_case"], w["plength"], w["x"]
    cols = MR.layout(mid, pl)
    with open_acc(accel_mod, w) as acc:
        with accel_mod.ModeTable(acc) as mt:
            got = mt.columns()
            assert got.dtype == cols.dtype and np.array_equal(got, cols), "the layout is not the restatement's"
            rows, st = mt.derive(P)
        own = [acc.model_explicit(p) for p in P]
    assert np.all(st == 0) and rows.shape == (len(P), len(cols))
    worst = 0.0
    for p, r, (m_own, st_own) in zip(P, rows, own):
        R, S = MR.reconstruct(mid, pl, x, p, r, cols)
        assert st_own == 0
        refs = [m_own]
        if oracle_rows:
            m_orc, st_orc = pyorc().model(mid, p, pl, x)
            assert st_orc == 0
            refs.append(m_orc)
        for M in refs:
            ratio = MR.worst_ratio(R, S, M)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (mid, ratio)
    return worst, check_identities(w, cols, P, rows)


def same_results(a, b):
    for k in a:
        if isinstance(a[k], np.ndarray) and a[k].dtype == np.float64:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        else:
            assert np.array_equal(a[k], b[k]), k


def collect(mt, with_quantiles=True):
    out = mt.result()
    if with_quantiles and out["n_used"] > 0:
        q = mt.quantiles(QS)
        out.update(q_ranks=q["ranks"], q_values=q["values"])
    return out


def check_statistics(tag, res, rows):
    """Item 5 against the accepted derived rows: count, min, max exact; mean within n 2^-52 mean|c|; the variance within
    4 n 2^-52 mean(c^2) of the long-double values."""
    n = len(rows)
    c = rows.astype(LD)
    assert res["n_used"] == n and res["n_cols"] == rows.shape[1], tag
    assert np.array_equal(bits(res["min"]), bits(rows.min(axis=0))) and np.array_equal(bits(res["max"]), bits(rows.max(axis=0))), tag
    mean = c.mean(axis=0)
    assert np.all(np.abs(res["mean"].astype(LD) - mean) <= n * ULP * np.abs(c).mean(axis=0)), tag
    if n < 2:
        assert np.all(np.isnan(res["sd"])), tag
    else:
        var = ((c - mean) ** 2).sum(axis=0) / (n - 1)
        assert np.all(np.abs(res["sd"].astype(LD) ** 2 - var) <= 4 * n * ULP * (c * c).mean(axis=0)), tag


def check_quantiles(tag, res, rows):
    """Item 6: the ranks of tmq_rank, and the order statistic itself, bit for bit."""
    n = len(rows)
    assert np.array_equal(res["q_ranks"], ranks_of(QS, n)), tag
    want = np.sort(rows, axis=0)[res["q_ranks"]]
    assert np.array_equal(bits(res["q_values"]), bits(want)), tag
