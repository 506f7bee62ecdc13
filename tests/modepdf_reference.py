"""numpy float64 restatement of the four rules of tamcmc_accel_pdf.h (tamcmc_modepdf_*): the class rule, the sorted column,
the shortest window and the contour levels.  Everything is an integer count or an order statistic, so the library must
return these numbers bit for bit."""
import math

import numpy as np

MAX_BINS, MAX_BINS2D, RANGE = 4096, 128, 1


def range_ok(lo, hi):
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(np.isfinite(lo) and np.isfinite(hi) and hi >= lo and np.isfinite(np.float64(hi) - np.float64(lo)))


def classes(v, lo, hi, bins):
    """int64 class of every value: -1 below, -2 above, else min(floor((v - lo) * s), bins - 1) with s = bins / (hi - lo);
    class 0 throughout when not hi > lo."""
    v, lo, hi = np.asarray(v, dtype=np.float64), np.float64(lo), np.float64(hi)
    out = np.zeros(v.shape, dtype=np.int64)
    if hi > lo:
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            s = np.float64(bins) / (hi - lo)
            u = (v - lo) * s
        inside = (v >= lo) & (v <= hi)
        f = np.where(np.isnan(u) | ~inside, 0.0, np.minimum(np.floor(np.where(inside, u, 0.0)), np.float64(bins - 1)))
        out = f.astype(np.int64)
    out[v < lo] = -1
    out[v > hi] = -2
    return out


def hist(V, bins, lo=None, hi=None):
    """V (n, n_sel): dict of counts (n_sel, bins), below, above, range (n_sel, 2), status as ModeTable.hist returns them."""
    V = np.asarray(V, dtype=np.float64)
    n, ns = V.shape
    counts = np.zeros((ns, bins), dtype=np.int64)
    below, above = np.zeros(ns, dtype=np.int64), np.zeros(ns, dtype=np.int64)
    rng, status = np.zeros((ns, 2)), np.zeros(ns, dtype=np.int32)
    for j in range(ns):
        l, h = (V[:, j].min(), V[:, j].max()) if lo is None else (np.float64(lo[j]), np.float64(hi[j]))
        rng[j] = l, h
        if not range_ok(l, h):
            assert lo is None, "an explicit range is refused, not flagged"
            status[j] = RANGE
            continue
        c = classes(V[:, j], l, h, bins)
        counts[j] = np.bincount(c[c >= 0], minlength=bins)
        below[j], above[j] = np.sum(c == -1), np.sum(c == -2)
    return dict(counts=counts, below=below, above=above, range=rng, status=status)


def edges(lo, hi, bins):
    e = np.float64(lo) + (np.float64(hi) - np.float64(lo)) * (np.arange(bins + 1, dtype=np.float64) / np.float64(bins))
    e[bins] = hi
    return e


def window(mass, n):
    return max(1, min(n, int(math.ceil(np.float64(mass) * np.float64(n)))))


def sorted_column(v):
    """ascending in the order of the quantiles' keys: -0 and +0 one value, returned as +0"""
    return np.sort(np.asarray(v, dtype=np.float64) + 0.0)


def hpd(V, mass):
    """V (n, n_sel): dict of k (n_mass), start, lo, hi (n_mass, n_sel): the first shortest window, a NaN width last."""
    V = np.asarray(V, dtype=np.float64)
    n, ns = V.shape
    mass = np.atleast_1d(np.asarray(mass, dtype=np.float64))
    k = np.array([window(m, n) for m in mass], dtype=np.int64)
    start = np.zeros((mass.size, ns), dtype=np.int64)
    lo, hi = np.zeros((mass.size, ns)), np.zeros((mass.size, ns))
    for j in range(ns):
        s = sorted_column(V[:, j])
        for m, km in enumerate(k):
            with np.errstate(invalid="ignore", over="ignore"):
                w = s[km - 1:] - s[:n - km + 1]
            i = 0 if np.all(np.isnan(w)) else int(np.nanargmin(w))     # (argmin returns the first index of the minimum)
            start[m, j], lo[m, j], hi[m, j] = i, s[i], s[i + km - 1]
    return dict(k=k, start=start, lo=lo, hi=hi)


def level(counts, mass):
    """the largest t such that the cells with count >= t hold at least ceil(mass * n_in) samples; 0 where n_in = 0"""
    c = np.sort(np.asarray(counts, dtype=np.int64).ravel())[::-1]
    n_in = int(c.sum())
    if n_in == 0:
        return 0
    need = window(mass, n_in)
    return int(c[np.searchsorted(np.cumsum(c), need)])


def hist2d(V, pairs, bins, lo=None, hi=None, mass=()):
    """V (n, n_cols): dict of counts (n_pairs, bins, bins), outside, level (n_mass, n_pairs), status as ModeTable.hist2d."""
    V = np.asarray(V, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    npair = len(pairs)
    counts = np.zeros((npair, bins, bins), dtype=np.int64)
    outside, status = np.zeros(npair, dtype=np.int64), np.zeros(npair, dtype=np.int32)
    lev = np.zeros((len(mass), npair), dtype=np.int64)
    lo = None if lo is None else np.asarray(lo, dtype=np.float64).reshape(-1, 2)
    hi = None if hi is None else np.asarray(hi, dtype=np.float64).reshape(-1, 2)
    for p, (a, b) in enumerate(pairs):
        cls = []
        for ax, col in enumerate((a, b)):
            l, h = (V[:, col].min(), V[:, col].max()) if lo is None else (lo[p, ax], hi[p, ax])
            if not range_ok(l, h):
                status[p] = RANGE
                break
            cls.append(classes(V[:, col], l, h, bins))
        if status[p]:
            continue
        ins = (cls[0] >= 0) & (cls[1] >= 0)
        outside[p] = np.sum(~ins)
        counts[p] = np.bincount(cls[0][ins] * bins + cls[1][ins], minlength=bins * bins).reshape(bins, bins)
        for m, ms in enumerate(mass):
            lev[m, p] = level(counts[p], ms)
    return dict(counts=counts, outside=outside, level=lev, status=status)
