"""An independent numpy statement of the mode table's rank-normalised diagnostics (include/tamcmc_accel.h, "Mode table
diagnostics on ranks", steps 1-7), for tests/test_moderank_gpu.py and tests/test_cli_moderank_gpu.py.  Nothing here is shared
with the library: ranks come from np.sort and np.searchsorted on the key order, Phi^-1 from mpmath at 40 digits, the finish is
ess_reference.finish and the lag products' long-double values and bound are modediag_reference.lag.

key()        the order: v + 0.0 (so that -0 and +0 are one value) as a monotone uint64.
rank2()      #{s < v_t} + #{s <= v_t} + 1, an int64 per sample.
z_exact()    a = 4 rank2 - 3, D = 8 n + 2, the smaller tail inverted at 40 digits: (z as float64, the bound
             10 2^-50 q / phi(z) + 4 2^-52 |z|), per distinct rank2; cached per (min(a, D - a), D).
median(), quantile()   0.5 s[(n-1)/2] + 0.5 s[n/2] of the sorted column; the order statistic of rank ceil(q n) - 1.
welford_mean()         the float64 recurrence mean += (v - mean) / count, in t order, for every column of an (n, m) array at once.
pick(), totals()       step 6's NaN-skipping minimum / maximum of two arrays; step 7 from the arrays.
"""
import functools
import math

import mpmath
import numpy as np

LD = np.longdouble
U = 2.0 ** -52
OUT = ("ess_bulk", "ess_tail", "rhat", "tau_bulk", "rhat_bulk", "rhat_fold", "ess_q05", "ess_q95")
SERIES = ("z", "zfold", "i05", "i95")
TOTALS = ("n_used", "lag", "min_ess_bulk", "col_min_ess_bulk", "min_ess_tail", "col_min_ess_tail", "max_rhat", "col_max_rhat",
          "n_truncated", "n_constant", "n_rhat_high")


def key(v):
    u = (np.asarray(v, dtype=np.float64) + 0.0).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def rank2(v):
    k = key(v)
    s = np.sort(k)
    return (np.searchsorted(s, k, side="left") + np.searchsorted(s, k, side="right") + 1).astype(np.int64)


def sorted_values(v):
    v = np.asarray(v, dtype=np.float64) + 0.0
    return v[np.argsort(key(v), kind="stable")]


def median(v):
    s = sorted_values(v)
    n = s.size
    return np.float64(0.5) * s[(n - 1) // 2] + np.float64(0.5) * s[n // 2]


def quantile(v, q):
    s = sorted_values(v)
    n = s.size
    return s[min(max(int(math.ceil(np.float64(q) * np.float64(n))) - 1, 0), n - 1)]


@functools.lru_cache(maxsize=None)
def _g_exact(m, D):
    """g(m / D) = -Phi^-1(m / D) at 40 digits, 0 < m / D < 1/2: (float64 value, q / phi(g) as float64)"""
    with mpmath.workdps(40):
        q = mpmath.mpf(m) / mpmath.mpf(D)
        g = mpmath.sqrt(2) * mpmath.erfinv(1 - 2 * q)
        phi = mpmath.exp(-g * g / 2) / mpmath.sqrt(2 * mpmath.pi)
        return float(g), float(q / phi), g


def z_exact(r2, n):
    """For an array of rank2 values: (z float64 nearest the exact value, bound, error function) -- error(z_lib) evaluates
    |z_lib - z_exact| with the 40-digit value, so that the comparison itself adds nothing."""
    r2 = np.asarray(r2, dtype=np.int64)
    D = 8 * n + 2
    z, bound, exact = np.empty(r2.size), np.empty(r2.size), []
    for i, r in enumerate(r2):
        a = 4 * int(r) - 3
        b = D - a
        if a == b:
            z[i], bound[i] = 0.0, 0.0
            exact.append(mpmath.mpf(0))
            continue
        g, sens, gm = _g_exact(min(a, b), D)
        z[i] = -g if a < b else g
        bound[i] = 10 * 2.0 ** -50 * sens + 4 * U * abs(g)
        exact.append(-gm if a < b else gm)
    return z, bound, exact


def z_error(z_lib, exact):
    with mpmath.workdps(40):
        return np.array([float(abs(mpmath.mpf(float(x)) - e)) for x, e in zip(z_lib, exact)])


def welford_mean(S):
    S = np.asarray(S, dtype=np.float64)
    m = np.zeros(S.shape[1])
    for t in range(S.shape[0]):
        m = m + (S[t] - m) / np.float64(t + 1)
    return m


def pick(a, b, smaller):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        both = np.where(b < a, b, a) if smaller else np.where(b > a, b, a)
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, both))


def totals(cols, ess_bulk, ess_tail, rhat, cut_bulk, A0_bulk, L, n):
    def extreme(v, better):
        best, at = np.nan, -1
        for c, x in zip(cols, v):
            if not np.isnan(x) and (at < 0 or better(x, best)):
                best, at = float(x), int(c)
        return best, at
    mb, cb = extreme(ess_bulk, lambda a, b: a < b)
    mt, ct = extreme(ess_tail, lambda a, b: a < b)
    mr, cr = extreme(rhat, lambda a, b: a > b)
    with np.errstate(invalid="ignore"):
        return dict(n_used=int(n), lag=int(L), min_ess_bulk=mb, col_min_ess_bulk=cb, min_ess_tail=mt, col_min_ess_tail=ct, max_rhat=mr,
                    col_max_rhat=cr, n_truncated=int(np.sum(np.asarray(cut_bulk) == L + 1)), n_constant=int(np.sum(np.asarray(A0_bulk) == 0.0)),
                    n_rhat_high=int(np.sum(np.asarray(rhat) > 1.01)))

