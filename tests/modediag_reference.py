"""An independent numpy statement of the mode table's diagnostics (include/tamcmc_accel.h, "Mode table diagnostics"), for
tests/test_modediag_gpu.py and tests/test_cli_modediag_gpu.py.  Nothing here is shared with the library; the lag products'
long-double values, their sensitivity bound and the finish are those of tests/ess_reference.py.

centred()    d = rows - mean in long double with the mean taken as given, and the one-ulp-per-value error e = 2^-52 |d|.
lag()        ess_reference.lag_products on it: A (L + 1, n_cols) in long double and the bound of every entry.
cov_sums()   S_ij = sum_t d_i d_j in long double and the bound, the same expression with two columns:
               n 2^-53 sum_t |d_i d_j|  +  sum_t (e_i |d_j| + |d_i| e_j).
corr()       r_ij = S_ij / sqrt(S_ii S_jj) in long double and what the bounds of the three sums move it by, to first order,
               b_ij / sqrt(S_ii S_jj) + |r_ij| (b_ii / S_ii + b_jj / S_jj) / 2,
             plus 8 ulp of max(|r|, 1) for the host's two square roots, product and two divisions (cov = S / (n - 1) twice over).
totals()     the totals from the arrays, in column order: the first column wins a tie, a NaN is skipped.
headline()   the columns chainsummary_hip --modes-corr takes: the chain-level ones and freq ... splitting of every multiplet.
"""
import numpy as np

import ess_reference as ER

LD = np.longdouble
U = 2.0 ** -52


def centred(rows, mean):
    d = np.asarray(rows).astype(LD) - np.asarray(mean).astype(LD)
    return d, U * np.abs(d).astype(np.float64)


def lag(d, e, L):
    return ER.lag_products(d, e, L)


def cov_sums(d, e):
    d = np.asarray(d, dtype=LD)
    n = d.shape[0]
    ad, e = np.abs(d).astype(np.float64), np.asarray(e, dtype=np.float64)
    S = d.T @ d
    cross = e.T @ ad
    bound = n * 0.5 * U * (ad.T @ ad) + cross + cross.T
    return S, bound


def corr(S, bound):
    var = np.diag(S).astype(LD)
    with np.errstate(all="ignore"):
        den = np.sqrt(var[:, None] * var[None, :])
        r = S / den
        rel = (np.diag(bound) / var.astype(np.float64))
        b = (bound / den).astype(np.float64) + np.abs(r).astype(np.float64) * 0.5 * (rel[:, None] + rel[None, :])
    bad = ~((var > 0) & np.isfinite(var))
    r[bad, :] = np.nan
    r[:, bad] = np.nan
    return r, b


def totals(ess, rhat, cut, A0, L, n):
    def extreme(v, better):
        best, at = np.nan, -1
        for c, x in enumerate(v):
            if not np.isnan(x) and (at < 0 or better(x, best)):
                best, at = x, c
        return best, at
    min_ess, col_min = extreme(ess, lambda a, b: a < b)
    max_rhat, col_max = extreme(rhat, lambda a, b: a > b)
    with np.errstate(invalid="ignore"):
        return dict(n_used=int(n), lag=int(L), min_ess=min_ess, col_min_ess=col_min, max_rhat=max_rhat, col_max_rhat=col_max,
                    n_truncated=int(np.sum(np.asarray(cut) == L + 1)), n_constant=int(np.sum(np.asarray(A0) == 0.0)),
                    n_rhat_high=int(np.sum(np.asarray(rhat) > 1.01)))


def headline(cols):
    """Indices of the columns whose kind is inclination ... splitting (codes 0 ... 8), in table order."""
    return np.flatnonzero(np.asarray(cols["kind"]) <= 8).astype(np.int32)
