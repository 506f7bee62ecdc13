"""An independent numpy reference of the posterior predictive check (tamcmc_summary_predictive_*, include/tamcmc_accel.h),
written from the definitions there and run in long double (or, to measure what float64 costs, in float64).  Needs neither
scipy nor mpmath: the incomplete gamma functions are log-domain sums, erfc is a series below 1 and a continued fraction
above (tests/test_summary_predictive_host.py pins it against mpmath where that is installed).

Sums over samples are taken one sample after the other (np.cumsum), the order of any streaming sum: the float64 run then
carries the n 2^-52 accumulation error a float64 stream cannot avoid, and its distance from the long-double run is an
honest measure of it."""
import numpy as np

LD = np.longdouble


def _seq_sum(a):
    """Sum over axis 0, one row after the other."""
    return np.cumsum(a, axis=0)[-1]


def log_half_erfc(r, dtype=LD):
    """log(erfc(r) / 2), elementwise, finite for every finite r of moderate size (r^2 must not overflow)."""
    r = np.asarray(r, dtype=dtype)
    x = np.abs(r)
    out = np.empty(r.shape, dtype=dtype)
    sqrt_pi = np.sqrt(dtype(np.pi) if dtype is not LD else LD(4) * np.arctan(LD(1)))
    half = dtype(0.5)
    # x < 1: erf(x) = 2 / sqrt(pi) exp(-x^2) sum_n 2^n x^(2n+1) / (1 3 5 ... (2n+1)), terms of one sign; erfc = 1 - erf >= 0.157
    small = x < 1
    xs = x[small]
    t = xs.copy()
    s = xs.copy()
    for n in range(1, 80):
        t = t * (2 * xs * xs) / dtype(2 * n + 1)
        s = s + t
    erfc_small = 1 - 2 / sqrt_pi * np.exp(-xs * xs) * s
    # x >= 1: erfc(x) = exp(-x^2) / (sqrt(pi) K), K = x + (1/2) / (x + 1 / (x + (3/2) / (x + ...))), evaluated bottom-up at a
    # fixed depth: 400 levels below 3 (the truncation error is about exp(-2 x sqrt(2 N)): 5e-25 at x = 1), 60 above
    big = ~small
    xb = x[big]
    K = xb.copy()
    for depth, sel in ((400, xb < 3), (60, xb >= 3)):
        xx = xb[sel]
        k_ = xx.copy()
        for k in range(depth, 0, -1):
            k_ = xx + (dtype(k) * half) / k_
        K[sel] = k_
    log_erfc_big = -xb * xb - np.log(K * sqrt_pi)
    # r >= 0: log(erfc(x) / 2); r < 0: erfc(r) / 2 = 1 - erfc(x) / 2
    log_half = np.empty(r.shape, dtype=dtype)
    log_half[small] = np.log(erfc_small * half)
    log_half[big] = log_erfc_big - np.log(dtype(2))
    neg = r < 0
    out[~neg] = log_half[~neg]
    out[neg] = np.log1p(-np.exp(log_half[neg]))
    return out


def log_gamma_tails(p, z, dtype=LD, closed_form=True):
    """(log P(p, z), log Q(p, z)) of the regularised incomplete gamma functions for an integer p >= 1, elementwise; z <= 0
    gives (-inf, 0).  p = 1 is the exponential distribution, Q = exp(-z) and P = 1 - exp(-z) = -expm1(-z): written down as
    such unless closed_form is False (the general sums give the same: tests/test_summary_predictive_host.py)."""
    z = np.asarray(z, dtype=dtype)
    pos = z > 0
    zz = z[pos]
    if p == 1 and closed_form:
        logP = np.full(z.shape, -np.inf, dtype=dtype)
        logQ = np.zeros(z.shape, dtype=dtype)
        logP[pos] = np.log(-np.expm1(-zz))
        logQ[pos] = -zz
        return logP, logQ
    lz = np.log(zz)
    lfact = np.concatenate([[dtype(0)], np.cumsum(np.log(np.arange(1, p + 300, dtype=dtype)))])     # log k!
    # Q = exp(-z) sum_{k<p} z^k / k!, as a log-sum-exp with the exact maximum
    terms = [dtype(k) * lz - lfact[k] for k in range(p)]
    m = terms[0]
    for t in terms[1:]:
        m = np.maximum(m, t)
    s = np.zeros_like(zz)
    for t in terms:
        s = s + np.exp(t - m)
    lq = -zz + m + np.log(s)
    # P = 1 - Q where Q < 1/2; elsewhere (z below the median, so z < p + 1) the series exp(-z) z^p / p! sum_j z^j / ((p+1) ... (p+j))
    with np.errstate(divide="ignore", invalid="ignore"):      # (Q = 1 to every digit, or a rounding above, at a small z: the series below takes over there)
        lp = np.log1p(-np.exp(lq))
    low = lq >= np.log(dtype(0.5))
    zl = zz[low]
    t = np.ones_like(zl)
    s = np.ones_like(zl)
    for j in range(1, 260):
        t = t * zl / dtype(p + j)
        s = s + t
    lp[low] = -zl + dtype(p) * lz[low] - lfact[p] + np.log(s)
    logP = np.full(z.shape, -np.inf, dtype=dtype)
    logQ = np.zeros(z.shape, dtype=dtype)
    logP[pos] = lp
    logQ[pos] = lq
    return logP, logQ


def _log_mean_exp(l):
    """log((1/n) sum_s exp l_s) per column, the exact maximum taken out; a column of -inf gives -inf."""
    n = l.shape[0]
    a = l.max(axis=0)
    fin = np.isfinite(a)
    out = np.full(l.shape[1], -np.inf, dtype=l.dtype)
    with np.errstate(invalid="ignore"):
        out[fin] = a[fin] + np.log(_seq_sum(np.exp(l[:, fin] - a[fin])) / l.dtype.type(n))
    return out


def predictive_reference(rows, y, like=0, p=1, sigma=None, dtype=LD):
    """rows: (n, Nx) model values of the accepted samples.  Returns dict(log_cdf, log_sf, mean_resid, pit) in `dtype`."""
    M = np.asarray(rows).astype(dtype)
    yq = np.asarray(y).astype(dtype)
    if like == 0:
        resid = yq / M
        logP, logQ = log_gamma_tails(int(p), dtype(int(p)) * yq / M, dtype)
    else:
        resid = (yq - M) / np.asarray(sigma).astype(dtype)
        logP, logQ = log_half_erfc(-resid, dtype), log_half_erfc(resid, dtype)
    lc, ls = _log_mean_exp(logP), _log_mean_exp(logQ)
    pit = np.where(lc < ls, np.exp(lc), -np.expm1(ls))
    return dict(log_cdf=lc, log_sf=ls, mean_resid=_seq_sum(resid) / dtype(M.shape[0]), pit=pit)


def totals_from_pit(pit):
    """ks_D and pit_hist as the header defines them, from the library's own pit: long double, bin order."""
    u = np.sort(np.asarray(pit, dtype=np.float64)).astype(LD)
    N = LD(u.size)
    k = np.arange(u.size).astype(LD)
    D = max(float(np.max((k + 1) / N - u)), float(np.max(u - k / N)), 0.0)
    cells = np.minimum(19, np.floor(20.0 * np.asarray(pit, dtype=np.float64)).astype(np.int64))
    return D, np.bincount(cells, minlength=20).astype(np.int64)
