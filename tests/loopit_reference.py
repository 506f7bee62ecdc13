"""An independent numpy reference of LOO-PIT (tamcmc_summary_loo_pit_*, include/tamcmc_accel.h), written from the
definition there and run in long double (or, to measure what float64 costs, in float64): per bin the PSIS weights of every
sample -- with the tie-mean rule for samples whose x are equal -- the predictive tails of predictive_reference.py, and the
four sums, each with its exact maximum taken out."""
import math

import numpy as np

from predictive_reference import log_gamma_tails, log_half_erfc
from summary_support import tail_M, x_of

LD = np.longdouble
KEYS = ("loo_log_cdf", "loo_log_sf", "loo_pit", "is_ess", "log_wsum")


def _smoothed(tail, c, dtype):
    """zt of an ascending tail z (step 3 of the PSIS-LOO definition); zt = z where there is no usable fit."""
    L = tail.size
    if L < 5:
        return tail.copy()
    eps10 = dtype(10.0 * 2.0 ** -52)
    ec = np.exp(c)
    t = np.exp(tail) - ec
    m = 30 + int(math.floor(math.sqrt(L)))
    q = int(math.floor(L / 4.0 + 0.5))
    j = np.arange(1, m + 1).astype(dtype)
    theta = (1 - np.sqrt(dtype(m) / (j - dtype(0.5)))) / (3 * t[q - 1]) + 1 / t[L - 1]
    k = np.mean(np.log1p(-theta[:, None] * t[None, :]), axis=1)
    ell = L * (np.log(-theta / k) - k - 1)
    w = 1 / np.sum(np.exp(ell[None, :] - ell[:, None]), axis=1)
    w = np.where(w < eps10, dtype(0), w)
    w = w / np.sum(w)
    that = np.sum(w * theta)
    kk = np.mean(np.log1p(-that * t))
    sigma = -kk / that
    kh = (L * kk + 5) / (L + 10)
    if not np.isfinite(kh):
        return tail.copy()
    lp = np.log1p(-(np.arange(1, L + 1).astype(dtype) - dtype(0.5)) / L)
    inner = -sigma * lp if kh == 0 else sigma / kh * np.expm1(-kh * lp)
    return np.minimum(np.log(inner + ec), dtype(0))


def log_weights(x, dtype=LD):
    """x: (n, Nx) values of -l.  Returns (lw (n, Nx), xmax (Nx), log_wsum_direct (Nx)): the log weight of every sample by
    steps 1-2 of the definition, and log(sum_body exp z + sum_T exp zt) formed without the per-sample detour."""
    x = np.asarray(x, dtype=dtype)
    n, nx = x.shape
    M = tail_M(n)
    log_min = np.log(dtype(np.finfo(np.float64).tiny))
    lw = np.empty_like(x)
    xmax = x.max(axis=0)
    direct = np.empty(nx, dtype=dtype)
    for i in range(nx):
        order = np.argsort(x[:, i], kind="stable")
        xs = x[order, i]
        z = xs - xmax[i]
        if n > M:
            c = max(z[n - M - 1], log_min)
            in_tail = z > c
        else:
            c = dtype(np.inf)
            in_tail = np.zeros(n, dtype=bool)
        w = z.copy()
        tail = z[in_tail]
        zt = _smoothed(tail, c, dtype)
        direct[i] = np.log(np.sum(np.exp(z[~in_tail])) + np.sum(np.exp(zt)))
        if tail.size:
            # the tie-mean rule: equal x share the mean weight of the ranks they occupy, summed in ascending rank
            xt = xs[in_tail]
            start = np.flatnonzero(np.concatenate([[True], xt[1:] != xt[:-1]]))
            end = np.concatenate([start[1:], [xt.size]])
            for a, b in zip(start, end):
                if b - a > 1:
                    zt[a:b] = np.log(np.cumsum(np.exp(zt[a:b]))[-1] / dtype(b - a))
            w[in_tail] = zt
        lw[order, i] = w
    return lw, xmax, direct


def _lse(l):
    """log sum_s exp l_s per column, the exact maximum taken out, one sample after the other; all -inf gives -inf."""
    a = l.max(axis=0)
    fin = np.isfinite(a)
    out = np.full(l.shape[1], -np.inf, dtype=l.dtype)
    with np.errstate(invalid="ignore"):
        out[fin] = a[fin] + np.log(np.cumsum(np.exp(l[:, fin] - a[fin]), axis=0)[-1])
    return out


def loopit_reference(rows, y, like=0, p=1, sigma=None, dtype=LD, x=None):
    """rows: (n, Nx) model values of the accepted samples; x: -l of them where the caller perturbs it apart from the rows.
    Returns the five results of loo_pit_result in `dtype`, and two reference-side identities: elpd_from_weights =
    lse(lw - x) - lW (which is elpd_loo) and log_wsum_direct."""
    M = np.asarray(rows).astype(dtype)
    yq = np.asarray(y).astype(dtype)
    if x is None:
        x = x_of(rows, y, like, p, sigma, dtype)
    x = np.asarray(x, dtype=dtype)
    lw, xmax, direct = log_weights(x, dtype)
    if like == 0:
        logP, logQ = log_gamma_tails(int(p), dtype(int(p)) * yq / M, dtype)
    else:
        r = (yq - M) / np.asarray(sigma).astype(dtype)
        logP, logQ = log_half_erfc(-r, dtype), log_half_erfc(r, dtype)
    lW, lA, lB, lW2 = _lse(lw), _lse(lw + logP), _lse(lw + logQ), _lse(2 * lw)
    lc, ls = lA - lW, lB - lW
    out = dict(loo_log_cdf=lc, loo_log_sf=ls, loo_pit=np.where(lc < ls, np.exp(lc), -np.expm1(ls)), is_ess=np.exp(2 * lW - lW2),
               log_wsum=lW, elpd_from_weights=_lse(lw - x) - lW, log_wsum_direct=direct)
    bad = ~np.isfinite(xmax)
    for k in out:
        out[k] = np.where(bad, dtype(np.nan), out[k])
    return out
