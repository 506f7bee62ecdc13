"""An independent numpy reference of leave-one-window-out PSIS-LOO and its PIT sub-mode (tamcmc_summary_wloo_*,
include/tamcmc_accel.h), composed from the references the per-bin and the windowed suites already have: the window sums of
x = -l, taken one bin after the other in ascending order (np.cumsum), go through summary_support.psis_reference and
loopit_reference.log_weights with "bin" read as "window"; the predictive tails of a (sample, window) are
window_reference's -- log_gamma_tails at the shape p len, log_half_erfc of R / sqrt(len).  Run in long double, or in float64 to
measure what that format costs."""
import numpy as np

from loopit_reference import _lse, log_weights
from predictive_reference import log_gamma_tails, log_half_erfc
from summary_support import psis_reference, x_of
from window_reference import partition, window_sums

LD = np.longdouble
LOO_KEYS = ("elpd_lwo", "pareto_k", "cutoff")
PIT_KEYS = ("loo_log_cdf", "loo_log_sf", "loo_pit", "is_ess", "log_wsum")


def window_x(xbins, W, first=0):
    """(n, n_windows): x per bin added over each window in ascending bin order, starting from the first term."""
    _, begin, end = partition(xbins.shape[1], W, first)
    return np.stack([np.cumsum(xbins[:, b:e], axis=1)[:, -1] for b, e in zip(begin, end)], axis=1)


def wloo_reference(rows, y, W, first=0, like=0, p=1, sigma=None, dtype=LD, xbins=None, pit=True):
    """rows: (n, Nx) model values of the accepted samples; xbins: -l per bin where the caller perturbs it apart from the
    rows.  Returns elpd_lwo, pareto_k, cutoff, tail_len per window and, with `pit`, the five results of wloo_pit_result plus
    the two reference-side identities of loopit_reference (elpd_from_weights, log_wsum_direct)."""
    if xbins is None:
        xbins = x_of(rows, y, like, p, sigma, dtype)
    xw = window_x(np.asarray(xbins, dtype=dtype), W, first)
    r = psis_reference(xw, dtype)
    out = dict(elpd_lwo=r["elpd_loo"], pareto_k=r["pareto_k"], cutoff=r["cutoff"], tail_len=r["tail_len"])
    if not pit:
        return out
    lw, xmax, direct = log_weights(xw, dtype)
    S, length = window_sums(rows, y, W, first, like, sigma, dtype)
    logP, logQ = np.empty_like(S), np.empty_like(S)
    for ln in np.unique(length):
        sel = length == ln
        if like == 0:
            logP[:, sel], logQ[:, sel] = log_gamma_tails(int(p) * int(ln), dtype(int(p)) * S[:, sel], dtype)
        else:
            g = S[:, sel] / np.sqrt(dtype(int(ln)))
            logP[:, sel], logQ[:, sel] = log_half_erfc(-g, dtype), log_half_erfc(g, dtype)
    lW, lA, lB, lW2 = _lse(lw), _lse(lw + logP), _lse(lw + logQ), _lse(2 * lw)
    lc, ls = lA - lW, lB - lW
    res = dict(loo_log_cdf=lc, loo_log_sf=ls, loo_pit=np.where(lc < ls, np.exp(lc), -np.expm1(ls)), is_ess=np.exp(2 * lW - lW2),
               log_wsum=lW, elpd_from_weights=_lse(lw - xw) - lW, log_wsum_direct=direct)
    bad = ~np.isfinite(xmax)
    for k in res:
        res[k] = np.where(bad, dtype(np.nan), res[k])
    out.update(res)
    return out
