"""An independent numpy reference of the windowed predictive check (tamcmc_summary_window_*, include/tamcmc_accel.h),
written from the definitions there and run in long double (or, to measure what float64 costs, in float64).  Needs neither
scipy nor mpmath: the tails of a window sum are predictive_reference.log_gamma_tails at the shape p len and
predictive_reference.log_half_erfc, which tests/test_summary_window_host.py pins against mpmath at shapes up to 512 where
that is installed (the series of log_gamma_tails runs 260 terms: at shape 512 its first neglected term at z = a, the
largest z it is used for to within the distance from the mean to the median, is 5e-27 of the sum -- the same test checks that).

Sums over the bins of a window and over the samples are taken one after the other (np.cumsum)."""
import numpy as np

from predictive_reference import LD, _log_mean_exp, _seq_sum, log_gamma_tails, log_half_erfc, totals_from_pit


def partition(Nx, W, first=0):
    """(first as resolved, first_bin[n_windows], end_bin[n_windows]): window 0 is [0, min(first, Nx)), window w >= 1 is
    [first + (w - 1) W, min(first + w W, Nx)); n_windows = 1 + ceil(max(Nx - first, 0) / W)."""
    first = W if first == 0 else first
    assert 1 <= first <= W
    nw = 1 + -(-max(Nx - first, 0) // W)
    w = np.arange(nw, dtype=np.int64)
    begin = np.where(w == 0, 0, first + (w - 1) * W)
    end = np.minimum(first + w * W, Nx)
    return first, begin, end


def gathered(windows, Nx, W, first=0):
    """(the windows `windows` with window 0 and the last one, ascending and each once; the bins of those windows in order; first
    as resolved).  Window 0 comes first and only the last window can be short, so the gathered bins are a grid whose partition
    (W, first) has exactly these windows: a reference given that grid evaluates the chosen windows alone."""
    f, begin, end = partition(Nx, W, first)
    sel = np.unique(np.concatenate([np.asarray(windows, dtype=np.int64).reshape(-1), [0, len(begin) - 1]]))
    assert sel[0] == 0 and sel[-1] == len(begin) - 1
    cols = np.concatenate([np.arange(begin[i], end[i]) for i in sel])
    assert np.all((end - begin)[sel[1:-1]] == W) and (len(sel) == 1 or end[0] == f)
    return sel, cols, f


def windows_holding(bins, Nx, W, first=0):
    """gathered() of the windows that hold the bins `bins`."""
    f = W if first == 0 else first
    bins = np.asarray(bins, dtype=np.int64)
    return gathered(np.where(bins < f, 0, 1 + (bins - f) // W), Nx, W, first)


def window_sums(rows, y, W, first=0, like=0, sigma=None, dtype=LD):
    """(S[n, n_windows], len[n_windows]): the sum over each window of y / M (like 0) or (y - M) / sigma, ascending."""
    M = np.asarray(rows).astype(dtype)
    yq = np.asarray(y).astype(dtype)
    q = yq / M if like == 0 else (yq - M) / np.asarray(sigma).astype(dtype)
    _, begin, end = partition(M.shape[1], W, first)
    S = np.stack([np.cumsum(q[:, b:e], axis=1)[:, -1] for b, e in zip(begin, end)], axis=1)
    return S, end - begin


def window_reference(rows, y, W, first=0, like=0, p=1, sigma=None, dtype=LD):
    """rows: (n, Nx) model values of the accepted samples.  Returns dict(log_cdf, log_sf, mean_resid, pit) per window, in
    `dtype`."""
    S, length = window_sums(rows, y, W, first, like, sigma, dtype)
    logP, logQ = np.empty_like(S), np.empty_like(S)
    for ln in np.unique(length):
        sel = length == ln
        if like == 0:
            logP[:, sel], logQ[:, sel] = log_gamma_tails(int(p) * int(ln), dtype(int(p)) * S[:, sel], dtype)
        else:
            g = S[:, sel] / np.sqrt(dtype(int(ln)))
            logP[:, sel], logQ[:, sel] = log_half_erfc(-g, dtype), log_half_erfc(g, dtype)
    lc, ls = _log_mean_exp(logP), _log_mean_exp(logQ)
    pit = np.where(lc < ls, np.exp(lc), -np.expm1(ls))
    return dict(log_cdf=lc, log_sf=ls, mean_resid=_seq_sum(S / length.astype(dtype)) / dtype(S.shape[0]), pit=pit)


def window_totals(pit, log_cdf, log_sf):
    """The totals the header defines, from the library's own arrays: ks_D and pit_hist over the window PITs, the two minima
    with their windows (the first window wins a tie)."""
    D, hist = totals_from_pit(pit)
    ls, lc = np.asarray(log_sf, dtype=np.float64), np.asarray(log_cdf, dtype=np.float64)
    return dict(ks_D=D, pit_hist=hist, min_log_sf=float(ls.min()), win_min_log_sf=int(np.argmin(ls)),
                min_log_cdf=float(lc.min()), win_min_log_cdf=int(np.argmin(lc)))
