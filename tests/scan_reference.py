"""An independent numpy reference of the sliding-window predictive scan (tamcmc_summary_scan_*, include/tamcmc_accel.h),
written from the definitions there and run in long double (or, to measure what float64 costs, in float64): per position
j = 0 ... Nx - W the windowed check of the bins [j, j + W).  The tails are predictive_reference.log_gamma_tails at the shape
p W and predictive_reference.log_half_erfc, as in tests/window_reference.py; tests/test_summary_scan_host.py pins this file
to that one at aligned positions.

Sums over the bins of a window and over the samples are taken one term after the other, in ascending order."""
import numpy as np

from predictive_reference import LD, _log_mean_exp, _seq_sum, log_gamma_tails, log_half_erfc


def scan_sums(rows, y, W, like=0, sigma=None, dtype=LD):
    """S[n, Nx - W + 1]: the sum over the bins [j, j + W) of y / M (like 0) or (y - M) / sigma, ascending from bin j."""
    M = np.asarray(rows).astype(dtype)
    yq = np.asarray(y).astype(dtype)
    q = yq / M if like == 0 else (yq - M) / np.asarray(sigma).astype(dtype)
    n_pos = M.shape[1] - W + 1
    assert n_pos >= 1
    S = q[:, :n_pos].copy()
    for i in range(1, W):
        S = S + q[:, i:i + n_pos]
    return S


def scan_reference(rows, y, W, like=0, p=1, sigma=None, dtype=LD, positions=None):
    """rows: (n, Nx) model values of the accepted samples.  Returns dict(log_cdf, log_sf, mean_resid, pit) per position, in
    `dtype`; with `positions` (indices) for those positions alone, which saves the tails of the others."""
    S = scan_sums(rows, y, W, like, sigma, dtype)
    if positions is not None:
        S = S[:, np.asarray(positions, dtype=np.int64)]
    if like == 0:
        logP, logQ = log_gamma_tails(int(p) * int(W), dtype(int(p)) * S, dtype)
    else:
        g = S / np.sqrt(dtype(int(W)))
        logP, logQ = log_half_erfc(-g, dtype), log_half_erfc(g, dtype)
    lc, ls = _log_mean_exp(logP), _log_mean_exp(logQ)
    pit = np.where(lc < ls, np.exp(lc), -np.expm1(ls))
    return dict(log_cdf=lc, log_sf=ls, mean_resid=_seq_sum(S / dtype(int(W))) / dtype(S.shape[0]), pit=pit)


def default_line(W, Nx):
    """The Bonferroni line at 1 % over Nx / W independent windows."""
    return float(np.log(0.01 * float(W) / float(Nx)))


def scan_totals(log_cdf, log_sf):
    """The two minima with their positions: the first position wins a tie, a NaN is skipped, -1 where every value is NaN."""
    out = {}
    for name, v in (("log_sf", log_sf), ("log_cdf", log_cdf)):
        v = np.asarray(v, dtype=np.float64)
        if np.all(np.isnan(v)):
            out["min_" + name], out["pos_min_" + name] = float("nan"), -1
        else:
            out["min_" + name], out["pos_min_" + name] = float(np.nanmin(v)), int(np.nanargmin(v))
    return out


def regions(values, W, Nx, log_below=None, mean_resid=None):
    """The maximal runs of consecutive positions whose value is below the line (a NaN is never below it), in position order:
    a list of dicts pos_first, pos_last, bin_first = pos_first, bin_last = pos_last + W - 1, pos_min (the first position of
    the run's minimum), min_log and, where mean_resid is given, mean_resid_at_min.  log_below None: default_line(W, Nx)."""
    line = default_line(W, Nx) if log_below is None else float(log_below)
    assert line < 0
    v = np.asarray(values, dtype=np.float64)
    below = [bool(x < line) for x in v]
    out, j = [], 0
    while j < len(v):
        if not below[j]:
            j += 1
            continue
        e = j
        while e + 1 < len(v) and below[e + 1]:
            e += 1
        run = v[j:e + 1]
        at = j + int(np.argmin(run))
        r = dict(pos_first=j, pos_last=e, bin_first=j, bin_last=e + W - 1, pos_min=at, min_log=float(v[at]))
        if mean_resid is not None:
            r["mean_resid_at_min"] = float(mean_resid[at])
        out.append(r)
        j = e + 1
    return out
