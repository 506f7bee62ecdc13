"""An independent numpy statement of the ESS mode's definition (include/tamcmc_accel.h, "EFFECTIVE SAMPLE SIZE"), for
tests/test_summary_ess_gpu.py and tests/test_summary_ess_host.py.  Nothing here is shared with the library.

series()       both centred series from model rows, in long double (or any dtype), with the frozen mean_M / lppd given.
lag_products() A_k = sum_t d_t d_{t-k} in long double, and the bound on what a float64 accumulation of the same terms may
               differ by -- the SENSITIVITY, derived here:
                 * accumulation: n - k fused multiply-adds, each rounding a partial sum no larger than S_k = sum_t |d_t d_{t-k}|
                   to half an ulp: at most (n - k) 2^-53 S_k, stated as in the definition;
                 * one ulp in each centred value: d_t -> d_t + e_t moves A_k by at most sum_t (e_t |d_{t-k}| + |d_t| e_{t-k}),
                   e_t = 2^-52 |d_t| (the subtraction that forms d_t is exact up to its own rounding);
                 * likelihood series only, u = exp(l - lppd) - 1: one ulp in l (2^-52 |l|) and the rounding of l - lppd
                   (2^-53 |l - lppd|) pass through exp with the factor exp(l - lppd) = u + 1, and exp itself is within one ulp
                   (2^-52 (u + 1)): e_t gains (u_t + 1) (2^-52 |l_t| + 2^-53 |l_t - lppd| + 2^-52).
               The tests allow 10 x this: the terms are bounds on single effects, and the device's l differs from the long
               double l by the roundings of y / M, log M and their sum, which one ulp of l does not cover where they cancel.
finish()       Geyer's initial monotone sequence in plain float64, one bin at a time, operation by operation as the header
               states it.
rhat()         the split R-hat formula on rows, in long double.
"""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -52


def lag_limit(max_lag, n):
    m = min((max_lag or 255) | 1, n - 1)
    return m if m % 2 == 1 else m - 1


def like(rows, y, like_case=0, p=1.0, sigma=None, dtype=LD):
    Mq, yq = np.asarray(rows).astype(dtype), np.asarray(y).astype(dtype)
    if like_case == 0:
        return -dtype(float(int(p))) * (yq / Mq + np.log(Mq))                # `long p`, likelihoods.cpp:17
    return -((yq - Mq) ** 2) / np.asarray(sigma).astype(dtype) ** 2         # the reference's convention: no factor 1/2


def series(rows, y, mean_M, lppd, like_case=0, p=1.0, sigma=None, dtype=LD):
    """(a, u, e_a, e_u): the two centred series (n, Nx) and the one-ulp-per-value error of each, as derived above."""
    Mq = np.asarray(rows).astype(dtype)
    a = Mq - np.asarray(mean_M).astype(dtype)
    l = like(rows, y, like_case, p, sigma, dtype)
    z = l - np.asarray(lppd).astype(dtype)
    u = np.exp(z) - dtype(1)
    e_a = U * np.abs(a)
    e_u = U * np.abs(u) + (u + 1) * (U * np.abs(l) + 0.5 * U * np.abs(z) + U)
    return a, u, e_a, e_u


def lag_products(d, e, L):
    """A (L + 1, Nx) in long double and the sensitivity bound (float64) of every entry."""
    d = np.asarray(d, dtype=LD)
    n, nx = d.shape
    ad, e = np.abs(d).astype(np.float64), np.asarray(e, dtype=np.float64)
    A, bound = np.zeros((L + 1, nx), dtype=LD), np.zeros((L + 1, nx))
    for k in range(L + 1):
        A[k] = (d[k:] * d[:n - k]).sum(axis=0)
        S = (ad[k:] * ad[:n - k]).sum(axis=0)
        bound[k] = (n - k) * 0.5 * U * S + (e[k:] * ad[:n - k]).sum(axis=0) + (ad[k:] * e[:n - k]).sum(axis=0)
    return A, bound


def finish(A, n):
    """tau, ess (float64) and cut (int32) per bin from A (L + 1, Nx) float64."""
    A = np.asarray(A, dtype=np.float64)
    L, nx = A.shape[0] - 1, A.shape[1]
    floor = 1.0 / math.log10(float(n))
    tau, ess, cut = np.empty(nx), np.empty(nx), np.zeros(nx, dtype=np.int32)
    with np.errstate(all="ignore"):
        for i in range(nx):
            A0 = A[0, i]
            if A0 == 0.0 or not np.isfinite(A0):
                tau[i] = ess[i] = np.nan
                continue
            rho = A[:, i] / A0
            P = rho[0::2] + rho[1::2]
            K = len(P)
            for m in range(len(P)):
                if not P[m] >= 0.0:
                    K = m
                    break
            s, prev = np.float64(0.0), None
            for m in range(K):
                v = P[m] if prev is None or not prev < P[m] else prev
                s = s + v
                prev = v
            t = np.float64(-1.0) + np.float64(2.0) * s
            t = np.float64(floor) if t < floor else t
            tau[i], ess[i], cut[i] = t, np.float64(n) / t, 2 * K
    return tau, ess, cut


def rhat(rows):
    """Split R-hat per bin of rows (n, Nx), in long double."""
    x = np.asarray(rows).astype(LD)
    n = x.shape[0]
    h = n // 2
    a, b = x[:h], x[n - h:]
    m1, m2 = a.mean(axis=0), b.mean(axis=0)
    W = (((a - m1) ** 2).sum(axis=0) / (h - 1) + ((b - m2) ** 2).sum(axis=0) / (h - 1)) / 2
    mb = (m1 + m2) / 2
    Bn = (m1 - mb) ** 2 + (m2 - mb) ** 2
    with np.errstate(all="ignore"):
        return np.where(W == 0, LD(np.nan), np.sqrt((LD(h - 1) / LD(h) * W + Bn) / W))


def ar1(phi, n, sigma, seed):
    """A stationary AR(1) sequence of marginal standard deviation sigma."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n)
    z = np.empty(n)
    z[0] = e[0]
    c = math.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        z[t] = phi * z[t - 1] + c * e[t]
    return sigma * z


def ess_of_sequence(x, max_lag):
    """The rule applied to one sequence in float64 (centred with its own mean): tau, ess, cut and the P_m it summed."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    L = lag_limit(max_lag, n)
    d = x - x.mean()
    A = np.array([np.dot(d[k:], d[:n - k]) for k in range(L + 1)])
    tau, ess, cut = finish(A[:, None], n)
    rho = A / A[0]
    P = rho[0::2] + rho[1::2]
    return float(tau[0]), float(ess[0]), int(cut[0]), P
