"""Independent restatement, in numpy long double, of the comparison of fits (include/tamcmc_accel_compare.h, tamcmc_compare_*):
the variate of (unit, global replicate) from the Philox generator of tests/scan_null_reference.py, the inclusion rule, the pair
totals, the bootstrap's z with its first-order sensitivity, the counting rules, the weights, and the stacking objective with
its gradient, their sensitivity and the K = 2 optimum by bisection.  Nothing here calls the library.

Sensitivities (absolute, first order), the project's standing convention: every input of the float64 evaluation moved by a
relative 2^-50.
  z_k = N' B_k / A, A = sum e_i, B_k = sum e_i D_ki:  e_i dz/de_i = N' e_i (D_ki - B_k / A) / A,  D_ki dz/dD_ki = N' e_i D_ki / A,
      sens(z_k) = 2^-50 (N' / A) sum_i e_i (|D_ki - B_k / A| + |D_ki|).
  g_k = (1 / N') sum_i P_ki / den_i, den_i = sum_j w_j P_ji:  the P_ji of unit i move its term by at most
      (P_ki / den_i) (|1 - w_k P_ki / den_i| + sum_{j != k} w_j P_ji / den_i),
      sens(g_k) = 2^-50 (1 / N') sum_i of that."""
import numpy as np

import scan_null_reference as SN

LD = np.longdouble
EPS = 2.0 ** -52
REL = 2.0 ** -50
K_HIGH = 0.7


def variates(N, seed, g):
    """(e, sens): the N variates of global replicate g in long double, and the sensitivity the scan null's test uses for
    the chi(2,2p) p = 1 variate (one ulp for the logarithm, half an ulp for the division by p = 1)."""
    ue, uo = SN.uniforms(seed, g >> 1, np.arange(N, dtype=np.uint64), 0)
    e = -np.log(uo if g & 1 else ue)
    return e, 1.5 * EPS * e


def included(elpd):
    return np.all(np.isfinite(np.asarray(elpd, dtype=np.float64)), axis=0)


def pair_totals(elpd, khat, a, b):
    elpd = np.asarray(elpd, dtype=np.float64)
    inc = included(elpd)
    n = int(inc.sum())
    with np.errstate(invalid="ignore"):                     # (inf - inf in an excluded unit)
        d = (elpd[a] - elpd[b])[inc]
    out = dict(n_included=n, n_excluded=int(elpd.shape[1] - n), n_better=int((d > 0).sum()), n_worse=int((d < 0).sum()))
    dl = d.astype(LD)
    total = dl.sum() if n else LD("nan")
    out["elpd_diff"] = float(total)
    out["se_diff"] = float(np.sqrt(LD(n) / LD(n - 1) * ((dl - total / LD(n)) ** 2).sum())) if n >= 2 else float("nan")
    if khat is None:
        out["n_k_high"], out["diff_k_high"] = -1, float("nan")
    else:
        khat = np.asarray(khat, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            high = ((khat[a] > K_HIGH) | (khat[b] > K_HIGH))[inc]
        out["n_k_high"] = int(high.sum())
        out["diff_k_high"] = float(dl[high].sum()) if n else float("nan")
    return out


def z_ld(e, elpd):
    """(z, sens), each (K - 1,): the bootstrap's z of one replicate in long double from the variates e (N,), and its
    sensitivity (module docstring)."""
    elpd = np.asarray(elpd, dtype=np.float64)
    inc = included(elpd)
    n = LD(int(inc.sum()))
    e = np.asarray(e, dtype=LD)[inc]
    A = e.sum()
    z, sens = [], []
    for k in range(1, elpd.shape[0]):
        with np.errstate(invalid="ignore"):
            D = (elpd[k] - elpd[0])[inc].astype(LD)      # the float64 subtraction, then exact
        B = (e * D).sum()
        z.append(n * B / A)
        sens.append(REL * (n / A) * (e * (np.abs(D - B / A) + np.abs(D))).sum())
    return np.array(z, dtype=LD), np.array(sens, dtype=LD)


def rank(q, R):
    return min(max(int(np.ceil(q * R)) - 1, 0), R - 1)


def prob(za, zb):
    return int((za > zb).sum()), int((za == zb).sum())


def interval(za, zb, q):
    d = np.sort(np.asarray(za, dtype=np.float64) - np.asarray(zb, dtype=np.float64))
    return float(d[rank(q, d.size)])


def softmax(x):
    x = np.asarray(x, dtype=LD)
    w = np.exp(x - x.max())
    return w / w.sum()


def bma_plus(z, s):
    """z (R, K) with column 0 zero: the mean over r of the softmax of s z_r, in long double."""
    z = np.asarray(z, dtype=LD) * LD(s)
    w = np.exp(z - z.max(axis=1, keepdims=True))
    return (w / w.sum(axis=1, keepdims=True)).mean(axis=0)


def stack_P(elpd, s):
    """P (K, N') in long double over the included units."""
    elpd = np.asarray(elpd, dtype=np.float64)
    v = elpd[:, included(elpd)]
    return np.exp(LD(s) * (v - v.max(axis=0)).astype(LD))


def stack_g(w, P):
    """(g, sens, f): the EM gradient at w in long double, its sensitivity, and the objective."""
    w = np.asarray(w, dtype=LD)
    n = LD(P.shape[1])
    den = (w[:, None] * P).sum(axis=0)
    share = w[:, None] * P / den                         # w_j P_ji / den_i
    g = (P / den).sum(axis=1) / n
    others = share.sum(axis=0)[None, :] - share
    sens = REL * ((P / den) * (np.abs(1 - share) + others)).sum(axis=1) / n
    return g, sens, np.log(den).sum() / n


def stack_optimum_2(P):
    """f* of K = 2 by bisection on f'(w_0) in long double (f is concave in w_0 on [0, 1])."""
    def f(w0):
        return np.log(w0 * P[0] + (1 - w0) * P[1]).sum() / LD(P.shape[1])

    def df(w0):
        return ((P[0] - P[1]) / (w0 * P[0] + (1 - w0) * P[1])).sum()

    lo, hi = LD(0), LD(1)
    if df(lo) <= 0:
        return f(lo)
    if df(hi) >= 0:
        return f(hi)
    for _ in range(200):
        mid = (lo + hi) / 2
        if df(mid) > 0:
            lo = mid
        else:
            hi = mid
    return max(f(lo), f(hi))


def moments_case():
    """The fixed case of the moments check: N = 1000, d = 0.3 standard_t(5) + 0.02 as the first draw of
    numpy.random.default_rng(20261021); fit 0 is zero, fit 1 is d.  R = 4000, seed 12345."""
    d = 0.3 * np.random.default_rng(20261021).standard_t(5, 1000) + 0.02
    return np.stack([np.zeros(1000), d]), 4000, 12345


def moments_check(z, d):
    """z (R,) float64 or long double; d (N',) the included differences.  Under the Bayesian bootstrap E z = sum d and
    Var z = N' S / (N' + 1), S = sum (d - mean d)^2.  Returns the sample mean's and the sample variance's distance from
    these in their own standard errors: sqrt(Var z / R) for the mean, sqrt((m4 - var^2) / R) with the replicates' fourth central
    moment m4 for the variance.  (The long-double restatement of the fixed case sits at -1.25 and -2.36.)"""
    z = np.asarray(z, dtype=LD)
    d = np.asarray(d, dtype=LD)
    n, R = LD(d.size), LD(z.size)
    mean_exact = d.sum()
    var_exact = n * ((d - d.mean()) ** 2).sum() / (n + 1)
    m = z.mean()
    c = z - m
    var = (c ** 2).sum() / (R - 1)
    m4 = (c ** 4).mean()
    se_mean = np.sqrt(var_exact / R)
    se_var = np.sqrt((m4 - var ** 2) / R)
    return float((m - mean_exact) / se_mean), float((var - var_exact) / se_var)
