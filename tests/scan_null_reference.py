"""Independent restatement, in numpy, of the Monte-Carlo null of the scan (include/tamcmc_accel.h, tamcmc_scan_null_*): the
Philox4x32-10 generator with the header's counter and key, the two uniforms of a call, the variates in long double with the
sensitivity of the float64 evaluation, the sliding sums in float64 in the scan's order with the first position of each
extreme, and the counting rules of the calibration by brute force.  Nothing here calls the library.

Sensitivity of a variate (absolute, first order; u is exact): one ulp (2^-52 relative) for each log, sqrt and cospi, half an
ulp (2^-53 relative) for each addition, division and product.
  chi(2,2p)   q = (e_0 + ... + e_{p-1}) / p, every term positive: 2^-52 sum_k e_k (the logs) + 2^-53 sum_{i >= 1} s_i (the
              additions, s_i the partial sum after adding e_i), both over p, + 2^-53 q (the division).
  chi_square  q = sqrt(L) c, L = -log(u_even), c = cospi(2 u_odd): L's ulp is halved by the square root (2^-53), the square
              root's own ulp (2^-52), the cosine's (2^-52), the product's half (2^-53): 3 x 2^-52 |q|.  The reference forms
              cos(pi x) about the nearest multiple of 1/2 of x = 2 u_odd, which is exact in long double, so that it keeps its
              relative accuracy where the cosine passes through zero.
The long-double reference itself is good to about 2^-63 relative per operation, 2000 times finer."""
import numpy as np

LD = np.longdouble
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
EPS = 2.0 ** -52
PI = LD("3.14159265358979323846264338327950288")


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of counter words; returns the four output words as uint64 arrays below 2^32."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in (c0, c1, c2, c3)])
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        a = np.uint64(M0) * c0                               # below 2^64: no wrap
        b = np.uint64(M1) * c2
        n0 = (b >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (a >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c1, c3, c0, c2 = b & np.uint64(MASK), a & np.uint64(MASK), n0, n2
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(wa, wb):
    """(float64, long double): 52 bits of two words plus a half, times 2^-52: the same number in both."""
    n = (np.asarray(wa, dtype=np.uint64) << np.uint64(20)) | (np.asarray(wb, dtype=np.uint64) >> np.uint64(12))
    return (n.astype(np.float64) + 0.5) * 2.0 ** -52, (n.astype(LD) + LD(0.5)) * LD(2.0) ** -52


def uniforms(seed, rep, bins, t):
    """u_even, u_odd (long double) of call t for the bins, global replicate rep."""
    w = philox(bins, t, rep & MASK, (rep >> 32) & MASK, seed & MASK, (seed >> 32) & MASK)
    (e64, e), (o64, o) = uniform(w[0], w[1]), uniform(w[2], w[3])
    assert np.array_equal(e64.astype(LD), e) and np.array_equal(o64.astype(LD), o)        # exact in float64
    return e, o


def cospi_ld(x):
    """cos(pi x) for x in (0, 2), about the nearest multiple of 1/2 (x - h / 2 is exact)."""
    x = np.asarray(x, dtype=LD)
    h = np.rint(2 * x)
    d = (x - h / 2) * PI
    out = np.empty_like(x)
    for hv, f in ((0, np.cos), (1, lambda v: -np.sin(v)), (2, lambda v: -np.cos(v)), (3, np.sin), (4, np.cos)):
        m = h == hv
        out[m] = f(d[m])
    return out


def variates(like, p, Nx, seed, rep):
    """(q, sens): the Nx variates of global replicate rep in long double and their sensitivity (module docstring)."""
    bins = np.arange(Nx, dtype=np.uint64)
    if like != 0:
        ue, uo = uniforms(seed, rep, bins, 0)
        q = np.sqrt(-np.log(ue)) * cospi_ld(2 * uo)
        return q, 3.0 * EPS * np.abs(q)
    z = np.zeros(Nx, dtype=LD)
    logs = np.zeros(Nx, dtype=LD)
    adds = np.zeros(Nx, dtype=LD)
    for k in range(p):
        if k % 2 == 0:
            ue, uo = uniforms(seed, rep, bins, k // 2)
        e = -np.log(ue if k % 2 == 0 else uo)
        z = z + e
        logs += e
        if k >= 1:
            adds += z
    q = z / LD(p)
    return q, (EPS * logs + 0.5 * EPS * adds) / LD(p) + 0.5 * EPS * q


def sliding(q, W):
    """float64 sums of q[j : j + W] in ascending order from the first term, every position."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    n = q.size - W + 1
    s = q[:n].copy()
    for i in range(1, W):
        s = s + q[i:i + n]
    return s


def extremes(q, W):
    """(S_max, its first position, S_min, its first position)"""
    s = sliding(q, W)
    a, b = int(np.argmax(s)), int(np.argmin(s))
    return s[a], a, s[b], b


def calibration(m):
    """m: (R, K) min_log of one side.  Returns cnt (R, K) and vmin (R) by brute force."""
    m = np.asarray(m)
    cnt = np.stack([(m[None, :, k] <= m[:, None, k]).sum(axis=1) for k in range(m.shape[1])], axis=1)
    return cnt, cnt.min(axis=1)


def pvalue(m, k, v):
    R = m.shape[0]
    _, vmin = calibration(m)
    n = int((m[:, k] <= v).sum())
    return (1 + n) / (R + 1), (1 + int((vmin <= n).sum())) / (R + 1)


def line(m, k, alpha, joint):
    """The line, or None where j = floor(alpha (R + 1)) is no rank 1 ... R."""
    R = m.shape[0]
    j = int(np.floor(alpha * (R + 1)))
    if j < 1 or j > R:
        return None
    _, vmin = calibration(m)
    c = int(np.sort(vmin)[j - 1]) if joint else j
    return float(np.sort(m[:, k])[c - 1])


def ks_distance(x, cdf):
    """Kolmogorov distance of the sample x from the law with the given CDF."""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.size
    F = cdf(x)
    return float(max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(n) / n)))
