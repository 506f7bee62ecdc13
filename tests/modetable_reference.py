"""Reference side of the mode-table suites (tamcmc_modetable_*, include/tamcmc_accel.h).  numpy and long double only:
importing this module needs no GPU and no library.

  layout(model_case, plength)   the column layout restated from the id and plength: a structured array with the fields of
                                tamcmc_modetable_col.
  reconstruct(...)              the model row rebuilt from ONE table row plus the noise parameters of the params row, and the
                                first-order sensitivity S of every bin to a relative 2^-50 change of every table entry:

      R_i = noise_i + sum_j [lo_j <= i < hi_j] A_j(x_i) sum_m h_jm / (1 + 4 (x_i - nu_jm)^2 / Gamma_j^2)
      A_j = (1 + a (x_i / f_j - 1))^2 + (0.5 Gamma_j a / f_j)^2   for asymmetry a != 0, else 1
      noise = the Harvey-like sum on |noise params| (oracle/tamcmc_oracle.c:270-288, :488-494)

                                Nothing of the derivation is restated: a table row is a complete description of the
                                sample's mode spectrum, so the oracle's model row checks it.
  bound(M, S)                   RTOL_MODEL * |M_i| + 10 S_i per bin: the project's model bar plus ten times what a 2^-50
                                relative error of every entry could move the bin by (the table is rounded to double, and a
                                component frequency of 3000 widths carries its rounding 3000-fold into a Lorentzian's flank).
"""
import numpy as np

LD = np.longdouble
RTOL_MODEL = 1e-12
REL = LD(2.0) ** -50
KINDS = ("inclination", "eta", "a3", "asymmetry", "freq", "width", "height", "amplitude", "splitting", "window_lo", "window_hi",
         "nu_m", "h_m")
K = {name: k for k, name in enumerate(KINDS)}
COL_DTYPE = np.dtype([("kind", np.int32), ("mult", np.int32), ("order", np.int32), ("l", np.int32), ("m", np.int32),
                      ("param_index", np.int32)])
LOCAL_IDS = (11, 14)


def multiplets(model_case, plength):
    """[(n, l, params index of the frequency)] in the chain's table order: global ids order by order with l = 0 ... lmax
    inside, local ids degree by degree."""
    pl = [int(v) for v in plength]
    Nmax, lmax, Nfl = pl[0], pl[1], pl[2:6]
    off = [Nmax + lmax + sum(Nfl[:l]) for l in range(4)]
    if model_case in LOCAL_IDS:
        return [(n, l, off[l] + n) for l in range(4) for n in range(Nfl[l])]
    return [(n, l, off[l] + n) for n in range(Nmax) for l in range(lmax + 1)]


def layout(model_case, plength):
    rows = [(K[name], -1, -1, -1, 0, -1) for name in KINDS[:4]]
    for j, (n, l, idx) in enumerate(multiplets(model_case, plength)):
        rows += [(K[name], j, n, l, 0, idx if name == "freq" else -1) for name in KINDS[4:11]]
        rows += [(K["nu_m"], j, n, l, m, -1) for m in range(-l, l + 1)]
        rows += [(K["h_m"], j, n, l, m, -1) for m in range(-l, l + 1)]
    return np.array(rows, dtype=COL_DTYPE)


def first_columns(cols):
    """Column of `freq` of every multiplet, in order."""
    return np.flatnonzero(cols["kind"] == K["freq"])


def noise_row(plength, x, params):
    pl = [int(v) for v in plength]
    z, Nnoise = sum(pl[:8]), pl[8]
    npar = np.abs(np.asarray(params, dtype=np.float64)[z:z + Nnoise]).astype(LD)
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    y = np.zeros(xl.size, dtype=LD)
    for k in range((Nnoise - 1) // 3):
        H, tau, p = npar[3 * k:3 * k + 3]
        if tau != 0:
            y = y + H / ((LD(1e-3) * tau * xl) ** p + 1)
    return y + npar[Nnoise - 1]


def reconstruct(model_case, plength, x, params, row, cols=None):
    """(R, S): the rebuilt model row and the sensitivity of every bin, long double."""
    cols = layout(model_case, plength) if cols is None else cols
    row = np.asarray(row, dtype=np.float64)
    assert row.shape == (len(cols),)
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    R = noise_row(plength, x, params)
    S = np.zeros(xl.size, dtype=LD)
    a = LD(row[K["asymmetry"]])
    for c0 in first_columns(cols):
        l = int(cols["l"][c0])
        nc = 2 * l + 1
        f, G = LD(row[c0]), LD(row[c0 + 1])
        lo, hi = int(row[c0 + 5]), int(row[c0 + 6])
        assert row[c0 + 5] == lo and row[c0 + 6] == hi and 0 <= lo < hi <= xl.size
        xs = xl[lo:hi]
        nu = row[c0 + 7:c0 + 7 + nc].astype(LD)
        h = row[c0 + 7 + nc:c0 + 7 + 2 * nc].astype(LD)
        d = xs[None, :] - nu[:, None]
        if G == 0:
            # a width of exactly 0: the limit the oracle's quotient takes, h / (1 + inf) = 0 in every bin off the component
            # and h / (1 + 0 / 0) = NaN in a bin exactly on it; nothing for the sensitivity to weigh
            R[lo:hi] += np.where((d == 0).any(axis=0), LD(np.nan), LD(0))
            continue
        Lz = 1 / (1 + 4 * d * d / (G * G))
        hL = h[:, None] * Lz
        core = hL.sum(axis=0)
        if a != 0:
            b, c2 = 1 + a * (xs / f - 1), (LD(0.5) * G * a / f) ** 2
            A = b * b + c2
            dA_f = np.abs(2 * b * (-a * xs / f) - 2 * c2)                 # f dA/df
            dA_a = np.abs(2 * b * a * (xs / f - 1) + 2 * c2)              # a dA/da
            dA_G = 2 * c2                                                 # Gamma dA/dGamma
        else:
            A, dA_f, dA_a, dA_G = LD(1), LD(0), LD(0), LD(0)
        R[lo:hi] += A * core
        s = np.abs(A * hL).sum(axis=0)                                               # h dR/dh
        s = s + np.abs(A * hL * Lz * 8 * d * nu[:, None] / (G * G)).sum(axis=0)      # nu dR/dnu
        s = s + np.abs(A * (hL * Lz * 8 * d * d / (G * G)).sum(axis=0) + dA_G * core)  # Gamma dR/dGamma
        s = s + (dA_f + dA_a) * np.abs(core)
        S[lo:hi] += REL * s
    return R, S


def bound(M, S):
    return LD(RTOL_MODEL) * np.abs(np.asarray(M).astype(LD)) + 10 * S


def worst_ratio(R, S, M):
    """max_i |R_i - M_i| / bound_i."""
    return float(np.max(np.abs(R - np.asarray(M).astype(LD)) / bound(M, S)))


def c_lm(l, m, variant):
    """oracle/tamcmc_oracle.c:155-168"""
    if l == 1:
        return 0.0 if variant == 1 else float(m)
    if l == 2:
        return (5.0 * m ** 3 - 17.0 * m) / 3.0
    return 0.0


def q_lm(l, m):
    return (l * (l + 1) - 3.0 * m * m) / ((2 * l - 1) * (2 * l + 3))


def variant_of(model_case):
    return 1 if model_case in (6, 7, 8) else 2 if model_case in (13, 14) else 0


def fold(rows):
    """float64 restatement of the table's fold (tm_mt_fold_one, serial per column in push order, never contracted) and of
    the host's finish: dict of mean, sd, min, max of the columns of rows (n, n_cols).
      d = v - mean; mean += d / n; M2 += d * (v - mean); min / max keep the earlier of two equal values (so the zero that came
      first, with its sign); sd = sqrt(M2 / (n - 1)), NaN for n < 2."""
    rows = np.asarray(rows, dtype=np.float64)
    n, nc = rows.shape
    mean, M2 = np.zeros(nc), np.zeros(nc)
    mn, mx = rows[0].copy(), rows[0].copy()
    with np.errstate(all="ignore"):
        for t in range(n):
            v = rows[t]
            d = v - mean
            mean = mean + d / np.float64(t + 1)
            M2 = M2 + d * (v - mean)
            if t > 0:
                mn = np.where(v < mn, v, mn)
                mx = np.where(v > mx, v, mx)
        sd = np.sqrt(M2 / np.float64(n - 1)) if n >= 2 else np.full(nc, np.nan)
    return dict(mean=mean, sd=sd, min=mn, max=mx)
