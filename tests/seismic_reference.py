"""numpy restatement of the mode table's seismic indices (include/tamcmc_accel_seismic.h; csrc/tamcmc_seismic.h): the plan
from a reference row of base columns by the header's stated rules, and the evaluator -- Python-level ordered loops over a
column's terms, vectorised over samples -- in float64 (the same + - * / as the device: equal bits) and in np.longdouble (the
yardstick of the error bound).  Nothing here is derived from the library's output."""
import math

import numpy as np

import modetable_reference as MR

KINDS = ("dnu_fit", "epsilon", "numax", "dnu_nl", "d2nu", "d02", "d13", "d01", "d10", "r02", "r01", "r13", "r10")
K = {k: len(MR.KINDS) + i for i, k in enumerate(KINDS)}
ALL_KINDS = tuple(MR.KINDS) + KINDS
ONE = -1                    # src of a term that reads the constant 1.0
MARGIN, GAP = 0.35, 0.25
RATIOS = ("r02", "r01", "r13", "r10")


class Refused(Exception):
    pass


def ls_coefficients(ks):
    """Slope and intercept coefficients of the orders ks (ascending), every sum in that order in float64."""
    T = len(ks)
    sk = 0.0
    for k in ks:
        sk = sk + float(k)
    kbar = sk / float(T)
    S = 0.0
    for k in ks:
        d = float(k) - kbar
        S = S + d * d
    c = [(float(k) - kbar) / S for k in ks]
    a = [1.0 / float(T) - kbar * ci for ci in c]
    return c, a


def assign(cols, ref):
    """(modes, info): modes[l] = [(k, freq column, amplitude column)] in ascending k of the assigned modes of degree l."""
    ref = np.asarray(ref, dtype=np.float64)
    fc = {l: [int(c) for c in np.flatnonzero((cols["kind"] == MR.K["freq"]) & (cols["l"] == l))] for l in range(4)}
    r = sorted(fc[0], key=lambda c: ref[c])                 # (stable: ties in column order)
    T = len(r)
    if T < 3 or not np.all(np.isfinite(ref[r])):
        raise Refused("fewer than 3 radial modes")
    c, a = ls_coefficients(list(range(T)))
    b_ref = 0.0
    for ci, col in zip(c, r):
        b_ref = b_ref + ci * float(ref[col])
    a_ref = 0.0
    for ai, col in zip(a, r):
        a_ref = a_ref + ai * float(ref[col])
    if not (b_ref > 0.0 and math.isfinite(b_ref) and math.isfinite(a_ref)):
        raise Refused("slope")
    for i, col in enumerate(r):
        if not abs(float(ref[col]) - (a_ref + b_ref * float(i))) <= GAP * b_ref:
            raise Refused("radial gap")
    nb = math.floor(a_ref / b_ref - 0.5)
    if not abs(nb) < 1e9:
        raise Refused("orders are 32-bit")
    off = MR.K["amplitude"] - MR.K["freq"]
    modes = {0: [(i, col, col + off) for i, col in enumerate(r)]}
    n_un = 0
    for l in (1, 2, 3):
        u = [(float(ref[col]) - a_ref) / b_ref - float(l) / 2.0 for col in fc[l]]
        kk = [float(np.rint(v)) for v in u]
        out = []
        for i, col in enumerate(fc[l]):
            ok = abs(u[i] - kk[i]) <= MARGIN and all(j == i or kk[j] != kk[i] for j in range(len(kk)))
            if ok:
                out.append((int(kk[i]), col, col + off))
            else:
                n_un += 1
        modes[l] = sorted(out)
    info = dict(n_base_cols=len(cols), n_radial=T, n_unassigned=n_un, n_base=int(nb), dnu_ref=b_ref, eps_ref=a_ref / b_ref - float(nb),
                a_ref=a_ref)
    return modes, info


def plan(cols, ref):
    """The plan: dict of cols (MR.COL_DTYPE, the index columns), terms (per column: (n_num, src, wsrc, coef, offset)) and the
    info numbers.  Raises Refused."""
    modes, info = assign(cols, ref)
    nbase = info["n_base"]
    where = {l: {k: fcol for (k, fcol, _) in modes[l]} for l in range(4)}
    out_cols, terms = [], []

    def nu(l, k, coef):
        return (where[l].get(k), -1, coef)

    def add(kind, k, l, num, den=(), offset=0.0):
        if any(t[0] is None for t in list(num) + list(den)):
            return
        ordered = kind not in ("dnu_fit", "epsilon", "numax")
        out_cols.append((K[kind], -1, nbase + k if ordered else -1, l, 0, -1))
        tt = list(num) + list(den)
        terms.append(dict(n_num=len(num), n_den=len(den), src=np.array([t[0] for t in tt], dtype=np.int32),
                          wsrc=np.array([t[1] for t in tt], dtype=np.int32), coef=np.array([t[2] for t in tt], dtype=np.float64),
                          offset=float(offset)))

    c0 = a0 = None
    for l in range(4):
        if len(modes[l]) < 2:
            continue
        c, a = ls_coefficients([m[0] for m in modes[l]])
        add("dnu_fit", 0, l, [(m[1], -1, ci) for m, ci in zip(modes[l], c)])
        if l == 0:
            c0, a0 = c, a
    add("epsilon", 0, -1, [(m[1], -1, ai) for m, ai in zip(modes[0], a0)], [(m[1], -1, ci) for m, ci in zip(modes[0], c0)], float(nbase))
    add("numax", 0, -1, [(m[1], m[2], 1.0) for m in modes[0]], [(ONE, m[2], 1.0) for m in modes[0]])
    ks = [m[0] for l in range(4) for m in modes[l]]
    orders = range(min(ks) - 1, max(ks) + 2)
    n02 = lambda k: [nu(0, k, 1.0), nu(2, k - 1, -1.0)]
    n13 = lambda k: [nu(1, k, 1.0), nu(3, k - 1, -1.0)]
    n01 = lambda k: [nu(0, k - 1, 0.125), nu(1, k - 1, -0.5), nu(0, k, 0.75), nu(1, k, -0.5), nu(0, k + 1, 0.125)]
    n10 = lambda k: [nu(1, k - 1, -0.125), nu(0, k, 0.5), nu(1, k, -0.75), nu(0, k + 1, 0.5), nu(1, k + 1, -0.125)]
    dl1 = lambda k: [nu(1, k, 1.0), nu(1, k - 1, -1.0)]
    dl0 = lambda k: [nu(0, k + 1, 1.0), nu(0, k, -1.0)]
    for l in range(4):
        for k in orders:
            add("dnu_nl", k, l, [nu(l, k, 1.0), nu(l, k - 1, -1.0)])
    for l in range(4):
        for k in orders:
            add("d2nu", k, l, [nu(l, k + 1, 1.0), nu(l, k, -2.0), nu(l, k - 1, 1.0)])
    for kind, l, num, den in (("d02", 0, n02, None), ("d13", 1, n13, None), ("d01", 0, n01, None), ("d10", 1, n10, None),
                              ("r02", 0, n02, dl1), ("r01", 0, n01, dl1), ("r13", 1, n13, dl0), ("r10", 1, n10, dl0)):
        for k in orders:
            add(kind, k, l, num(k), den(k) if den else ())
    info = dict(info, n_index_cols=len(out_cols))
    return dict(cols=np.array(out_cols, dtype=MR.COL_DTYPE), terms=terms, info=info)


def _sum(x, t, lo, hi, dtype):
    acc = np.zeros(x.shape[0], dtype=dtype)
    for i in range(lo, hi):
        s, ws = int(t["src"][i]), int(t["wsrc"][i])
        v = dtype(t["coef"][i]) * (x[:, s] if s >= 0 else np.ones(x.shape[0], dtype=dtype))
        if ws >= 0:
            w = x[:, ws]
            v = v * (w * w)
        acc = acc + v
    return acc


def evaluate(terms, base_rows, dtype=np.float64):
    """(n, n_index) index columns of the base rows (n, n_base_cols): the stated arithmetic in `dtype`."""
    x = np.asarray(base_rows, dtype=np.float64).astype(dtype)
    out = np.empty((x.shape[0], len(terms)), dtype=dtype)
    with np.errstate(all="ignore"):
        for j, t in enumerate(terms):
            n1, n2 = t["n_num"], t["n_num"] + t["n_den"]
            v = _sum(x, t, 0, n1, dtype)
            if n2 > n1:
                v = v / _sum(x, t, n1, n2, dtype)
            if t["offset"] != 0.0:
                v = v - dtype(t["offset"])
            out[:, j] = v
    return out


def sensitivity(terms, base_rows):
    """(n, n_index): the first-order change of every index column under a relative change of 1 in each of its sources, summed
    in absolute value (long double): |d value / d x_s| |x_s| over the sources s, products of weights included."""
    x = np.asarray(base_rows, dtype=np.float64).astype(np.longdouble)
    out = np.zeros((x.shape[0], len(terms)), dtype=np.longdouble)
    with np.errstate(all="ignore"):
        for j, t in enumerate(terms):
            n1, n2 = t["n_num"], t["n_num"] + t["n_den"]

            def mag(lo, hi):
                acc = np.zeros(x.shape[0], dtype=np.longdouble)
                for i in range(lo, hi):
                    s, ws = int(t["src"][i]), int(t["wsrc"][i])
                    v = np.abs(np.longdouble(t["coef"][i]) * (x[:, s] if s >= 0 else 1.0))
                    if ws >= 0:
                        v = v * (x[:, ws] * x[:, ws]) * (3.0 if s >= 0 else 2.0)     # x_s once, the weight twice
                    acc = acc + v
                return acc
            num = _sum(x, t, 0, n1, np.longdouble)
            if n2 > n1:
                den = _sum(x, t, n1, n2, np.longdouble)
                out[:, j] = mag(0, n1) / np.abs(den) + np.abs(num) * mag(n1, n2) / (den * den)
            else:
                out[:, j] = mag(0, n1)
    return out
