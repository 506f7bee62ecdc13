"""Parameter rows at which a formula of the derivation changes branch or degenerates: zero / negative splittings and
asymmetry, inclination 0 / 45 / 90 / beyond, atan(p4 / p3) with p3 = 0, a vanishing visibility or height, a mode exactly on
a bin, two modes on one frequency, equal / negative / tiny widths, an AppWidth width that overflows, a switched-off Harvey
profile.  Shared by the eval suite (tests/test_special_values_gpu.py) and the mode-table suite
(tests/test_modetable_special_gpu.py).  Importing this module needs no GPU."""
import numpy as np

VARIANTS = (dict(asym=0.0), dict(asym=25.0), dict(asym=0.0, do_amp=True))


def cases(mid, w):
    """[(name, params row, kind)] of workload w of model id mid; kind is None, "inc90" (d/d(inclination) is analytically
    zero) or "overflow" (id 9: the width exponent becomes nu_dip, ~2600, and exp() over- and underflows)."""
    pl = np.asarray(w["plength"])
    off = np.concatenate([[0], np.cumsum(pl)])
    base = np.asarray(w["params_true"], dtype=float)
    out = [("base", base, None)]

    def setp(name, idx, val, kind=None):
        p = base.copy()
        p[idx] = val
        out.append((name, p, kind))
    s6 = off[6]
    atan_pair = mid in (2, 9, 10, 11, 12, 13, 14)          # params[s+3], [s+4] = sqrt(a1) cos i, sqrt(a1) sin i
    for j in range(min(int(pl[6]), 6)):
        setp(f"split[{j}]=0", s6 + j, 0.0, "inc90" if (atan_pair and j == 3) else None)
        setp(f"split[{j}]<0", s6 + j, -abs(base[s6 + j]) - 1e-3)
    if pl[9] >= 1:
        for v in (0.0, 90.0, 45.0, 1e-9, 89.999999, 150.0, -20.0):
            setp(f"inc={v}", off[9], v, "inc90" if abs(v - 90.0) < 1e-4 else None)
    if pl[1] >= 1:
        setp("V1=0", off[1], 0.0)
    if pl[0] >= 1:
        setp("H0=0", off[0], 0.0)
        setp("H0<0", off[0], -base[off[0]])
    if pl[2] >= 2:
        setp("f on a bin", off[2], w["x"][np.searchsorted(w["x"], base[off[2]])])
        setp("f0==f1", off[2] + 1, base[off[2]])
    wd = off[7]
    if pl[7] >= 2:
        setp("W[1]=W[0]", wd + 1, base[wd], "overflow" if mid == 9 else None)      # id 9: exponent := nu_dip (~2600)
        setp("W[0]<0", wd, -base[wd])
        setp("W[0] tiny", wd, 1e-6)
    if pl[8] >= 3:
        setp("Harvey H=0", off[8], 0.0)
        setp("Harvey tau=0", off[8] + 1, 0.0)
    return out
