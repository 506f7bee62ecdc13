"""Builders of the directed edge suite (tests/test_edges_host.py, tests/test_edges_gpu.py).  Test helper only; no GPU.

The hot path cuts a spectrum into units of 512 bins, cells of 8 units and tiles of 1-16 units, and every multiplet has a
truncation window [imin, imax).  The suite does not ask the library where its tiles are: it runs every unit count
through the thresholds of the tile rules (part A), puts a window edge on, before and behind EVERY unit boundary
(part B) and walks the multiplet count over the lane-group switches up to the documented limit (part C).  The judge is
always the oracle (oracle/pyoracle.py); everything here is derived from it and from the inputs alone."""
import math

import numpy as np

import longgrids
import workloads as W
from tamcmc_amd import synth

UNIT = 512

# ---------------------------------------------------------------------------------------------------------------------
# A. grid lengths

SWEEP_UNITS = list(range(1, 81)) + [95, 96, 97, 128, 195, 196, 197]
SHORT_UNITS = [1, 4, 5, 9, 10, 69, 70, 71, 72, 73, 196]
SWEEP_KINDS = ("main", "asym-chi2", "local")


def lengths(units):
    """512u - 1, 512u, 512u + 1 of every unit count u (512u + 1 has u + 1 units; duplicates dropped, Nx >= 2)."""
    out = set()
    for u in units:
        out.update(Nx for Nx in (UNIT * u - 1, UNIT * u, UNIT * u + 1) if Nx >= 2)
    return sorted(out)


def sweep_list():
    """(kind, Nx) of part A: the main sweep, then the asymmetric chi_square case and local id 11 at the shorter list."""
    out = [("main", Nx) for Nx in lengths(SWEEP_UNITS)]
    for kind in ("asym-chi2", "local"):
        out += [(kind, Nx) for Nx in lengths(SHORT_UNITS)]
    return out


_NOISE = None


def _noise(n):
    """-ln u of synth.make_spectrum's default stream: make_spectrum(m) == m * _noise(m.size) (one draw for all grids;
    tests/test_edges_host.py asserts the identity)."""
    global _NOISE
    if _NOISE is None or _NOISE.size < n:
        _NOISE = synth.make_spectrum(np.ones(max(n, 100353)))
    return _NOISE[:n]


def sweep_case(orc, kind, Nx, nchains=4):
    if kind == "main":
        w, like = W.layout(2, 2, Nmax=3, Nx=Nx), 0        # nine multiplets, trunc_c = 20: windows narrower than the grid from ~2000 bins on
    elif kind == "asym-chi2":
        w, like = W.any_model(2, Nx=Nx, asym=25.0), 1
    elif kind == "local":
        w, like = W.any_model(11, Nx=Nx), 0
    else:
        raise ValueError(kind)
    mid = int(w["model_case"])
    m, st = orc.model(mid, w["params_true"], w["plength"], w["x"])
    assert st == 0 and np.all(np.isfinite(m)) and np.all(m > 0), (kind, Nx, st)
    y = m * _noise(Nx)
    sig = 0.05 + 0.2 * np.abs(np.sin(np.arange(Nx))) if like == 1 else None
    return dict(tag=f"A {kind} Nx={Nx} ({(Nx + UNIT - 1) // UNIT} units)", mid=mid, w=w, y=y, sigma=sig, like=like,
                P=W.perturbed(w, nchains, scale=0.003), T=synth.temperatures(nchains), row=Nx % nchains)


_ORACLE = {}


def oracle_answers(orc, key, case, rows=None):
    """logL, status, model rows `rows` (default: the case's one row) and the analytic gradient of a case; computed once
    per key and shared by whoever asks again (the two tile modes of the GPU tests)."""
    if key in _ORACLE:
        return _ORACLE[key]
    w = case["w"]
    rows = [case["row"]] if rows is None else rows
    rL, rst, rm = orc.generate_batch(case["mid"], w["plength"], w["x"], case["y"], case["P"], case["T"], sigma_y=case["sigma"],
                                     likelihood_case=case["like"], want_models=True)
    g, gabs, gL, gst = orc.grad_analytic(case["mid"], w["plength"], w["x"], case["y"], case["P"], case["T"], w["index_to_relax"],
                                         sigma_y=case["sigma"], likelihood_case=case["like"])
    ans = dict(L=rL, st=rst, rows=list(rows), models=rm[rows].copy(), g=g, gabs=gabs, gst=gst)
    _ORACLE[key] = ans
    return ans


# ---------------------------------------------------------------------------------------------------------------------
# B. a window edge on every unit boundary

EDGE_GRIDS = (100000, 30000)          # 196 units (tail-shaped gradient tiles) and 59 units (short-grid rule): every boundary
CLAMP_GRIDS = (10240, 10241)          # imax == Nx with Nx a multiple of 512 and with Nx = 512 k + 1: the last boundaries only
PROBE = 3                             # the k = 3 mode of the l = 0 layout: Gamma = 2.5, so its window is fc -/+ 2.2 c Gamma
PROBE_H = 40.0                        # h_e / M_e = 2.3e-2 at the window edge (see the teeth condition)
Y_OVER_M = 3.0                        # datum at every targeted edge bin, as a multiple of the chain's model there
KINDS = ("imin==b", "imin==b-1", "imin==b+1", "imax==b", "imax==b-1", "imax==b+1")
ONE_BIN = "one-bin"


def edge_base(Nx):
    """l = 0 layout of four modes on a grid whose step (840 / Nx) is not a power of two; the probe raised to PROBE_H."""
    w = W.layout(2, 0, Nmax=4, Nx=Nx, grid=(2300.0, 840.0 / Nx))
    p = w["params_true"].copy()
    p[PROBE] = PROBE_H
    w["params_true"] = p
    b = W.split(w)
    ix = dict(H=PROBE, fc=b["Nmax"] + b["lmax"] + PROBE, G=b["w"] + PROBE, c=b["cfg"], a1=b["s"], N0=b["z"] + 9)
    assert p[ix["G"]] == 2.5 and p[ix["c"]] == 20.0 and p[ix["a1"]] >= 1.0
    return w, ix


def boundaries(Nx, full=True):
    """Every unit boundary 512 k <= Nx, Nx itself, and the row boundaries 512 k + 256 of ten units spread over the grid."""
    units = (Nx + UNIT - 1) // UNIT
    if not full:
        return sorted({UNIT * ((Nx - 1) // UNIT), Nx})
    bs = {UNIT * k for k in range(units + 1) if UNIT * k <= Nx} | {Nx}
    bs |= {UNIT * int(k) + 256 for k in np.linspace(0, (Nx - 257) // UNIT, 10).astype(int)}
    return sorted(bs)


def target_exists(edge, v, Nx):
    """Windows the oracle's formula can produce: imax <= 1 and imin >= Nx - 2 fall to its resets
    (pmax := x0 + c when pmax - step < x0, pmin := x_last - c when pmin + step >= x_last)."""
    return (0 <= v <= Nx - 3) if edge == "imin" else (2 <= v <= Nx)


class _Win:
    """The oracle's window of the probe of one grid."""

    def __init__(self, orc, x, w, ix):
        self.orc, self.x = orc, x
        self.x0, self.step = float(x[0]), float(x[1] - x[0])
        self.G, self.a1 = float(w["params_true"][ix["G"]]), float(w["params_true"][ix["a1"]])

    def __call__(self, fc, c):
        return self.orc.truncation_window(self.x, float(fc), self.a1, self.G, 0, float(c))

    def solve(self, edge, v, c):
        """fc whose window has `edge` == v, from the formula, checked with the oracle (a rounding miss: another fraction)."""
        hw = c * self.G * 2.2
        for frac in (0.5, 0.25, 0.75, 0.375, 0.625):
            fc = self.x0 + (v + frac) * self.step + hw if edge == "imin" else self.x0 + (v - frac) * self.step - hw
            st, a, b = self(fc, c)
            if st == 0 and (a if edge == "imin" else b) == v:
                return fc
        return None

    def adjacent(self, edge, v, c):
        """The two adjacent doubles of fc between which `edge` steps from v - 1 to v."""
        k = 1 if edge == "imin" else 2
        lo, hi = self.solve(edge, v - 1, c), self.solve(edge, v, c)
        if lo is None or hi is None:
            return None
        while np.nextafter(lo, np.inf) < hi:
            mid = lo + 0.5 * (hi - lo)
            if self(mid, c)[k] >= v:
                hi = mid
            else:
                lo = mid
        return lo, hi


def edge_chains(orc, Nx, full=True):
    """The chains of one grid of part B.  Returns a case dict: w, ix, x, P, T, y and `chains`, one record per chain:
    kind, b (boundary), edge ('imin' / 'imax' / None), v (target value of that edge), fc, c, win (target (imin, imax) or
    None), status (expected), e_in / e_out (edge bin inside the window / first bin outside, or -1), M_in / M_out (oracle
    model of the chain there), h_in / h_out (the probe's value there)."""
    w, ix = edge_base(Nx)
    x = w["x"]
    base = w["params_true"]
    win = _Win(orc, x, w, ix)
    c0, G = float(base[ix["c"]]), float(base[ix["G"]])
    recs, missing = [], []

    def add(kind, b, fc, c, edge=None, v=None, window=None, status=0, special=None):
        recs.append(dict(kind=kind, b=b, fc=fc, c=c, edge=edge, v=v, win=window, status=status, special=special))

    bs = boundaries(Nx, full)
    for b in bs:
        for kind in KINDS:
            edge, v = kind[:4], b + {"b": 0, "b-1": -1, "b+1": 1}[kind[6:]]
            if not target_exists(edge, v, Nx):
                continue
            fc = win.solve(edge, v, c0)
            if fc is None:
                missing.append((kind, b))
                continue
            add(kind, b, fc, c0, edge, v)
        # both edges inside one unit, one bin wide: [b - 1, b) and [b, b + 1)
        c7 = 0.25 * win.step / (2.2 * G)
        for lo in (b - 1, b):
            if not 0 <= lo <= Nx - 2:
                continue
            fc = win.x0 + (lo + 0.5) * win.step
            if win(fc, c7) == (0, lo, lo + 1):
                add(ONE_BIN, b, fc, c7, window=(lo, lo + 1))
            else:
                missing.append((ONE_BIN, b))
    # near-integer quotients: adjacent doubles of fc on either side of a step of imin (imax) at ten boundaries
    inner = [b for b in bs if b % UNIT == 0 and target_exists("imin", b - 1, Nx) and target_exists("imax", b - 1, Nx)
             and target_exists("imin", b, Nx)]
    for b in [inner[int(k)] for k in np.linspace(0, len(inner) - 1, min(10, len(inner))).astype(int)]:
        for edge in ("imin", "imax"):
            pair = win.adjacent(edge, b, c0)
            if pair is None:
                missing.append(("ulp-" + edge, b))
                continue
            add(f"ulp-{edge}-below", b, pair[0], c0, edge, b - 1)
            add(f"ulp-{edge}-at", b, pair[1], c0, edge, b)
    # clamps: the probe far below / above the grid (the pmax := x0 + c and pmin := x_last - c resets), the whole grid
    add("clamp-below", 0, win.x0 - 500.0, c0)
    add("clamp-above", Nx, float(x[-1]) + 500.0, c0)
    add("clamp-whole", Nx, win.x0 + 0.5 * Nx * win.step, 200.0, window=(0, Nx))
    for r in recs[-3:-1]:
        st, a, b_ = win(r["fc"], r["c"])
        assert st == 0
        r["win"] = (a, b_)
    # chains that do not evaluate, spread through the batch: an empty window of ONE multiplet (c = 0 and the probe on a
    # grid point whose quotient is an integer: floor == ceil), a negative trunc_c (every window empty), a NaN
    j_empty = next((j for j in list(range(Nx // 2, Nx)) + list(range(1, Nx // 2)) if win(float(x[j]), 0.0)[0] == orc.EMPTY_WINDOW), None)
    specials = [dict(kind="empty-all", b=0, fc=float(base[ix["fc"]]), c=-1.0, status=2, special=None),
                dict(kind="nan", b=0, fc=float(base[ix["fc"]]), c=c0, status=1, special="nan")]
    if j_empty is not None:       # (a grid none of whose points has an integer quotient does without)
        specials.insert(0, dict(kind="empty-one", b=j_empty, fc=float(x[j_empty]), c=0.0, status=2, special=None))
    ns = len(specials)
    chains, k = [], 0
    for i, r in enumerate(recs):
        if i % 97 == 48:
            chains.append(dict(specials[k % ns], edge=None, v=None, win=None))
            k += 1
        chains.append(r)
    for sp in specials:
        if sp["kind"] not in {c["kind"] for c in chains}:
            chains.append(dict(sp, edge=None, v=None, win=None))
    n = len(chains)
    P = np.tile(base, (n, 1))
    for i, r in enumerate(chains):
        P[i, ix["fc"]], P[i, ix["c"]] = r["fc"], r["c"]
        if r["special"] == "nan":
            P[i, ix["N0"]] = np.nan
    T = synth.temperatures(8)[np.arange(n) % 8]
    # the spectrum: noise around the base chain's model, then y_e = Y_OVER_M * M_e at every targeted edge bin
    m0, st0 = orc.model(2, base, w["plength"], x)
    assert st0 == 0 and np.all(m0 > 0)
    y = m0 * _noise(Nx)
    dummy = np.ones(Nx)
    for i0 in range(0, n, 64):
        sl = slice(i0, min(i0 + 64, n))
        _, st, models = orc.generate_batch(2, w["plength"], x, dummy, P[sl], T[sl], want_models=True)
        for i, r in enumerate(chains[sl], start=i0):
            r["e_in"] = r["e_out"] = -1
            if r["edge"] is None or st[i - i0] != 0:
                continue
            e_in, e_out = (r["v"], r["v"] - 1) if r["edge"] == "imin" else (r["v"] - 1, r["v"])
            for name, e in (("in", e_in), ("out", e_out)):
                if 0 <= e < Nx:
                    r["e_" + name] = e
                    r["M_" + name] = float(models[i - i0, e])
                    r["h_" + name] = PROBE_H / (1.0 + 4.0 * ((x[e] - r["fc"]) / G) ** 2)
                    y[e] = Y_OVER_M * r["M_" + name]
    return dict(tag=f"B Nx={Nx}", mid=2, w=w, ix=ix, x=x, y=y, sigma=None, like=0, P=P, T=T, chains=chains, missing=missing,
                boundaries=bs)


_EDGE = {}


def edge_case(orc, Nx):
    if Nx not in _EDGE:
        _EDGE[Nx] = edge_chains(orc, Nx, full=Nx in EDGE_GRIDS)
    return _EDGE[Nx]


def edge_logL(orc, case):
    """Oracle logL, status and analytic gradient of all chains of an edge case (cached: both tile modes share them)."""
    key = ("B", case["x"].size)
    if key not in _ORACLE:
        w = case["w"]
        L, st = orc.generate_batch(2, w["plength"], case["x"], case["y"], case["P"], case["T"])
        ok = st == 0
        g, gabs, _, gst = orc.grad_analytic(2, w["plength"], case["x"], case["y"], case["P"][ok], case["T"][ok], w["index_to_relax"])
        _ORACLE[key] = dict(L=L, st=st, ok=ok, g=g, gabs=gabs, gst=gst)
    return _ORACLE[key]


def teeth(case, L):
    """What one mislaid bin at the targeted edge would cost every chain that targets an edge, as a share of |logL|:
    a dropped bin (the edge bin inside the window) moves logL/T by |log(1 - h/M) + y (1/(M - h) - 1/M)| / T, a wrongly
    added one (the first bin outside) by the same with M + h.  Returns (chain indices, min over the two of delta / |logL|)."""
    idx, share = [], []
    for i, r in enumerate(case["chains"]):
        if r["edge"] is None:
            continue
        d = []
        for name, sign in (("in", -1.0), ("out", 1.0)):
            e = r["e_" + name]
            if e < 0:
                continue
            M, h, ye = r["M_" + name], r["h_" + name], case["y"][e]
            d.append(abs(math.log1p(sign * h / M) + ye * (1.0 / (M + sign * h) - 1.0 / M)) / case["T"][i])
        idx.append(i)
        share.append(min(d) / abs(L[i]))
    return np.array(idx), np.array(share)


# ---------------------------------------------------------------------------------------------------------------------
# C. multiplet counts: the lane-group switches of the setup kernel (16 / 32 / 64, a second trip above 64) and TM_MAXMULT = 256

MULT_SHAPES = [(16, 0), (17, 0), (32, 0), (33, 0), (64, 0), (65, 0), (4, 3), (8, 3), (16, 3), (85, 2), (64, 3), (128, 1)]   # (Nmax, lmax)
MULT_IDS = (2, 13)
MULT_REFUSED = (86, 2)        # 258 multiplets: tamcmc_ctx_create must refuse


def mult_case(orc, mid, Nmax, lmax, Nx=20000, nchains=3):
    w = W.layout(mid, lmax, Nmax=Nmax, Nx=Nx)
    m, st = orc.model(mid, w["params_true"], w["plength"], w["x"])
    assert st == 0 and np.all(np.isfinite(m)) and np.all(m > 0), (mid, Nmax, lmax, st)
    return dict(tag=f"C id {mid} {Nmax}x{lmax + 1} = {Nmax * (lmax + 1)} multiplets", mid=mid, w=w, y=m * _noise(Nx), sigma=None,
                like=0, P=W.perturbed(w, nchains, scale=0.003), T=synth.temperatures(nchains), row=0, n_mult=Nmax * (lmax + 1))


# The backward kernel's tables live in LDS; tamcmc_ctx_set_vars refuses variables whose tables would not fit.  The sum
# below restates the launcher's (tamcmc_backward.hip, tm_backward_lds_base) for the global ids other than 9.  It is a
# PRECONDITION helper: the tests use it to choose layouts and variable counts on either side of the bound and beyond
# the point where the per-multiplet records (352 bytes each) no longer fit beside the tables; what they assert is the
# library's behaviour (accepted: the gradient equals the oracle's; refused: E_NOGRAD and nothing changed).
BW_LDS_MAX = 150 * 1024       # dynamic LDS of a workgroup at most: 160 KB per CU less ~9.3 KB of static tables
BW_AUX_STAGED = 100 * 1024    # the records are staged in LDS while tables + records stay within this
NEAR_LIMIT_SHAPE = (60, 2)    # 180 multiplets with every entry a variable: 311 (id 2) / 488 (id 13) variables


def grad_tiles(Nx):
    units = (Nx + UNIT - 1) // UNIT
    assert 4 < units < 70     # the short-grid rule of tm_tiles
    s = max(units // 10, 1)
    return (units + s - 1) // s


def backward_lds_bytes(w, nvars):
    pl = w["plength"]
    assert w["model_case"] in (2, 3, 6, 7, 8, 10, 12, 13)
    assert int(pl.sum()) == w["params_true"].size
    return longgrids.backward_lds_bytes(w, nvars, grad_tiles(w["x"].size))     # (the sum itself: any tile count)


def records_bytes(w):
    return int(w["plength"][0]) * (int(w["plength"][1]) + 1) * 352


def spread_vars(w, n):
    """n variables of a global layout: eta, a3 and the asymmetry, every relaxed entry of the splitting block (a1 or the
    inclination pair) and of the noise block, and heights / visibilities / frequencies / widths (/ m-heights) spread evenly."""
    b = W.split(w)
    idx = [int(i) for i in w["index_to_relax"]]
    must = {b["s"] + 1, b["s"] + 2, b["s"] + 5} | {i for i in idx if b["s"] <= i < b["s"] + 6 or b["z"] <= i < b["z"] + 10}
    rest = [i for i in idx if i not in must]
    pick = {rest[int(k)] for k in np.linspace(0, len(rest) - 1, n - len(must))}
    out = np.array(sorted(must | pick), dtype=np.int32)
    assert n - 8 <= out.size <= n
    return out
