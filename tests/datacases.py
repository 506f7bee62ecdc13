"""Builders of the data-side suite (tests/test_data_values_host.py, tests/test_data_values_gpu.py).  Test helper only; no GPU.

The rest of the suite varies the parameters; here the DATA a context is created with (x, y, sigma_y), the chain
temperatures and likelihood_p leave the one decade of magnitude that synth.make_spectrum gives them:

  A  the same star in other units of power: everything the model is linear in, and y (and sigma_y), times
     s = 1e-12, 1e12, 2^-200, 2^200;
  B  one datum (or one sigma_y, or one temperature) set to 0, a negative value, 5e-324, 1e300, +inf, NaN; an all-zero
     spectrum; likelihood_p = 0, 0.9, -1, 3;
  C  grids that start at x = 0 (log x = -inf in the first bin);
  D  (GPU file only) tamcmc_eval_batch_device with a gradient buffer.

The judge is the oracle (oracle/pyoracle.py); tests/test_data_values_host.py proves on the CPU that the cases are what
they claim."""
import numpy as np

import edgecases as E
import layouts
import workloads as W
from tamcmc_amd import synth

NCHAINS = 3
GRIDS = layouts.GRIDS                                  # fused: 1900 bins (one tile), tiled: 28 000 bins (55 units)

# ---------------------------------------------------------------------------------------------------------------------
# A. power units

SCALES = {"1e-12": (1e-12, None), "1e12": (1e12, None), "2^-200": (2.0 ** -200, -200), "2^200": (2.0 ** 200, 200)}   # name -> (s, k)
POWER_KINDS = ("id2", "id13", "id11", "id1", "id2-chi2")


def power_workload(kind, Nx):
    """(workload, likelihood id) of a part-A kind."""
    if kind in ("id2", "id2-chi2"):
        return W.layout(2, 3, Nmax=3, Nx=Nx), int(kind == "id2-chi2")
    if kind == "id13":
        return W.layout(13, 3, Nmax=3, Nx=Nx), 0
    if kind == "id11":
        return W.layout(11, Nx=Nx), 0
    if kind == "id1":
        return W.make_gauss(1, Nx=Nx), 0
    raise ValueError(kind)


def linear_entries(w):
    """Indices of the params row the model is linear in (|.| of them, where the model takes it): heights or squared
    amplitudes, the id-13 height block, every Harvey H_k, the white noise, the Gaussian amplitude.  Visibilities,
    m-height ratios, taus, exponents, frequencies, widths are not among them."""
    mid, pl = int(w["model_case"]), [int(v) for v in w["plength"]]
    if mid == 1:
        return np.array([0, 3, 6])                     # Gaussian amplitude, Harvey H, white noise
    z = sum(pl[:8])
    idx = list(range(pl[0]))                           # heights (or amplitudes^2) of l = 0 / of every local mode
    idx += [z + 3 * k for k in range((pl[8] - 1) // 3)] + [z + pl[8] - 1]
    if mid == 13:
        idx += list(range(z + pl[8], z + pl[8] + pl[9]))
    return np.array(sorted(idx))


def _model(orc, w, params=None):
    m, st = orc.model(int(w["model_case"]), w["params_true"] if params is None else params, w["plength"], w["x"])
    assert st == 0 and np.all(np.isfinite(m)) and np.all(m > 0), (w["model_case"], st)
    return m


def base_case(orc, kind, grid, w=None, like=None, nchains=NCHAINS):
    """The unscaled case: spectrum = the oracle's model of params_true times make_spectrum's noise stream."""
    if w is None:
        w, like = power_workload(kind, GRIDS[grid])
    Nx = w["x"].size
    y = _model(orc, w) * E._noise(Nx)
    sig = 0.05 + 0.2 * np.abs(np.sin(np.arange(Nx))) if like == 1 else None
    return dict(tag=f"{kind} {grid}", kind=kind, grid=grid, mid=int(w["model_case"]), w=w, y=y, sigma=sig, like=like, p=1.0,
                P=W.perturbed(w, nchains, scale=0.003), T=synth.temperatures(nchains), row=Nx % nchains,
                lin=linear_entries(w))


def scaled(case, s, scale_params=None):
    """The case in units of power s times smaller (data and every linear entry times s).  scale_params: the entries
    to scale, default the case's linear entries."""
    idx = case["lin"] if scale_params is None else scale_params
    P = case["P"].copy()
    P[:, idx] *= s
    w = dict(case["w"])
    w["params_true"] = case["w"]["params_true"].copy()
    w["params_true"][idx] *= s
    return dict(case, tag=f"{case['tag']} x {s:.3g}", w=w, y=case["y"] * s, sigma=None if case["sigma"] is None else case["sigma"] * s,
                P=P, s=s)


_CACHE = {}


def power_case(orc, kind, grid, scale=None):
    key = ("A", kind, grid, scale)
    if key not in _CACHE:
        _CACHE[key] = base_case(orc, kind, grid) if scale is None else scaled(power_case(orc, kind, grid), SCALES[scale][0])
    return _CACHE[key]


def answers(orc, key, case, grad=True):
    """Oracle logL, status, the case's one model row and (grad) the analytic gradient; once per key."""
    key = ("ans",) + tuple(key)
    if key in _CACHE:
        return _CACHE[key]
    w = case["w"]
    L, st, rm = orc.generate_batch(case["mid"], w["plength"], w["x"], case["y"], case["P"], case["T"], sigma_y=case["sigma"],
                                   likelihood_case=case["like"], likelihood_p=case["p"], want_models=True)
    ans = dict(L=L, st=st, rows=[case["row"]], models=rm[[case["row"]]].copy())
    if grad:
        ans["g"], ans["gabs"], gL, ans["gst"] = orc.grad_analytic(case["mid"], w["plength"], w["x"], case["y"], case["P"], case["T"],
                                                                  w["index_to_relax"], sigma_y=case["sigma"],
                                                                  likelihood_case=case["like"], likelihood_p=case["p"])
    _CACHE[key] = ans
    return ans


LN2 = np.log(np.longdouble(2.0))


def identity_residual(L_s, L_1, T, p, Nx, log_s):
    """|L(s) + p Nx ln(s) / T - L(1)| per chain, in long double: chi(2,2p) in units of power s times smaller is the same
    likelihood plus p Nx ln s (every y/M is unchanged, every ln M grows by ln s)."""
    L_s, L_1, T = (np.asarray(a, dtype=np.longdouble) for a in (L_s, L_1, T))
    return np.abs(L_s + np.longdouble(p) * Nx * np.longdouble(log_s) / T - L_1)


# ---------------------------------------------------------------------------------------------------------------------
# B. special data, temperatures and likelihood_p

DATA_VALUES = (0.0, -3.0, 5e-324, 1e300, np.inf, np.nan)
DATA_STATUS = {0.0: (0, "finite"), -3.0: (0, "finite"), 5e-324: (0, "finite"), 1e300: (0, "finite"), np.inf: (0, "-inf")}   # NaN: (1, "nan")
SIGMA_VALUES = (0.0, -0.3, np.inf, np.nan, 1e-200, 1e200)
T_VALUES = (0.0, 5e-324, 1e-300, 1e300, np.inf, -2.0, np.nan)
P_VALUES = (0.0, 0.9, -1.0, 3.0)
SPECIAL_KINDS = {"id2": "tiled", "id11": "fused"}
TILE_BINS = 5 * E.UNIT                                 # equal-length tiles of the 55-unit grid (layouts.py)


def expected_kind(v):
    return (1, "nan") if v != v else DATA_STATUS[v]


def special_bins(orc, w):
    """{'in-window', 'outside', 'tile-first-row', 'last-partial-unit'} -> bin.  A bin is outside every window exactly where
    the model equals the model with every height zero (a Lorentzian is never 0 inside its window)."""
    Nx = w["x"].size
    full = _model(orc, w)
    p0 = w["params_true"].copy()
    assert int(w["model_case"]) in (2, 11)             # every height is, or is a multiple of, one of the first plength[0] entries
    p0[:int(w["plength"][0])] = 0.0
    bare, st = orc.model(int(w["model_case"]), p0, w["plength"], w["x"])
    assert st == 0
    out = np.flatnonzero(full == bare)
    inside = np.flatnonzero(full != bare)
    assert out.size > 0 and inside.size > 0
    peak = int(np.argmax(full - bare))
    units = (Nx + E.UNIT - 1) // E.UNIT
    assert Nx % E.UNIT != 0
    bins = {"in-window": peak, "outside": int(out[out.size // 2]),
            "tile-first-row": (TILE_BINS * 3 if units > 4 else 0) + 7, "last-partial-unit": Nx - 1}
    assert full[peak] != bare[peak] and bins["last-partial-unit"] >= E.UNIT * (units - 1)
    return bins


def special_workload(kind, Nx):
    if kind == "id2":
        return W.layout(2, 3, Nmax=3, Nx=Nx, trunc_c=3.0)     # trunc_c = 3: bins outside every window exist
    return W.layout(11, Nx=Nx, trunc_c=3.0)


def special_data_case(orc, kind):
    """One multi-spectrum chi(2,2p) case: spectra[0] is the base, then one copy per (value, place) with that bin set to the
    value, last an all-zero spectrum.  `batches`: lists of (chain's spectrum, chain's params row, T) of at most 16 chains,
    healthy chains (spectrum 0) between the damaged ones."""
    key = ("B", kind)
    if key in _CACHE:
        return _CACHE[key]
    grid = SPECIAL_KINDS[kind]
    case = base_case(orc, kind, grid, w=special_workload(kind, GRIDS[grid]), like=0)
    bins = special_bins(orc, case["w"])
    spectra, what = [case["y"]], [("base", None, None)]
    for v in DATA_VALUES:
        for place, i in bins.items():
            y = case["y"].copy()
            y[i] = v
            spectra.append(y)
            what.append((place, i, v))
    spectra.append(np.zeros_like(case["y"]))
    what.append(("all-zero", None, 0.0))
    case.update(spectra=np.stack(spectra), what=what, bins=bins, batches=_batches(len(spectra), case))
    _CACHE[key] = case
    return case


def _batches(nspec, case, per=12):
    """Damaged spectra `per` at a time, a chain on the base spectrum in front, after every fourth and behind."""
    out = []
    T3 = case["T"]
    for s0 in range(1, nspec, per):
        smap = []
        for k, s in enumerate(range(s0, min(s0 + per, nspec))):
            if k % 4 == 0:
                smap.append(0)
            smap.append(s)
        smap.append(0)
        rows = np.arange(len(smap)) % len(case["P"])
        out.append(dict(smap=np.array(smap, dtype=np.int32), P=case["P"][rows], T=T3[rows]))
        assert len(smap) <= 16
    return out


def sigma_case(orc):
    """Chi-square on the tiled id-2 grid: spectra share y; sigma_y[0] is the base, then one bin set to each SIGMA_VALUES."""
    key = ("B", "sigma")
    if key in _CACHE:
        return _CACHE[key]
    case = base_case(orc, "id2-chi2", "tiled", w=special_workload("id2", GRIDS["tiled"]), like=1)
    i = special_bins(orc, case["w"])["in-window"]
    sig = [case["sigma"]]
    for v in SIGMA_VALUES:
        s = case["sigma"].copy()
        s[i] = v
        sig.append(s)
    n = len(sig)
    smap = np.array([0] + list(range(1, n)) + [0], dtype=np.int32)
    rows = np.arange(smap.size) % len(case["P"])
    case.update(spectra=np.tile(case["y"], (n, 1)), sigmas=np.stack(sig), bin=i,
                batches=[dict(smap=smap, P=case["P"][rows], T=case["T"][rows])])
    _CACHE[key] = case
    return case


def temperature_batch(case):
    """Chains on the base spectrum, every second one at a special temperature."""
    T = []
    for k, v in enumerate(T_VALUES):
        T += [case["T"][k % len(case["T"])], v]
    T.append(case["T"][0])
    T = np.array(T)
    rows = np.arange(T.size) % len(case["P"])
    return dict(smap=np.zeros(T.size, dtype=np.int32), P=case["P"][rows], T=T)


def batch_answers(orc, key, case, batch, p=1.0):
    """The oracle on a batch of a multi-spectrum case: chain by chain on the chain's own spectrum (and sigma)."""
    key = ("bans",) + tuple(key)
    if key in _CACHE:
        return _CACHE[key]
    w, n = case["w"], len(batch["smap"])
    L, st = np.empty(n), np.empty(n, dtype=np.int32)
    nv = w["index_to_relax"].size
    g, gabs, gst = np.empty((n, nv)), np.empty((n, nv)), np.empty(n, dtype=np.int32)
    for s in np.unique(batch["smap"]):
        k = np.flatnonzero(batch["smap"] == s)
        sig = case["sigmas"][s] if case["like"] == 1 else None
        L[k], st[k] = orc.generate_batch(case["mid"], w["plength"], w["x"], case["spectra"][s], batch["P"][k], batch["T"][k],
                                         sigma_y=sig, likelihood_case=case["like"], likelihood_p=p)
        g[k], gabs[k], _, gst[k] = orc.grad_analytic(case["mid"], w["plength"], w["x"], case["spectra"][s], batch["P"][k],
                                                     batch["T"][k], w["index_to_relax"], sigma_y=sig, likelihood_case=case["like"],
                                                     likelihood_p=p)
    ans = dict(L=L, st=st, g=g, gabs=gabs, gst=gst)
    _CACHE[key] = ans
    return ans


def negative_model_case(orc, grid):
    """Id 0 (Gaussian + constant, the one model whose amplitude and constant do not pass through abs()): chains 0 and 2 are
    healthy, chain 1 has both negative -- EVERY model value is negative -- and chain 3 the constant alone.  The reference
    takes log of a negative number: NaN, status 1.  The device multiplies the mantissas of a tile and takes one log, so
    an even number of negative values per tile (grid and every run of whole units have an even number of bins) would
    give it a positive product: only the collected sign bits tell."""
    key = ("B", "negM", grid)
    if key in _CACHE:
        return _CACHE[key]
    case = base_case(orc, "id0", grid, w=W.make_gauss(0, Nx=GRIDS[grid]), like=0, nchains=4)
    P = case["P"].copy()
    P[1, 0], P[1, 3] = -abs(P[1, 0]), -abs(P[1, 3])
    P[3, 3] = -abs(P[3, 3])
    case.update(P=P, row=0)
    w = case["w"]
    neg = [int(np.sum(orc.model(0, p, w["plength"], w["x"])[0] < 0)) for p in P]
    Nx = w["x"].size
    assert neg[0] == 0 and neg[2] == 0 and neg[1] == Nx and 0 < neg[3] < Nx and Nx % 2 == 0 and E.UNIT % 2 == 0
    _CACHE[key] = case
    return case


def classify(L, st):
    """'finite', '-inf', '+inf', '-0', '+0' or 'nan' per chain (status in front where it is not 0)."""
    out = []
    for l, s in zip(L, st):
        k = "nan" if l != l else ("-inf" if l == -np.inf else "+inf" if l == np.inf else
                                  ("-0" if np.signbit(l) else "+0") if l == 0 else "finite")
        out.append((int(s), k))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# C. grids that start at x = 0

ZERO_KINDS = ("id2-fused", "id2-tiled", "id1", "id11")


def zero_grid_workload(kind):
    if kind == "id2-fused":
        return W.layout(2, 2, Nmax=3, grid=(0.0, 1.4), Nx=GRIDS["fused"])
    if kind == "id2-tiled":
        return W.layout(2, 2, Nmax=3, grid=(0.0, 0.1), Nx=GRIDS["tiled"])      # no polynomial cell (W.poly_cells)
    if kind == "id1":
        w = W.make_gauss(1, Nx=GRIDS["fused"])
        w["x"] = synth.grid(GRIDS["fused"], 0.0, 1.6)
        return w
    if kind == "id11":
        return W.layout(11, grid=(0.0, 0.1), Nx=GRIDS["fused"])
    raise ValueError(kind)


def harvey_entries(w):
    """{'H': [...], 'tau': [...], 'p': [...]} of the ACTIVE Harvey profiles (positions in the params row)."""
    mid, pl = int(w["model_case"]), [int(v) for v in w["plength"]]
    z, nh = (3, 1) if mid == 1 else (sum(pl[:8]), (pl[8] - 1) // 3)
    act = [k for k in range(nh) if w["params_true"][z + 3 * k + 1] != 0.0]
    return {name: [z + 3 * k + j for k in act] for j, name in enumerate(("H", "tau", "p"))}


def zero_grid_case(orc, kind):
    key = ("C", kind)
    if key not in _CACHE:
        w = zero_grid_workload(kind)
        assert w["x"][0] == 0.0
        _CACHE[key] = base_case(orc, kind, "tiled" if w["x"].size > 4 * E.UNIT else "fused", w=w, like=0)
    return _CACHE[key]
