"""Cases and restated rules of the long-grid suite (tests/test_long_grids_host.py, tests/test_long_grids_gpu.py).  Test
helper only; no GPU.

tamcmc_ctx_create accepts 2 <= Nx <= 2^28.  Between 1.2e6 bins -- the longest grid of the other suites -- and that limit
the library changes behaviour at these points, and every case here stands on one side of one of them at the library's
own default geometry (B), or reaches it on a short grid through a tile count given by hand (C):

  1  TM_EQ_MAXU = 4096 units: under TAMCMC_EQUAL_COST=1 a grid of 4095 units is balanced with one unit of slack, one of
     4096 has no slack (tiles of equal length), one of 4097 is too long for the LDS prefix of the unit costs;
  2  TM_ORDER_MAX = 1024 tiles: up to it the setup kernel ranks a chain's tiles (s_cost and its four pad slots), above
     it the rank table is the identity -- 8192 / 8193 units in the likelihood launch, 7124 / 7125 in the gradient
     launch with its tail of 4-unit tiles;
  3  65535 tiles: above it the eval launch is chain-major, grid = (tiles, chains), with the slot rotation;
  4  the backward kernel's table of tile starts in LDS: 4 bytes per gradient tile beside the tables of the layout;
  5  a multiplet's window spanning hundreds of gradient tiles, or all of them;
  6  the in-launch finalize of the likelihood launch at 1025 tiles and more.

The functions below RESTATE tm_units, tm_tiles, the tail rule of tamcmc_ctx_create, tm_setup_balances and
tm_backward_lds_base; the GPU tests assert them against tamcmc_ctx_geometry / tamcmc_ctx_geometry_grad and against what
tamcmc_ctx_set_vars accepts, so that a case cannot drift to the wrong side of its threshold unnoticed."""
import numpy as np

import workloads as W
from tamcmc_amd import synth

UNIT = 512
TILE_MAXU = 8            # TM_TILE_MAXU: units per gradient tile (and per balanced tile) at most
TILE_MAXU_L = 16         # TM_TILE_MAXU_L
EQ_MAXU = 4096           # TM_EQ_MAXU
ORDER_MAX = 1024         # TM_ORDER_MAX
GRID_Y_MAX = 65535       # tiles above this: chain-major launch (tm_eval_args)
TILES_ENV_MAX = 1 << 20  # TAMCMC_TILES / TAMCMC_TILES_GRAD accepted up to this

BW_LDS_MAX = 150 * 1024      # TM_BW_LDS_MAX
BW_AUX_STAGED = 100 * 1024   # the per-multiplet records are staged in LDS while tables + records stay within this
BW_ATTR = 48 * 1024          # more dynamic LDS than this needs hipFuncSetAttribute
RECORD_BYTES = 352           # sizeof(TmMultFull)


# ---------------------------------------------------------------------------------------------------------------------
# A. restated geometry

def units_of(Nx):
    return (Nx + UNIT - 1) // UNIT


def tiles_of(units):
    """tm_tiles (tamcmc_dev.h)."""
    if units <= 4:
        return 1
    if units < 70:
        s = max(units // 10, 1)
        return (units + s - 1) // s
    return (units + TILE_MAXU - 1) // TILE_MAXU


def grad_geometry(units, equal_cost=0, frac=85, su2=4):
    """(tiles_g, t1, su1, su2) of the gradient launch at the default switches: tm_tiles, then the tail rule of
    tamcmc_ctx_create (85 % of the units in 8-unit tiles, the rest in 4-unit tiles; off below 70 units and under
    TAMCMC_EQUAL_COST=1).  t1 = 0: all tiles alike."""
    tiles = tiles_of(units)
    if units >= 70 and not equal_cost:
        t1 = (units * frac // 100 + TILE_MAXU // 2) // TILE_MAXU
        rest = units - t1 * TILE_MAXU
        if t1 >= 1 and rest > 0:
            return t1 + (rest + su2 - 1) // su2, t1, TILE_MAXU, su2
    return tiles, 0, 0, 0


def grad_tile_of_unit(units, u, equal_cost=0):
    """tm_tile_of_unit for tiles of equal length (the default geometry of the gradient launch)."""
    tiles, t1, su1, su2 = grad_geometry(units, equal_cost)
    if t1 <= 0:
        return u // ((units + tiles - 1) // tiles)
    return u // su1 if u < t1 * su1 else t1 + (u - t1 * su1) // su2


def likelihood_max_units(units, tiles, equal_cost):
    """cost_l.pad of tamcmc_ctx_create: the bound on a likelihood tile's length."""
    return TILE_MAXU if (equal_cost and tiles * TILE_MAXU > units) else TILE_MAXU_L


def balances(units, tiles, equal_cost, max_units_per_tile=TILE_MAXU):
    """tm_setup_balances (tamcmc_dev.h): per-chain boundaries of equal cost, or tiles of equal length."""
    return bool(equal_cost and max_units_per_tile == TILE_MAXU and 1 < tiles <= ORDER_MAX and units <= EQ_MAXU
                and tiles * TILE_MAXU > units)


def backward_lds_bytes(w, nvars, tiles):
    """tm_backward_lds_base (tamcmc_backward.hip) for the global ids other than 9: the backward kernel's dynamic LDS
    without the staged records, for `tiles` gradient tiles."""
    pl = w["plength"]
    assert w["model_case"] in (2, 3, 6, 7, 8, 10, 12, 13)
    Np, nm = int(pl.sum()), int(pl[0]) * (int(pl[1]) + 1)
    npairs = nm * 12 + 64
    return ((Np + nvars) * 8 + npairs * 8 + nm * (20 + 24 + 1) * 8 + 16 + ((npairs + 7) & ~7) * 4 + ((tiles + 2) & ~1) * 4
            + ((Np + 1) & ~1) * 4 + 8 * nvars * 8)


def records_bytes(w):
    return int(w["plength"][0]) * (int(w["plength"][1]) + 1) * RECORD_BYTES


def largest_tiles_within(w, nvars, limit, records=False):
    """Largest gradient tile count whose restated sum (plus the records) stays within `limit` bytes."""
    extra = records_bytes(w) if records else 0
    fixed = backward_lds_bytes(w, nvars, 0) + extra - 2 * 4        # (tiles = 0 carries ((0 + 2) & ~1) * 4 = 8 bytes)
    t = (limit - fixed) // 4 - 2
    t -= t % 2                                                       # ((t + 2) & ~1): even t and t + 1 cost the same
    while backward_lds_bytes(w, nvars, t + 1) + extra <= limit:
        t += 1
    assert backward_lds_bytes(w, nvars, t) + extra <= limit < backward_lds_bytes(w, nvars, t + 1) + extra
    return t


# ---------------------------------------------------------------------------------------------------------------------
# B. long grids at the default geometry

_NOISE = None


def _noise(n):
    """-ln u of one seeded draw shared by all grids (4.2e6 values; the first n)."""
    global _NOISE
    if _NOISE is None or _NOISE.size < n:
        _NOISE = -np.log1p(-np.random.default_rng(20240611).random(max(n, UNIT * 8193)))
    return _NOISE[:n]


def Nx_of(units, exact=False):
    return UNIT * units if exact else UNIT * units - 37


# name -> units, exact multiple of 512, environment, what it stands beside.  `side` is checked on the host (restated
# rule) and on the GPU (the library's own accessors).
def _b(units, exact=False, env=None, kind="star", item=0, **side):
    return dict(units=units, exact=exact, env=dict(env or {}), kind=kind, item=item, side=side)


CASES = {}
for _u in (4095, 4096, 4097):
    for _x in ((False, True) if _u == 4096 else (False,)):
        for _ec in (0, 1):
            CASES[f"u{_u}{'x' if _x else ''}-equal-cost-{_ec}"] = _b(
                _u, _x, {"TAMCMC_EQUAL_COST": str(_ec)}, item=1, balanced=bool(_ec and _u == 4095))
CASES["u8192-likelihood-1024-tiles"] = _b(8192, item=2, tiles=1024)
CASES["u8192x-likelihood-1024-tiles"] = _b(8192, True, item=2, tiles=1024)
CASES["u8192-likelihood-1024-tiles-prio"] = _b(8192, env={"TAMCMC_PRIO": "1"}, item=2, tiles=1024)
CASES["u8193-likelihood-1025-tiles"] = _b(8193, item=2, tiles=1025)
CASES["u7124-gradient-1024-tiles"] = _b(7124, item=2, tiles_grad=1024)
CASES["u7125-gradient-1025-tiles"] = _b(7125, item=2, tiles_grad=1025)
CASES["u8193-window-spans-all-tiles"] = _b(8193, kind="nine-wide", item=5, tiles=1025)
WINDOW_CASE, WIDE_CASE = "u8193-likelihood-1025-tiles", "u8193-window-spans-all-tiles"


def expected_geometry(name):
    """(tiles_l, tiles_g, balanced_l, balanced_g) of a case by the restated rules."""
    c = CASES[name]
    u, ec = c["units"], int(c["env"].get("TAMCMC_EQUAL_COST", "0"))
    tl, tg = tiles_of(u), grad_geometry(u, ec)[0]
    return tl, tg, balances(u, tl, ec, likelihood_max_units(u, tl, ec)), balances(u, tg, ec)


_BUILT = {}


def build(orc, name):
    """The inputs of a case: one synthetic star stretched over the grid (the 21-multiplet benchmark layout, 44
    variables) with 3 chains at distinct temperatures -- the tests evaluate the first two, and all three once for the
    batch-independence check; `nine-wide`: the 9-multiplet layout with trunc_c = 10000 (every window the whole grid),
    one chain evaluated.  Cases on the same grid share their inputs."""
    c = CASES[name]
    Nx = Nx_of(c["units"], c["exact"])
    key = (c["kind"], Nx)
    if key not in _BUILT:
        if c["kind"] == "star":
            w = synth.workload_c2(Nx=Nx)
            w["x"] = synth.grid(Nx, 2300.0, 840.0 / Nx)
            P, n_eval = synth.chain_params(w, 3), 2
        else:
            w = W.layout(2, 2, Nmax=3, Nx=Nx, trunc_c=10000.0)
            P, n_eval = W.perturbed(w, 2, scale=0.003), 1
        m, st = orc.model(2, w["params_true"], w["plength"], w["x"])
        _BUILT[key] = dict(key=key, mid=2, w=w, Nx=Nx, truth_ok=bool(st == 0 and np.all(np.isfinite(m)) and np.all(m > 0)),
                           y=m * _noise(Nx), P=P, T=synth.temperatures(4)[1:1 + len(P)], n_eval=n_eval)
    return dict(_BUILT[key], name=name, env=c["env"], units=c["units"], side=c["side"], item=c["item"])


_ORACLE = {}


def oracle_answers(orc, case):
    """Oracle logL, status and analytic gradient of the chains a case evaluates; once per grid."""
    key = case["key"]
    if key not in _ORACLE:
        w, n = case["w"], case["n_eval"]
        g, gabs, L, st = orc.grad_analytic(case["mid"], w["plength"], w["x"], case["y"], case["P"][:n], case["T"][:n],
                                           w["index_to_relax"])
        L2, st2 = orc.generate_batch(case["mid"], w["plength"], w["x"], case["y"], case["P"][:n], case["T"][:n])
        assert np.array_equal(L, L2) and np.array_equal(st, st2)      # the gradient is taken at the oracle's own evaluation
        _ORACLE[key] = dict(L=L, st=st, g=g, gabs=gabs)
    return _ORACLE[key]


def l0_windows(orc, case, row=None):
    """The oracle's truncation windows [imin, imax) of the l = 0 modes of a params row (default: the truth)."""
    w = case["w"]
    p = w["params_true"] if row is None else row
    b = W.split(w)
    out = []
    for k in range(b["Nmax"]):
        st, lo, hi = orc.truncation_window(w["x"], float(p[b["Nmax"] + b["lmax"] + k]), float(p[b["s"]]), float(p[b["w"] + k]), 0,
                                           float(p[b["cfg"]]))
        assert st == 0
        out.append((lo, hi))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# C. tile counts by hand on a short grid

SHORT_NX = 2560                           # 5 units: the shortest grid on which TAMCMC_TILES / TAMCMC_TILES_GRAD are read
HAND_TILES = (65535, 65536, 70001)        # (tiles - 1) & 7 = 6, 7, 0: the slot rotation of the chain-major launch
SHORT_LAYOUTS = ("nine", "star")


def short_case(orc, layout):
    """3 chains on 2560 bins: the 9-multiplet layout with all its variables, or the benchmark layout with its 44."""
    key = ("short", layout)
    if key not in _BUILT:
        if layout == "nine":
            w = W.layout(2, 2, Nmax=3, Nx=SHORT_NX)
            P = W.perturbed(w, 3, scale=0.003)
        else:
            w = synth.workload_c2(Nx=SHORT_NX)
            w["x"] = synth.grid(SHORT_NX, 2300.0, 840.0 / SHORT_NX)
            P = synth.chain_params(w, 3)
        m, st = orc.model(2, w["params_true"], w["plength"], w["x"])
        _BUILT[key] = dict(key=key, mid=2, w=w, Nx=SHORT_NX, truth_ok=bool(st == 0 and np.all(np.isfinite(m)) and np.all(m > 0)),
                           y=m * _noise(SHORT_NX), P=P, T=synth.temperatures(4)[1:4], n_eval=3, name=f"short-{layout}", units=5)
    return _BUILT[key]


def short_oracle(orc, case, idx=None, rows=(1,)):
    """Oracle logL, status, model rows and gradient (variables idx, default all) of a short case; memoized."""
    w = case["w"]
    idx = w["index_to_relax"] if idx is None else np.asarray(idx, dtype=np.int32)
    key = (case["key"], tuple(idx.tolist()))
    if key not in _ORACLE:
        L, st, m = orc.generate_batch(case["mid"], w["plength"], w["x"], case["y"], case["P"], case["T"], want_models=True)
        g, gabs, _, gst = orc.grad_analytic(case["mid"], w["plength"], w["x"], case["y"], case["P"], case["T"], idx)
        _ORACLE[key] = dict(L=L, st=st, rows=list(rows), models=m[list(rows)].copy(), g=g, gabs=gabs, gst=gst)
    return _ORACLE[key]


def lds_points(w, nvars):
    """Gradient tile counts of a short case at the three LDS switches: (largest accepted T*, largest with the records
    staged, largest below the 48 KB attribute path)."""
    t_star = largest_tiles_within(w, nvars, BW_LDS_MAX)
    t_aux = largest_tiles_within(w, nvars, BW_AUX_STAGED, records=True)
    t_attr = largest_tiles_within(w, nvars, BW_ATTR, records=True)
    return t_star, t_aux, t_attr
