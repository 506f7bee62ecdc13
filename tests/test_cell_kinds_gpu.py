"""The three kinds of background cells of pass 1 (tamcmc_eval_body.h, TmCellKind) and the changes between them inside one tile.

The eval kernels walk a tile cell by cell (8 units of 512 bins) and pick, where the walk enters a cell, the loops compiled
for that cell's kind: the cell's Taylor polynomial, exp() per Harvey profile and bin where the setup kernel found the
polynomial not valid, or white noise alone for a chain without an active profile.  The smallest shapes at which that
walk can go wrong: id 2 with two modes of every degree 0..3 (multiplets of 1, 3, 5 and 7 components; with degrees above 0
the library takes no fewer than two radial orders: the widths are interpolated between the l = 0 modes), 2 chains, a grid of
three cells plus a partial unit (3 * 4096 + 300 bins = 25 units), and tiles of 5 and of 3 units of equal length
(TAMCMC_TILES / TAMCMC_TILES_GRAD = 5, 9), which put an odd first unit, an odd last unit, a pair and a whole tile on
either side of a change of kind at unit 8 or 16:

  su = 5:  [5, 10)  unit 5 alone, pair 6-7 | pair 8-9          [15, 20)  unit 15 alone | pairs 16-17, 18-19
  su = 3:  [0, 3)   pair 0-1, unit 2 alone (odd last unit before the change)       [3, 6)  unit 3 alone, pair 4-5
           [6, 9)   pair 6-7 | unit 8 alone (odd last unit after the change)       [9, 12) unit 9 alone (odd first unit after it)
           [15, 18) unit 15 alone | pair 16-17                  [24, 25)  the partial unit (guarded path)

Grids (kinds by the setup kernel's own criterion, tamcmc_setup_body.h: every active profile needs p * span <= 0.04, span
the cell's half-width in log x, and t0 = (1e-3 tau x_c)^p < 1e290 -- evaluated on the CPU by cell_kinds() and asserted):
  "exp-poly"  starts at 1694.5 uHz, step 0.0084: with p = 4 the first cell is too wide in log x (p * span = 0.0404), the
              later ones are not (0.0396, 0.0388): exp -> poly at unit 8;
  "poly-exp"  the change the other way round.  The span of a cell shrinks along a uniform grid, so the first rule cannot
              give it; the second can: a profile with p = 60 whose t0 passes 1e290 between two cell centres (narrow cells:
              step 0.0005 at 2000 uHz, p * span = 0.031).  Chain 0 changes at unit 8, chain 1 (tau 0.1 % smaller) at 16.
              Where it counts that profile is below 1e-290 of the model, and the terms of its own H and tau derivatives
              sit at the underflow threshold of fp64: those two are left out of the variables;
  "no-harvey" the first grid with every tau = 0: no profile is active.

Checked per grid and tile length: status, logL (1e-10 relative) and every gradient entry (tests/gradcheck.py) against the
CPU oracle -- the bars of tests/test_grad_gpu.py; the default against TAMCMC_BG_EXACT=1 (all cells exp) at that file's
1e-13 / 1e-11; each chain alone against the same chain in the batch, bit for bit; the likelihood launch against the logL
of the gradient launch (rtol 1e-13, as tests/test_grad_gpu.py compares them)."""
import math

import numpy as np
import pytest

import gradcheck
from tamcmc_amd import synth

pytestmark = pytest.mark.gpu

UNIT, CELL_UNITS = 512, 8
NX = 3 * CELL_UNITS * UNIT + 300
UNITS = (NX + UNIT - 1) // UNIT
TILES = (5, 9)                      # equal-length tiles of 5 and of 3 units
T = np.array([1.0, 3.7])

C2_PROFILES = [11.049588, 49.669854, 4.0, 0.93569041, 1.3516447, 2.0]
WHITE = 0.13392108
# poly-exp: 1e-3 * tau * x_c = 10^(290/60) between the centres of cells 0 and 1 (chain 0) and of cells 1 and 2 (chain 1)
P60 = 60.0
X0_B, STEP_B = 2000.0, 0.0005
_XC = [X0_B + STEP_B * (ce * CELL_UNITS * UNIT + CELL_UNITS * UNIT // 2) for ce in range(3)]
TAU_B = [1e3 * 10.0 ** (290.0 / P60) / math.sqrt(_XC[k] * _XC[k + 1]) for k in (0, 1)]

GRIDS = {
    # name: (x0, step, noise block, mode frequencies of l = 0..3, width, a1, expected kinds per chain)
    "exp-poly": (1694.5, 0.0084, [0.0, 0.0, 1.0] + C2_PROFILES + [WHITE], ((1715.0, 1775.0), (1732.0, 1792.0), (1708.0, 1758.0), (1725.0, 1780.0)), 1.4, 1.4,
                 [["exp", "poly", "poly", "poly"]] * 2),
    "poly-exp": (X0_B, STEP_B, [0.4, TAU_B[0], P60] + C2_PROFILES + [WHITE], ((2001.5, 2004.6), (2003.0, 2006.0), (2001.0, 2004.5), (2002.2, 2005.5)), 0.15, 0.4,
                 [["poly", "exp", "exp", "exp"], ["poly", "poly", "exp", "exp"]]),
    "no-harvey": (1694.5, 0.0084, [0.0, 0.0, 1.0, 11.049588, 0.0, 4.0, 0.93569041, 0.0, 2.0, WHITE],
                  ((1715.0, 1775.0), (1732.0, 1792.0), (1708.0, 1758.0), (1725.0, 1780.0)), 1.4, 1.4, [["none"] * 4] * 2),
}


def cell_kinds(w, p):
    """Kind of every cell of one chain by the rule of tamcmc_setup_body.h (and the margin by which the rule decides)."""
    pl, x = w["plength"], w["x"]
    z = int(pl[:8].sum())
    prof = [(abs(p[z + 3 * k + 1]), abs(p[z + 3 * k + 2])) for k in range(3)]
    prof = [(tau, pw) for (tau, pw) in prof if tau != 0 and pw != 0]
    lx = np.log(x)
    cb = CELL_UNITS * UNIT
    kinds, margin = [], np.inf
    for ce in range((x.size + cb - 1) // cb):
        base = ce * cb
        tb = min(cb, x.size - base)
        ic, i1 = min(base + tb // 2, x.size - 1), min(base + tb - 1, x.size - 1)
        span = max(abs(lx[base] - lx[ic]), abs(lx[i1] - lx[ic]))
        ok = True
        for (tau, pw) in prof:
            lt0 = pw * (math.log(1e-3 * tau) + lx[ic])
            ok = ok and pw * span <= 0.04 and lt0 < math.log(1e290)
            margin = min(margin, abs(pw * span / 0.04 - 1.0), abs(lt0 - math.log(1e290)))
        kinds.append("none" if not prof else "poly" if ok else "exp")
    return kinds, margin


def tiles_of(ntiles):
    su = (UNITS + ntiles - 1) // ntiles
    return [(u, min(u + su, UNITS)) for u in range(0, UNITS, su)]


@pytest.fixture(scope="module")
def cases(orc):
    """Workload, spectrum, chains and the oracle's answers of every grid: computed once, shared, never modified."""
    out = {}
    for name, (x0, step, noise, freqs, width, a1, want) in GRIDS.items():
        x = synth.grid(NX, x0, step)
        modes = [[(nu, width * (1.0 + 0.1 * l + 0.05 * k), 1.2 - 0.15 * l) for k, nu in enumerate(fl)] for l, fl in enumerate(freqs)]
        w = synth._global_workload(2, modes, [1.5, 0.53, 0.2], a1, 55.0, 1e-5, 0.01, 0.0, noise, 20.0, False, x)
        z = int(w["plength"][:8].sum())
        if name == "poly-exp":
            w["relax"][z] = w["relax"][z + 1] = 0
            w["index_to_relax"] = np.flatnonzero(w["relax"]).astype(np.int32)
        rng = np.random.default_rng(41)
        P = np.tile(w["params_true"], (2, 1))
        idx = w["index_to_relax"]
        P[:, idx] *= 1.0 + 0.002 * rng.standard_normal((2, idx.size))
        if name == "poly-exp":
            P[0, z + 1], P[1, z + 1] = TAU_B       # the change of kind of each chain is set by its tau, exactly
        m, st = orc.model(2, w["params_true"], w["plength"], x)
        assert st == 0 and np.all(m > 0)
        y = synth.make_spectrum(m, seed=53)
        rL, rst = orc.generate_batch(2, w["plength"], x, y, P, T)
        g, gabs, gL, gst = orc.grad_analytic(2, w["plength"], x, y, P, T, idx)
        assert np.all(rst == 0) and np.all(gst == 0) and np.array_equal(gL, rL)
        for v in (x, y, P, rL, g, gabs):
            v.setflags(write=False)
        out[name] = dict(w=w, y=y, P=P, rL=rL, g=g, gabs=gabs, want=want)
    return out


def test_tiles_put_odd_units_on_both_sides_of_a_change():
    """The tile bounds the cases rely on (equal-length tiles: tamcmc_setup_body.h, su = ceil(units / tiles))."""
    assert UNITS == 25
    t5, t3 = tiles_of(5), tiles_of(9)
    assert (6, 9) in t3 and (0, 3) in t3 and (9, 12) in t3 and (15, 18) in t3 and (24, 25) in t3
    assert (5, 10) in t5 and (15, 20) in t5


@pytest.mark.parametrize("name", list(GRIDS))
def test_kinds_by_the_setup_criterion(cases, name):
    c = cases[name]
    for k in range(2):
        kinds, margin = cell_kinds(c["w"], c["P"][k])
        assert kinds == c["want"][k], (name, k, kinds)
        assert margin > 5e-3, (name, k, margin)        # no cell sits on the threshold: rounding of log() cannot flip it


def _run(accel_mod, c, P, Tc):
    with accel_mod.Accel(2, c["w"]["plength"], c["w"]["x"], c["y"]) as acc:
        acc.set_vars(c["w"]["index_to_relax"])
        L, st = acc.eval_batch(P, Tc)
        Lg, stg, g = acc.eval_batch(P, Tc, grad=True)
    return L, st, Lg, stg, g


@pytest.mark.parametrize("ntiles", TILES, ids=[f"tiles{t}" for t in TILES])
@pytest.mark.parametrize("name", list(GRIDS))
def test_cell_kinds(accel_mod, cases, monkeypatch, name, ntiles):
    c = cases[name]
    P = c["P"]
    monkeypatch.setenv("TAMCMC_EQUAL_COST", "0")
    monkeypatch.setenv("TAMCMC_TILES", str(ntiles))
    monkeypatch.setenv("TAMCMC_TILES_GRAD", str(ntiles))
    monkeypatch.setenv("TAMCMC_BG_EXACT", "0")
    L, st, Lg, stg, g = _run(accel_mod, c, P, T)
    # against the CPU oracle
    assert np.all(st == 0) and np.all(stg == 0)
    eL = max(float(np.max(np.abs(v - c["rL"]) / np.abs(c["rL"]))) for v in (L, Lg))
    ec, er = gradcheck.assert_grad_entrywise(g, c["g"], c["gabs"], tag=f"{name} tiles {ntiles}")
    # the likelihood launch against the gradient launch
    eP = float(np.max(np.abs(L - Lg) / np.abs(Lg)))
    print(f"\n{name}, {ntiles} tiles: logL {eL:.2e} relative, likelihood vs gradient launch {eP:.2e}, gradient entries "
          f"{ec:.2e} of their sum|terms| ({er:.2e} relative)")
    assert eL <= 1e-10, (name, eL)
    assert np.allclose(L, Lg, rtol=1e-13, atol=0), (name, eP)
    # each chain alone: the same bits
    for k in range(2):
        L1, st1, Lg1, stg1, g1 = _run(accel_mod, c, P[k:k + 1], T[k:k + 1])
        assert L1[0] == L[k] and Lg1[0] == Lg[k] and np.array_equal(g1[0], g[k]), (name, k)
    # every cell on exp() per bin
    monkeypatch.setenv("TAMCMC_BG_EXACT", "1")
    Lx, stx, Lgx, stgx, gx = _run(accel_mod, c, P, T)
    assert np.all(stx == 0) and np.all(stgx == 0)
    scale = np.max(np.abs(gx), axis=1, keepdims=True)
    eX = float(np.max(np.abs(g - gx) / scale))
    print(f"  default vs exp() per bin: logL {float(np.max(np.abs(L - Lx) / np.abs(Lx))):.2e}, gradient {eX:.2e} of the row's largest entry")
    assert np.allclose(L, Lx, rtol=1e-13, atol=0) and np.allclose(Lg, Lgx, rtol=1e-13, atol=0)
    assert eX < 1e-11
    if name == "no-harvey":
        assert np.array_equal(g, gx) and np.array_equal(L, Lx)      # no profile: the switch has nothing to change
    else:
        assert not np.array_equal(g, gx)                              # the two paths really are different code
    gradcheck.assert_grad_entrywise(gx, c["g"], c["gabs"], tag=f"{name} tiles {ntiles}, exact cells")
