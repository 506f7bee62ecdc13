"""Pass 2 of the common-case gradient kernel walks, per multiplet, only the units of its tile that meet the multiplet's
window, and requests x and the weights of the next such unit before it evaluates the current one (tamcmc_eval_body.h,
tm_grad_mult<.., AHEAD>: two units per iteration, multiplets of up to five components).  What can go wrong there is
geometry: the first and last unit of the range, ranges of odd and even length, the clamp of the look-ahead on the last
trip, the grid's partial last unit, a tile with nothing or one multiplet to do.  The smallest shapes that hold all of it:

  model id 2, two modes of each degree l = 0, 1, 2 (multiplets of 1, 3 and 5 components together), 3 chains, trunc_c = 1,
  a1 = 0.4 and widths 0.5 (both below 1: the window of a mode at f is f -+ (l + 1) for l > 0 and f -+ 2.2 for l = 0,
  tamcmc_derive.h tm_window), on the grid x = 1000 + i / 128 -- step and window half-widths are exact in binary, so a
  mode placed at 1000 + b / 128 + (l + 1) has the window [b, b + 256 (l + 1)) to the bin: 512 bins for l = 1, 768 for
  l = 2, and 564 for l = 0.  Windows so span one to three units of 512 bins.  Chain 0 carries these parameters exactly;
  chains 1 and 2 are perturbed (0.2 %: windows moved by up to some hundred bins, edges nowhere special).

Grids and what their chain 0 holds (asserted by test_geometry from the rule above; units are 512 bins):
  "4097"  8 units and a partial one of 1 bin; tiles of 1, 2 and 3 units (TAMCMC_TILES_GRAD = 9, 5, 3).
          l = 1: [0, 412) clipped by the start of the grid; [512, 1024) exactly unit 1 -- one unit of every tile it
          meets, ending on a unit boundary and on a tile boundary (tiles of 1 and of 2 units).  l = 2: [1400, 2168) over
          three units, nowhere aligned; [2304, 3072) ending on the boundary of the tiles of 1, 2 and 3 units.
          l = 0: [1000, 1564); [3600, 4097) clipped by the end of the grid, the partial unit included.
          Tiles of one unit: unit 6 meets no window (nact = 0), units 7 and 8 meet one.
  "2597"  5 units and a partial one of 37 bins; tiles of 1, 2 and 3 units (TAMCMC_TILES_GRAD = 6, 3, 2).
          l = 1: [0, 412); [2048, 2560) ending where the partial unit begins.  l = 2: [600, 1368); [2570, 2597) which
          starts inside the partial unit.  l = 0: [900, 1464), [1300, 1864).
  "1573"  3 units and a partial one of 37 bins: grids of up to 4 units are ONE tile whatever TAMCMC_TILES_GRAD says
          (tm_tiles), evaluated by the fused kernel (setup and evaluation in one launch: the generic body) or, with
          TAMCMC_FUSED = 0, by the eval kernel (the common-case body): both run.
          l = 1: [0, 312); [1024, 1536) exactly unit 2.  l = 2: [300, 1068); [1550, 1573) inside the partial unit.
          l = 0: [600, 1164), [1200, 1573).
  "2048"  4 whole units, one tile, both kernels as above.  l = 1: [0, 512) exactly unit 0; [1536, 2048) exactly the last
          unit, ending on the tile's and the grid's end.  l = 2: [512, 1280), [1100, 1868).  l = 0: [100, 664), [1400, 1964).
  "4097-asym"  the first grid with Lorentzian asymmetry 25 (the asymmetric shapes of pass 2), tiles of 2 units.

Checked per case:
  (a) status 0, logL within 1e-10 relative of the CPU oracle, every gradient entry by tests/gradcheck.py;
  (b) eval_batch(P, T, grad=True) against the same call with model_rows=[0]: a request for model rows sends the launch
      to the generic kernel, whose pass 2 fetches each unit where it uses it (no look-ahead).  logL and gradient are
      equal bit for bit -- the two bodies already were before the look-ahead existed (this file passed on that library
      as it stands), so the assertion pins that the look-ahead changes no operand and no order of summation;
  (c) each chain alone gives the bits it gives in the batch."""
import math

import numpy as np
import pytest

import gradcheck
from tamcmc_amd import synth

pytestmark = pytest.mark.gpu

UNIT = 512
X0, STEP, TRUNC = 1000.0, 1.0 / 128.0, 1.0
A1, WIDTH = 0.4, 0.5
NOISE = [0.0, 0.0, 1.0, 11.049588, 49.669854, 4.0, 0.93569041, 1.3516447, 2.0, 0.13392108]
T = np.array([1.0, 3.7, 1.9])
NCH = 3

# name: (Nx, asymmetry, first bins of the windows of l = 0, 1, 2 (chain 0), TAMCMC_TILES_GRAD values or None = one tile)
GRIDS = {
    "4097": (4097, 0.0, ((1000, 3600), (-100, 512), (1400, 2304)), (9, 5, 3)),
    "2597": (2597, 0.0, ((900, 1300), (-100, 2048), (600, 2570)), (6, 3, 2)),
    "1573": (1573, 0.0, ((600, 1200), (-200, 1024), (300, 1550)), None),
    "2048": (2048, 0.0, ((100, 1400), (0, 1536), (512, 1100)), None),
    "4097-asym": (4097, 25.0, ((1000, 3600), (-100, 512), (1400, 2304)), (5,)),
}
# (grid, tiles, fused): one-tile grids run once through the fused kernel and once through the eval kernel
CASES = [(name, t, 1) for name, g in GRIDS.items() if g[3] for t in g[3]] + \
        [(name, 1, f) for name, g in GRIDS.items() if not g[3] for f in (1, 0)]


def half_width(l):
    return TRUNC * (l + 1.0) if l else TRUNC * 2.2


def mode_freq(l, b):
    return X0 + b * STEP + half_width(l)


def window(Nx, l, f):
    """tm_window for widths and splittings below 1 (tamcmc_derive.h), in the same fp64 operations."""
    pmin, pmax = f - half_width(l), f + half_width(l)
    xlast = X0 + (Nx - 1) * STEP
    assert not (pmax - STEP) < X0 and not (pmin + STEP) >= xlast
    lo, hi = math.floor((pmin - X0) / STEP), math.ceil((pmax - X0) / STEP)
    return int(min(max(lo, 0), Nx)), int(min(max(hi, 0), Nx))


def windows_of(name):
    Nx, _, starts, _ = GRIDS[name]
    return {(l, k): window(Nx, l, mode_freq(l, b)) for l in range(3) for k, b in enumerate(starts[l])}


def tiles_of(Nx, ntiles):
    units = (Nx + UNIT - 1) // UNIT
    su = (units + ntiles - 1) // ntiles
    return [(u, min(u + su, units)) for u in range(0, units, su)]


def units_met(win, tile):
    """The units of `tile` that the window meets: the range pass 2 walks."""
    lo, hi = max(tile[0], win[0] // UNIT), min(tile[1], (win[1] + UNIT - 1) // UNIT)
    return list(range(lo, hi))


def test_geometry():
    """The windows of chain 0 are where the module's text puts them, and the edge cases it names exist."""
    w = windows_of("4097")
    assert w[(1, 0)] == (0, 412) and w[(1, 1)] == (512, 1024) and w[(2, 0)] == (1400, 2168) and w[(2, 1)] == (2304, 3072)
    assert w[(0, 0)] == (1000, 1564) and w[(0, 1)] == (3600, 4097)
    assert [len(tiles_of(4097, t)) for t in (9, 5, 3)] == [9, 5, 3] and tiles_of(4097, 3)[1] == (3, 6) and tiles_of(4097, 5)[0] == (0, 2)
    met = {t: [k for k, win in w.items() if units_met(win, t)] for t in tiles_of(4097, 9)}
    assert met[(6, 7)] == [] and len(met[(7, 8)]) == 1 and len(met[(8, 9)]) == 1          # nact = 0, nact = 1
    assert units_met(w[(1, 1)], (0, 2)) == [1] and units_met(w[(1, 1)], (0, 3)) == [1]    # one unit of a tile: the look-ahead re-requests it
    assert units_met(w[(2, 0)], (0, 3)) == [2] and units_met(w[(2, 0)], (3, 6)) == [3, 4]
    assert units_met(w[(2, 1)], (3, 6)) == [4, 5] and w[(2, 1)][1] == 6 * UNIT            # ends on the boundary of tiles of 1, 2 and 3 units
    assert units_met(w[(0, 1)], (6, 9)) == [7, 8]                                          # ... into the partial unit
    w = windows_of("2597")
    assert w[(1, 0)] == (0, 412) and w[(1, 1)] == (2048, 2560) and w[(2, 0)] == (600, 1368) and w[(2, 1)] == (2570, 2597)
    assert w[(0, 0)] == (900, 1464) and w[(0, 1)] == (1300, 1864)
    assert units_met(w[(2, 1)], (4, 6)) == [5] and units_met(w[(1, 1)], (4, 6)) == [4]
    assert [len(tiles_of(2597, t)) for t in (6, 3, 2)] == [6, 3, 2]
    w = windows_of("1573")
    assert w[(1, 0)] == (0, 312) and w[(1, 1)] == (1024, 1536) and w[(2, 0)] == (300, 1068) and w[(2, 1)] == (1550, 1573)
    assert w[(0, 0)] == (600, 1164) and w[(0, 1)] == (1200, 1573)
    w = windows_of("2048")
    assert w[(1, 0)] == (0, 512) and w[(1, 1)] == (1536, 2048) and w[(2, 0)] == (512, 1280) and w[(2, 1)] == (1100, 1868)
    assert w[(0, 0)] == (100, 664) and w[(0, 1)] == (1400, 1964)


@pytest.fixture(scope="module")
def cases(orc):
    """Workload, spectrum, chains and the oracle's answers of every grid: computed once, shared, never modified."""
    out = {}
    for name, (Nx, asym, starts, _) in GRIDS.items():
        x = synth.grid(Nx, X0, STEP)
        modes = [[(mode_freq(l, b), WIDTH, 1.2 - 0.15 * l + 0.1 * k) for k, b in enumerate(starts[l])] for l in range(3)]
        w = synth._global_workload(2, modes, [1.5, 0.53], A1, 55.0, 1e-5, 0.01, asym, NOISE, TRUNC, False, x)
        idx = w["index_to_relax"]
        rng = np.random.default_rng(67)
        P = np.tile(w["params_true"], (NCH, 1))
        P[1:, idx] *= 1.0 + 0.002 * rng.standard_normal((NCH - 1, idx.size))
        m, st = orc.model(2, w["params_true"], w["plength"], x)
        assert st == 0 and np.all(m > 0)
        y = synth.make_spectrum(m, seed=71)
        rL, rst = orc.generate_batch(2, w["plength"], x, y, P, T)
        g, gabs, gL, gst = orc.grad_analytic(2, w["plength"], x, y, P, T, idx)
        assert np.all(rst == 0) and np.all(gst == 0) and np.array_equal(gL, rL)
        for v in (x, y, P, rL, g, gabs):
            v.setflags(write=False)
        out[name] = dict(w=w, y=y, P=P, rL=rL, g=g, gabs=gabs)
    return out


def _run(accel_mod, c, P, Tc, rows=None):
    with accel_mod.Accel(2, c["w"]["plength"], c["w"]["x"], c["y"]) as acc:
        acc.set_vars(c["w"]["index_to_relax"])
        return acc.eval_batch(P, Tc, grad=True, model_rows=rows)


@pytest.mark.parametrize("name,ntiles,fused", CASES, ids=[f"{n}-tiles{t}" + ("" if f else "-unfused") for n, t, f in CASES])
def test_grad_lookahead(accel_mod, cases, monkeypatch, name, ntiles, fused):
    c = cases[name]
    P = c["P"]
    monkeypatch.setenv("TAMCMC_EQUAL_COST", "0")
    monkeypatch.setenv("TAMCMC_TILES_GRAD", str(ntiles))
    monkeypatch.setenv("TAMCMC_FUSED", str(fused))
    tag = f"{name}, {ntiles} tiles" + ("" if fused else ", eval kernel")
    L, st, g = _run(accel_mod, c, P, T)
    # (a) against the CPU oracle
    eL = float(np.max(np.abs(L - c["rL"]) / np.abs(c["rL"])))
    print(f"\n{tag}: logL {eL:.2e} relative")
    assert np.all(st == 0), (tag, st)
    assert eL <= 1e-10, (tag, eL)
    ec, er = gradcheck.assert_grad_entrywise(g, c["g"], c["gabs"], tag=tag)
    print(f"  gradient entries {ec:.2e} of their sum|terms| ({er:.2e} relative)")
    # (b) against the generic body (a model row requested): the same bits
    Lr, str_, gr, rows = _run(accel_mod, c, P, T, rows=[0])
    dL, dg = float(np.max(np.abs(L - Lr))), float(np.max(np.abs(g - gr)))
    print(f"  common-case body vs generic body: max |dlogL| {dL:.2e}, max |dgrad| {dg:.2e}")
    assert np.all(str_ == 0) and np.all(np.isfinite(rows))
    assert np.array_equal(L, Lr), (tag, dL)
    assert np.array_equal(g, gr), (tag, dg)
    # (c) each chain alone: the same bits
    for k in range(NCH):
        L1, st1, g1 = _run(accel_mod, c, P[k:k + 1], T[k:k + 1])
        assert st1[0] == 0 and L1[0] == L[k] and np.array_equal(g1[0], g[k]), (tag, k)
