"""The cross-wave sums of the gradient kernels (tamcmc_eval_body.h: TM_ROW_K, TM_ROWS, the flush behind pass 2).

Every wave of a gradient workgroup keeps rows of 24 doubles in LDS that only it writes -- the likelihood triple, the noise
sums of the (at most two) cells its tile meets, the butterfly results of up to K = TM_ROW_K = 6 consecutive active
multiplets -- and the workgroup adds the four waves once per chunk of K multiplets.  What can go wrong there is counting
and masking: the chunk bounds (nact = 0, 1, K-1, K, K+1, 2K, 2K+1), a row that is reused by the next chunk, the slots a
shape does not write (stored as zero, never read), the second noise part, and a wave that runs ahead of its neighbours.
The smallest shapes that hold all of it:

  model id 2, 3 chains, trunc_c = 1, a1 = 0.4, widths 0.5: the window of a mode at f is f -+ (l + 1) for l > 0 and
  f -+ 2.2 for l = 0 (tamcmc_derive.h, tm_window), on the grid x = 2000 + i / 128 (cells of 4096 bins are narrow enough
  in log x for the background polynomial).  The table of a global id is radial-order-major, j = n (lmax + 1) + l, and a
  tile's active list keeps table order.

  "pair" grids: 5157 bins = 10 units of 512 and one of 37, two tiles of equal length (TAMCMC_TILES_GRAD = 2): tile A =
      units [0, 6) = x in [2000, 2024), tile B = units [6, 11) = x in [2024, 2040.29), which crosses the cell boundary at
      unit 8 (both noise parts).  lmax = 3, Nmax = 4: 16 multiplets of 1, 3, 5 and 7 components; the set S of table
      indices goes wholly inside tile A, the rest wholly inside tile B, so (nact of A, nact of B) is (|S|, 16 - |S|):
      the prefixes |S| = 0, 1, 4, 5, 6, 7, 12, 13, 16 give A every count asked for and B 16, 15, 12, 11, 10, 9, 4, 3, 0
      -- B with 0 is the crossing tile with background only, A with 4 is all four shapes in one chunk.
      "stale": B = {3, 5, 6, 7, 9, 10, 12} = (l3, l1, l2, l3, l1, l2 | l0): K + 1 entries, the last one an l = 0
      multiplet (slots 0, 7, 11) in the row an l = 3 multiplet (slots 0..6, 7..10, 11) used in the chunk before.
      The prefixes 4 and 16 and "stale" run with Lorentzian asymmetry 25 as well (the four asymmetric shapes: slots
      21..23), "stale" also with every tau = 0 (nh = 0: no Harvey profile) and with TAMCMC_BG_EXACT = 1 (exp per bin in
      both cells), prefix 16 with TAMCMC_BG_EXACT = 1 too (the crossing tile without multiplets on the fallback).
  "one" grids: 1573 bins = 3 units and one of 37: one tile whatever the tile count, run by the fused kernel (setup and
      evaluation in one launch, the generic body) and, with TAMCMC_FUSED = 0, by the eval kernel (the common-case body).
      Every window meets the grid (a window outside it is moved to its edge by the reference's rule), so nact is the
      table's size (lmax + 1) Nmax: 1, 5, 6, 7, 8, 12, 13 from (0,1), (0,5), (2,2), (0,7), (3,2), (3,3), (0,13).  nact = 0
      does not exist on a one-tile grid of a model with modes; the pair grids and the Gaussian model below have it.
  pair grids "tail-in" / "tail-out": prefix 12 with the window of one l = 1 multiplet of tile B running through the
      grid's partial last unit, or ending where that unit begins (pass 2 evaluates that unit behind its pipelined loop).
  generic gradient kernel: "stale" with the chi_square likelihood, and model id 1 (Harvey + Gaussian, no modes:
      nact = 0 in every tile) on the pair grid.

Checked per case: status 0, logL within 1e-10 relative of the CPU oracle and every gradient entry by tests/gradcheck.py
(the bars of tests/test_grad_gpu.py); then bit for bit: each chain alone against the same chain in the batch, a second
evaluation on the same context, and TAMCMC_ORDER = 0, 1, 2 against each other.  The file uses no new API and passes on
the library before the rows existed: it pins values and invariances, not the mechanism."""
import math
import os
import re

import numpy as np
import pytest

import gradcheck
import workloads as W
from tamcmc_amd import synth

UNIT, CELL_UNITS = 512, 8
K = 6                                  # TM_ROW_K (test_constants_match_the_kernel)
X0, STEP, TRUNC = 2000.0, 1.0 / 128.0, 1.0
A1, WIDTH = 0.4, 0.5
NOISE = [0.0, 0.0, 1.0, 11.049588, 49.669854, 4.0, 0.93569041, 1.3516447, 2.0, 0.13392108]
NOISE_NONE = [0.0, 0.0, 1.0, 11.049588, 0.0, 4.0, 0.93569041, 0.0, 2.0, 0.13392108]
T = np.array([1.0, 3.7, 1.9])
NCH = 3
VIS = [1.5, 0.53, 0.2]

NX_PAIR, NX_ONE = 10 * UNIT + 37, 3 * UNIT + 37
TILE_A, TILE_B = (0, 6), (6, 11)
STALE_B = (3, 5, 6, 7, 9, 10, 12)
PREFIXES = (0, 1, K - 2, K - 1, K, K + 1, 2 * K, 2 * K + 1, 16)
ONE_LAYOUTS = {1: (0, 1), K - 1: (0, K - 1), K: (2, 2), K + 1: (0, K + 1), K + 2: (3, 2), 2 * K: (3, 3), 2 * K + 1: (0, 2 * K + 1)}

# name -> (set S of table indices inside tile A, asymmetry, noise block, environment)
PAIR_CASES = {f"prefix{n}": (tuple(range(n)), 0.0, NOISE, {}) for n in PREFIXES}
PAIR_CASES["stale"] = (tuple(j for j in range(16) if j not in STALE_B), 0.0, NOISE, {})
PAIR_CASES["prefix4-asym"] = (tuple(range(4)), 25.0, NOISE, {})
PAIR_CASES["prefix16-asym"] = (tuple(range(16)), 25.0, NOISE, {})
PAIR_CASES["stale-asym"] = (PAIR_CASES["stale"][0], 25.0, NOISE, {})
PAIR_CASES["stale-noharvey"] = (PAIR_CASES["stale"][0], 0.0, NOISE_NONE, {})
PAIR_CASES["stale-exp"] = (PAIR_CASES["stale"][0], 0.0, NOISE, {"TAMCMC_BG_EXACT": "1"})
PAIR_CASES["prefix16-exp"] = (tuple(range(16)), 0.0, NOISE, {"TAMCMC_BG_EXACT": "1"})
# the grid's partial last unit (unit 10: bins 5120 .. 5156) and the window of the l = 1 multiplet j = 13 of tile B:
# "tail-in" f = 2039: [2037, 2041] runs past the end of the grid; "tail-out" f = 2038: [2036, 2040] ends at bin 5120 in
# chain 0, some bins to either side of it in chains 1 and 2
TAIL_F = {"tail-in": 2039.0, "tail-out": 2038.0}
for _n, _f in TAIL_F.items():
    PAIR_CASES[_n] = (tuple(range(12)), 0.0, NOISE, {})


def half_width(l):
    return TRUNC * (l + 1.0) if l else TRUNC * 2.2


def window(Nx, l, f):
    """tm_window for widths and splittings below 1 (tamcmc_derive.h), in the same fp64 operations."""
    pmin, pmax = f - half_width(l), f + half_width(l)
    xlast = X0 + (Nx - 1) * STEP
    assert not (pmax - STEP) < X0 and not (pmin + STEP) >= xlast
    lo, hi = math.floor((pmin - X0) / STEP), math.ceil((pmax - X0) / STEP)
    return int(min(max(lo, 0), Nx)), int(min(max(hi, 0), Nx))


def spread(lo, hi, n):
    return [lo + (hi - lo) * (k + 0.5) / n for k in range(n)]


def pair_frequencies(S):
    """Frequency of every table index j = 4 n + l: S evenly inside tile A, the rest inside tile B, each in table order (so
    the l = 0 frequencies, the nodes of the width interpolation, ascend with n)."""
    inA, inB = sorted(S), sorted(set(range(16)) - set(S))
    f = {}
    for j, v in zip(inA, spread(2004.5, 2019.5, len(inA))):
        f[j] = v
    for j, v in zip(inB, spread(2028.5, 2035.5, len(inB))):
        f[j] = v
    return f


def active(Nx, lmax, P_row, w, tile):
    """Table indices whose window (from the chain's own frequencies) meets the tile."""
    names = w["names"]
    fidx = [i for i, nm in enumerate(names) if nm == "Frequency_l"]
    Nmax = len(fidx) // (lmax + 1)
    out = []
    for j in range((lmax + 1) * Nmax):
        n, l = divmod(j, lmax + 1)
        lo, hi = window(Nx, l, float(P_row[fidx[l * Nmax + n]]))
        if lo < tile[1] * UNIT and hi > tile[0] * UNIT:
            out.append(j)
    return out


def build(orc, Nx, lmax, Nmax, freqs, asym, noise, like=0):
    """Workload, spectrum, chains and the oracle's answers of one case."""
    x = synth.grid(Nx, X0, STEP)
    modes = [[(freqs[n * (lmax + 1) + l], WIDTH, 1.2 - 0.15 * l + 0.1 * n) for n in range(Nmax)] for l in range(lmax + 1)]
    w = synth._global_workload(2, modes, VIS[:lmax], A1, 55.0, 1e-5, 0.01, asym, noise, TRUNC, False, x)
    idx = w["index_to_relax"]
    rng = np.random.default_rng(83)
    P = np.tile(w["params_true"], (NCH, 1))
    # chains 1 and 2: 0.2 % on everything but the frequencies, which move by some bins only (the windows stay in their tile)
    scale = np.array([2e-6 if w["names"][i] == "Frequency_l" else 2e-3 for i in idx])
    P[1:, idx] *= 1.0 + scale * rng.standard_normal((NCH - 1, idx.size))
    m, st = orc.model(2, w["params_true"], w["plength"], x)
    assert st == 0 and np.all(m > 0)
    y = synth.make_spectrum(m, seed=89)
    sig = (0.05 + 0.2 * np.abs(np.sin(np.arange(Nx)))) if like else None
    rL, rst = orc.generate_batch(2, w["plength"], x, y, P, T, sigma_y=sig, likelihood_case=like)
    g, gabs, gL, gst = orc.grad_analytic(2, w["plength"], x, y, P, T, idx, sigma_y=sig, likelihood_case=like)
    assert np.all(rst == 0) and np.all(gst == 0) and np.array_equal(gL, rL)
    for v in (x, y, P, rL, g, gabs):
        v.setflags(write=False)
    return dict(mid=2, w=w, y=y, P=P, rL=rL, g=g, gabs=gabs, sig=sig, like=like, lmax=lmax)


_CACHE = {}


def pair_case(orc, name, like=0):
    key = (name, like)
    if key not in _CACHE:
        S, asym, noise, _ = PAIR_CASES[name]
        f = pair_frequencies(S)
        if name in TAIL_F:
            f[13] = TAIL_F[name]
        _CACHE[key] = build(orc, NX_PAIR, 3, 4, f, asym, noise, like)
    return _CACHE[key]


def one_case(orc, nact):
    key = ("one", nact)
    if key not in _CACHE:
        lmax, Nmax = ONE_LAYOUTS[nact]
        f = spread(2001.0, 2011.0, nact)
        _CACHE[key] = build(orc, NX_ONE, lmax, Nmax, {j: f[j] for j in range(nact)}, 0.0, NOISE)
    return _CACHE[key]


def test_constants_match_the_kernel():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tamcmc-c-_amd", "csrc", "tamcmc_eval_body.h")).read()
    m = re.search(r"#define TM_ROW_K (\d+)", src)
    assert m is None or int(m.group(1)) == K        # (a library from before the rows has no chunks: every count is plain there)
    units = (NX_PAIR + UNIT - 1) // UNIT
    su = (units + 1) // 2
    assert [(u, min(u + su, units)) for u in range(0, units, su)] == [TILE_A, TILE_B]
    assert TILE_B[0] < CELL_UNITS < TILE_B[1] and TILE_A[1] <= CELL_UNITS          # B crosses the cell boundary, A does not
    assert sorted(ONE_LAYOUTS) == [1, K - 1, K, K + 1, K + 2, 2 * K, 2 * K + 1]
    assert all((lm + 1) * nm == n for n, (lm, nm) in ONE_LAYOUTS.items()) and (NX_ONE + UNIT - 1) // UNIT <= 4
    # the stale-row case: entry K of B's list is an l = 0 multiplet, entry 0 -- the same row one chunk earlier -- an l = 3 one
    assert len(STALE_B) == K + 1 and STALE_B[K] % 4 == 0 and STALE_B[0] % 4 == 3
    assert window(NX_PAIR, 1, TAIL_F["tail-in"]) == (37 * 128, NX_PAIR) and window(NX_PAIR, 1, TAIL_F["tail-out"]) == (36 * 128, 10 * UNIT)


@pytest.mark.parametrize("name", list(PAIR_CASES))
def test_active_counts_of_the_pair_grids(orc, name):
    """Every chain of a pair case has the multiplets of S in tile A alone and the others in tile B alone."""
    c = pair_case(orc, name)
    S = list(PAIR_CASES[name][0])
    rest = [j for j in range(16) if j not in S]
    for k in range(NCH):
        assert active(NX_PAIR, 3, c["P"][k], c["w"], TILE_A) == S, (name, k)
        assert active(NX_PAIR, 3, c["P"][k], c["w"], TILE_B) == rest, (name, k)


def _run(accel_mod, c, P, Tc, twice=False):
    with accel_mod.Accel(c["mid"], c["w"]["plength"], c["w"]["x"], c["y"], sigma_y=c["sig"], likelihood_case=c["like"]) as acc:
        acc.set_vars(c["w"]["index_to_relax"])
        r = acc.eval_batch(P, Tc, grad=True)
        if twice:
            r2 = acc.eval_batch(P, Tc, grad=True)
            assert all(np.array_equal(u, v) for u, v in zip(r, r2)), "second evaluation on the same context differs"
    return r


def check(accel_mod, monkeypatch, c, tag, env, orders=(2,)):
    P = c["P"]
    n = P.shape[0]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("TAMCMC_ORDER", str(orders[0]))
    L, st, g = _run(accel_mod, c, P, T[:n], twice=True)
    eL = float(np.max(np.abs(L - c["rL"]) / np.abs(c["rL"])))
    print(f"\n{tag}: logL {eL:.2e} relative")
    assert np.all(st == 0), (tag, st)
    assert eL <= 1e-10, (tag, eL)
    ec, er = gradcheck.assert_grad_entrywise(g, c["g"], c["gabs"], tag=tag)
    print(f"  gradient entries {ec:.2e} of their sum|terms| ({er:.2e} relative)")
    for k in range(n):
        L1, st1, g1 = _run(accel_mod, c, P[k:k + 1], T[k:k + 1])
        assert st1[0] == 0 and L1[0] == L[k] and np.array_equal(g1[0], g[k]), (tag, "chain alone", k)
    for o in orders[1:]:
        monkeypatch.setenv("TAMCMC_ORDER", str(o))
        Lo, sto, go = _run(accel_mod, c, P, T[:n])
        assert np.array_equal(sto, st) and np.array_equal(Lo, L) and np.array_equal(go, g), (tag, "TAMCMC_ORDER", o)


PAIR_ENV = {"TAMCMC_EQUAL_COST": "0", "TAMCMC_TILES_GRAD": "2", "TAMCMC_FUSED": "1", "TAMCMC_BG_EXACT": "0"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PAIR_CASES))
def test_rowsums_two_tiles(accel_mod, orc, monkeypatch, name):
    c = pair_case(orc, name)
    check(accel_mod, monkeypatch, c, f"pair {name}", {**PAIR_ENV, **PAIR_CASES[name][3]}, orders=(2, 0, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("fused", (1, 0), ids=("fused", "unfused"))
@pytest.mark.parametrize("nact", sorted(ONE_LAYOUTS))
def test_rowsums_one_tile(accel_mod, orc, monkeypatch, nact, fused):
    c = one_case(orc, nact)
    for k in range(NCH):
        assert active(NX_ONE, c["lmax"], c["P"][k], c["w"], (0, 4)) == list(range(nact))
    check(accel_mod, monkeypatch, c, f"one tile, nact {nact}" + ("" if fused else ", eval kernel"),
          {**PAIR_ENV, "TAMCMC_FUSED": str(fused)}, orders=(2, 0, 1))


@pytest.mark.gpu
def test_rowsums_generic_kernel_chi_square(accel_mod, orc, monkeypatch):
    """The chi_square likelihood sends the launch to the generic gradient kernel (GEN = true)."""
    c = pair_case(orc, "stale", like=1)
    check(accel_mod, monkeypatch, c, "pair stale, chi_square", PAIR_ENV, orders=(2, 0, 1))


@pytest.mark.gpu
def test_rowsums_generic_kernel_gaussian_model(accel_mod, orc, monkeypatch):
    """Model id 1 (Harvey profiles + a Gaussian, no modes): the generic gradient kernel with nact = 0 in both tiles, the
    second of which crosses the cell boundary."""
    w = W.make_gauss(1, Nx=NX_PAIR)
    m, st = orc.model(1, w["params_true"], w["plength"], w["x"])
    assert st == 0
    y = synth.make_spectrum(m, seed=97)
    P = W.perturbed(w, NCH, scale=0.002, seed=5)
    idx = w["index_to_relax"]
    rL, rst = orc.generate_batch(1, w["plength"], w["x"], y, P, T)
    g, gabs, gL, gst = orc.grad_analytic(1, w["plength"], w["x"], y, P, T, idx)
    assert np.all(rst == 0) and np.all(gst == 0)
    c = dict(mid=1, w=w, y=y, P=P, rL=rL, g=g, gabs=gabs, sig=None, like=0)
    check(accel_mod, monkeypatch, c, "pair grid, id 1", PAIR_ENV, orders=(2, 0, 1))
