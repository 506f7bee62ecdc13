"""Specialisation matrix: every global model id at lmax = 0..3 and the local ids with l = 3 modes, each symmetric,
asymmetric in the amplitude form and asymmetric with a narrow window (trunc_c = 7), on a one-tile grid (fused launch)
and on a tiled grid under both tile cuts (TAMCMC_EQUAL_COST = 0 / 1); and Harvey backgrounds beyond the synthetic
star's on id 2 and id 13 at lmax = 3.  Case list and what each case reaches: tests/layouts.py (its coverage is checked
on the CPU by tests/test_layout_matrix.py).

Per case, against the CPU oracle, with the suite's bars: status identical; logL of the likelihood launch (specialised
and generic kernels) and of the gradient launch within 1e-10 relative of the oracle and within 1e-12 of each other;
one model row within 1e-12 per bin; every gradient entry through tests/gradcheck.py."""
import numpy as np
import pytest

import gradcheck
import layouts as LY
import workloads as W
from tamcmc_amd import synth

pytestmark = pytest.mark.gpu

RTOL_LOGL = 1e-10
RTOL_PATHS = 1e-12
RTOL_MODEL = 1e-12
T = np.array([1.0, 2.3, 7.1])

_WORST = dict(logL=0.0, paths=0.0, model=0.0, grad_cond=0.0, grad_rel=0.0, cases=0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\nlayout matrix: {_WORST['cases']} device runs; worst logL {_WORST['logL']:.2e} relative, likelihood vs "
          f"gradient launch {_WORST['paths']:.2e}, model {_WORST['model']:.2e}; gradient worst entry "
          f"{_WORST['grad_cond']:.2e} of its sum|terms|, {_WORST['grad_rel']:.2e} relative")


def _inputs(orc, w, seed):
    mid = w["model_case"]
    m, st = orc.model(mid, w["params_true"], w["plength"], w["x"])
    assert st == 0 and np.all(m > 0)
    y = synth.make_spectrum(m, seed=seed)
    P = W.perturbed(w, LY.NCHAINS, scale=0.003, seed=5)
    rL, rst, rm = orc.generate_batch(mid, w["plength"], w["x"], y, P, T, want_models=True)
    g, gabs, gL, gst = orc.grad_analytic(mid, w["plength"], w["x"], y, P, T, w["index_to_relax"])
    assert np.all(rst == 0) and np.all(gst == 0) and np.array_equal(gL, rL)
    return y, P, (rL, rst, rm, g, gabs)


def _device(accel_mod, w, y, P, row):
    with accel_mod.Accel(w["model_case"], w["plength"], w["x"], y) as acc:      # the library accepts the layout
        acc.set_vars(w["index_to_relax"])
        L, st = acc.eval_batch(P, T)                                            # specialised likelihood kernel
        L2, st2, models = acc.eval_batch(P, T, model_rows=[row])                # generic kernel, model row written
        Lg, stg, g = acc.eval_batch(P, T, grad=True)
    return L, st, L2, st2, models, Lg, stg, g


def _check(tag, out, ref, row):
    L, st, L2, st2, models, Lg, stg, g = out
    rL, rst, rm, rg, rgabs = ref
    assert np.array_equal(st, rst) and np.array_equal(st2, rst) and np.array_equal(stg, rst), (tag, st, st2, stg, rst)
    eL = max(float(np.max(np.abs(v - rL) / np.abs(rL))) for v in (L, L2, Lg))
    eP = max(float(np.max(np.abs(v - L) / np.abs(L))) for v in (L2, Lg))
    eM = float(np.max(np.abs(models[0] - rm[row]) / np.abs(rm[row])))
    assert eL <= RTOL_LOGL, (tag, "logL", eL)
    assert eP <= RTOL_PATHS, (tag, "likelihood vs gradient launch", eP)
    assert eM <= RTOL_MODEL, (tag, "model row", eM)
    ec, er = gradcheck.assert_grad_entrywise(g, rg, rgabs, tag=tag)
    _WORST["logL"] = max(_WORST["logL"], eL)
    _WORST["paths"] = max(_WORST["paths"], eP)
    _WORST["model"] = max(_WORST["model"], eM)
    _WORST["grad_cond"] = max(_WORST["grad_cond"], ec)
    _WORST["grad_rel"] = max(_WORST["grad_rel"], er)
    _WORST["cases"] += 1


@pytest.mark.parametrize("mid,lmax", LY.LAYOUTS, ids=[f"id{m}-l{l}" for (m, l) in LY.LAYOUTS])
@pytest.mark.parametrize("variant", list(LY.VARIANTS))
def test_layout_matrix(accel_mod, orc, monkeypatch, mid, lmax, variant):
    for k, grid in enumerate(LY.GRIDS):
        w = LY.matrix_case(mid, lmax, variant, grid)
        y, P, ref = _inputs(orc, w, seed=101 + 7 * mid + lmax + 13 * k)
        row = (mid + lmax) % LY.NCHAINS
        for ec in ((None,) if grid == "fused" else ("0", "1")):
            if ec is not None:
                monkeypatch.setenv("TAMCMC_EQUAL_COST", ec)
            _check(f"id {mid} lmax {lmax} {variant} {grid} equal_cost={ec}", _device(accel_mod, w, y, P, row), ref, row)


@pytest.mark.parametrize("mid", LY.BACKGROUND_IDS)
@pytest.mark.parametrize("bg", list(LY.BACKGROUNDS))
def test_harvey_backgrounds(accel_mod, orc, monkeypatch, mid, bg):
    w = LY.background_case(mid, bg)
    y, P, ref = _inputs(orc, w, seed=211 + mid)
    for ec in ("0", "1"):
        monkeypatch.setenv("TAMCMC_EQUAL_COST", ec)
        _check(f"id {mid} background {bg} equal_cost={ec}", _device(accel_mod, w, y, P, 1), ref, 1)
    if bg != "mixed":
        return
    # one chain, both kinds of cells (and a tile meeting one of each): the same batch on exp()-per-bin cells only
    for p in P:
        npoly, cells = W.poly_cells(w, p)
        assert 0 < npoly < cells
    monkeypatch.setenv("TAMCMC_EQUAL_COST", "0")
    out = []
    for exact in ("0", "1"):
        monkeypatch.setenv("TAMCMC_BG_EXACT", exact)
        with accel_mod.Accel(mid, w["plength"], w["x"], y) as acc:
            acc.set_vars(w["index_to_relax"])
            out.append(acc.eval_batch(P, T, grad=True))
    (L0, s0, g0), (L1, s1, g1) = out
    assert np.all(s0 == 0) and np.all(s1 == 0)
    assert np.allclose(L0, L1, rtol=1e-13, atol=0)
    scale = np.max(np.abs(g1), axis=1, keepdims=True)
    assert np.max(np.abs(g0 - g1) / scale) < 1e-11
    assert not np.array_equal(g0, g1)      # the two paths really are different code
    gradcheck.assert_grad_entrywise(g1, ref[3], ref[4], tag=f"id {mid} mixed background, exact cells")
