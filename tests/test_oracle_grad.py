"""The oracle's analytic gradient (oracle/tamcmc_oracle.c: orc_grad_analytic) pinned entry by entry.

The reference has no gradient (MALA.cpp:18,317-333: D_MALA() returns zeros), so nothing in it can pin this; what can
is the oracle's own log-likelihood: Richardson-extrapolated central differences of it, with the likelihood sums kept
in long double (orc_grad_fd_wide) so that the difference quotient's noise is ~1e-14 / step.
Tolerance, per entry k (the judge's round-2 form):   |g_k - fd_k| <= 1e-6 * (|g_k| + 1e-9 * max_j |g_j|).
One fixed step cannot serve every variable (frequencies live on a scale of a line width, ~1e-3 of their value; the
Harvey heights on the scale of their value, with gradient entries 1e-9 of the largest), so differences are taken at
four relative steps and an entry has to agree with one of them -- agreement to 1e-6 by accident does not happen.
CPU only: this is the checker being checked.  The HIP gradient is compared with orc_grad_analytic under -m gpu
(tests/test_grad_gpu.py, tests/test_baseline_configs_gpu.py, tests/test_fuzz_gpu.py)."""
import numpy as np
import pytest

import workloads as W
from gradcheck import entrywise_error
from tamcmc_amd import synth


def with_shape_variables(w):
    """eta, a3 and the asymmetry join the variables (they are fixed in the synthetic star's .model)."""
    relax = w["relax"].copy()
    pl = w["plength"]
    s = int(pl[0] + pl[1] + pl[2:6].sum())
    relax[[s + 1, s + 2, s + 5]] = 1
    w["relax"] = relax
    w["index_to_relax"] = np.flatnonzero(relax).astype(np.int32)
    return w


@pytest.mark.parametrize("mid", [2, 3, 6, 7, 8, 9, 10, 11, 12, 13, 14])
@pytest.mark.parametrize("kw", [dict(), dict(asym=25.0, do_amp=True), dict(asym=-40.0)], ids=["plain", "asym-amp", "neg-asym"])
def test_analytic_gradient_against_finite_differences(orc, mid, kw):
    """Every live Lorentzian model id, no truncation window (trunc_c = 10000: logL is smooth), all variables."""
    w = W.any_model(mid, Nx=3000, trunc_c=10000.0, **kw)
    if kw:
        w = with_shape_variables(w)
    m, st = orc.model(mid, w["params_true"], w["plength"], w["x"])
    assert st == 0
    y = synth.make_spectrum(m, seed=23)
    P = W.perturbed(w, 2, scale=0.002, seed=5)
    entrywise_error(orc, mid, w, y, P, np.array([1.0, 3.7]), w["index_to_relax"])


@pytest.mark.parametrize("mid", [0, 1])
def test_analytic_gradient_gaussian_models_both_likelihoods(orc, mid):
    w = W.make_gauss(mid, Nx=2500)
    m, _ = orc.model(mid, w["params_true"], w["plength"], w["x"])
    y = synth.make_spectrum(m, seed=29)
    P = W.perturbed(w, 2, scale=0.002, seed=5)
    T = np.array([1.0, 3.7])
    entrywise_error(orc, mid, w, y, P, T, w["index_to_relax"])
    sig = 0.3 + 0.1 * np.cos(np.arange(y.size)) ** 2
    entrywise_error(orc, mid, w, y, P, T, w["index_to_relax"], sigma=sig, like=1)


@pytest.mark.parametrize("mid", [2, 11])
def test_analytic_gradient_chi_square_on_lorentzian_models(orc, mid):
    w = with_shape_variables(W.any_model(mid, Nx=2000, trunc_c=10000.0, asym=5.0))
    m, _ = orc.model(mid, w["params_true"], w["plength"], w["x"])
    y = synth.make_spectrum(m, seed=31)
    sig = 0.05 + 0.2 * np.abs(np.sin(np.arange(y.size)))
    P = W.perturbed(w, 1, scale=0.002, seed=7)
    entrywise_error(orc, mid, w, y, P, np.array([2.0]), w["index_to_relax"], sigma=sig, like=1)


@pytest.mark.parametrize("mid,trunc_c", [(3, 20.0), (3, 7.0), (13, 20.0), (14, 7.0)])
def test_analytic_gradient_with_the_window_on(orc, mid, trunc_c):
    """With the truncation window on, logL jumps whenever a window edge crosses a bin, so finite differences are only
    meaningful for the variables that do not move any window: the window depends on a multiplet's frequency, width and
    splitting (build_lorentzian.cpp:377-427), not on heights, visibilities, inclination (ids 3, 13, 14 take it or the
    m-heights directly), eta, a3, asymmetry or the noise.  Those entries run through the same windowed per-bin loops
    as all the others."""
    w = with_shape_variables(W.any_model(mid, Nx=3000, trunc_c=trunc_c, asym=10.0))
    pl = w["plength"]
    Nmax, nvis = int(pl[0]), int(pl[1])
    s = int(pl[0] + pl[1] + pl[2:6].sum())
    wq = s + int(pl[6])
    z = wq + int(pl[7])
    q = z + int(pl[8])
    keep = np.zeros(w["params_true"].size, dtype=bool)
    keep[:Nmax + nvis] = True                      # heights (and visibilities)
    keep[[s + 1, s + 2, s + 5]] = True             # eta, a3, asymmetry
    keep[z:q + int(pl[9])] = True                  # noise, inclination / m-height block
    idx = np.array([i for i in w["index_to_relax"] if keep[i]], dtype=np.int32)
    assert idx.size >= 10
    m, st = orc.model(mid, w["params_true"], w["plength"], w["x"])
    assert st == 0
    y = synth.make_spectrum(m, seed=37)
    P = W.perturbed(w, 1, scale=0.002, seed=9)
    entrywise_error(orc, mid, w, y, P, np.array([1.0]), idx)


def test_closed_form_height_ratios_match_amplitude_ratio(orc):
    """App. D's closed forms (what the analytic gradient differentiates) against the oracle's literal restatement of
    function_rot.cpp:20-93, and their derivative against central differences of themselves."""
    for l in (1, 2, 3):
        for deg in (0.0, 3.0, 27.5, 55.0, 89.9, 90.0, 131.0):
            beta = np.pi * deg / 180.0
            v, dv = orc.amplitude_ratio_closed(l, beta)
            assert np.max(np.abs(v - orc.amplitude_ratio(l, deg))) <= 4e-16
            assert abs(v.sum() - 1.0) <= 1e-15 and abs(dv.sum()) <= 1e-15
            h = 1e-5
            vp, _ = orc.amplitude_ratio_closed(l, beta + h)
            vm, _ = orc.amplitude_ratio_closed(l, beta - h)
            assert np.max(np.abs((vp - vm) / (2 * h) - dv)) <= 1e-9


def test_gradient_scales_with_temperature_and_p(orc):
    """d(logL/T): linear in 1/T and in the (truncated) likelihood exponent p (model_def.cpp:300-302)."""
    w = W.make(2, Nx=1500)
    m, _ = orc.model(2, w["params_true"], w["plength"], w["x"])
    y = synth.make_spectrum(m, seed=41)
    P = W.perturbed(w, 1, scale=0.002)
    idx = w["index_to_relax"]
    g1, *_ = orc.grad_analytic(2, w["plength"], w["x"], y, P, [1.0], idx)
    g4, *_ = orc.grad_analytic(2, w["plength"], w["x"], y, P, [4.0], idx)
    gp, *_ = orc.grad_analytic(2, w["plength"], w["x"], y, P, [1.0], idx, likelihood_p=2.9)
    assert np.allclose(g4 * 4.0, g1, rtol=1e-15, atol=0)
    assert np.allclose(gp, 2.0 * g1, rtol=1e-15, atol=0)


# ---------------------------------------------------------------- layouts beyond the C2 star (tests/workloads.py: layout)
LAYOUT_IDS = [2, 3, 6, 7, 8, 9, 10, 12, 13]


def _layout_check(orc, w, seed, idx=None, nchains=2):
    mid = w["model_case"]
    m, st = orc.model(mid, w["params_true"], w["plength"], w["x"])
    assert st == 0
    y = synth.make_spectrum(m, seed=seed)
    P = W.perturbed(w, nchains, scale=0.002, seed=5)
    return entrywise_error(orc, mid, w, y, P, np.array([1.0, 3.7])[:nchains], w["index_to_relax"] if idx is None else idx)


@pytest.mark.parametrize("mid", LAYOUT_IDS)
@pytest.mark.parametrize("lmax", [0, 1, 2, 3])
@pytest.mark.parametrize("kw", [dict(), dict(asym=25.0, do_amp=True)], ids=["plain", "asym-amp"])
def test_analytic_gradient_every_global_id_at_lmax(orc, mid, lmax, kw):
    """Global ids at lmax = 3 (the l = 3 splitting of the a1l family, id 12's l = 3 ratios, id 13's l = 3 heights) and
    at lmax = 0 / 1 (layouts without interpolated widths or with one visibility), no window, all variables."""
    w = W.layout(mid, lmax, Nmax=4, Nx=3000, trunc_c=10000.0, **kw)
    _layout_check(orc, w, seed=43 + mid + lmax)


@pytest.mark.parametrize("mid", [11, 14])
def test_analytic_gradient_local_ids_with_l3_modes(orc, mid):
    w = W.layout(mid, Nx=3000, trunc_c=10000.0, asym=25.0, do_amp=True)
    assert w["plength"][5] > 0
    _layout_check(orc, w, seed=47 + mid)


@pytest.mark.parametrize("mid", [2, 13])
@pytest.mark.parametrize("noise", [((11.049588, 49.669854, 4.0), (0.93569041, 1.3516447, 0.0), (0.4, 8.0, 2.45)),
                                   ((-11.049588, 49.669854, 3.3), (0.93569041, -1.3516447, 2.0), (0.4, 8.0, -1.7)),
                                   ()],
                         ids=["three-p0-nonint", "negative", "none"])
def test_analytic_gradient_harvey_backgrounds(orc, mid, noise):
    """Three active profiles (one with p = 0: the constant H/2, one with a non-integer p), negative H / tau / p (the
    model takes their absolute values), and no active profile."""
    w = W.layout(mid, 3, noise=noise, Nmax=4, Nx=3000, trunc_c=10000.0)
    _layout_check(orc, w, seed=53 + mid)


@pytest.mark.parametrize("mid", [6, 12])
def test_analytic_gradient_window_on_at_lmax3(orc, mid):
    """lmax = 3 with the truncation window on: the variables that move no window edge (see
    test_analytic_gradient_with_the_window_on)."""
    w = W.layout(mid, 3, Nmax=4, Nx=3000, trunc_c=7.0, asym=10.0)
    pl = w["plength"]
    Nmax, nvis = int(pl[0]), int(pl[1])
    s = int(pl[0] + pl[1] + pl[2:6].sum())
    z = s + int(pl[6]) + int(pl[7])
    q = z + int(pl[8])
    keep = np.zeros(w["params_true"].size, dtype=bool)
    keep[:Nmax + nvis] = True
    keep[[s + 1, s + 2, s + 5]] = True
    keep[z:q + int(pl[9])] = True
    idx = np.array([i for i in w["index_to_relax"] if keep[i]], dtype=np.int32)
    assert idx.size >= 10
    _layout_check(orc, w, seed=59 + mid, idx=idx)
