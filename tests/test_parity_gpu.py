"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle on the same
seeded inputs.  Tolerances (written here once):
    log-likelihood  : |dL| <= 1e-10 * |L|          (north-star: "log-L within 1e-10 relative")
    model spectrum  : max |dM|/M <= 1e-12 per bin
    status codes    : identical
    gradient        : every entry against the oracle's analytic gradient, with the per-entry bar of
                      tests/gradcheck.py (the reference has no gradient)
"""
import numpy as np
import pytest

import gradcheck
import workloads as W
from tamcmc_amd import synth

pytestmark = pytest.mark.gpu

RTOL_LOGL = 1e-10
RTOL_MODEL = 1e-12


def spectrum_for(orc, w, seed=17):
    m, st = orc.model(w["model_case"], w["params_true"], w["plength"], w["x"])
    assert st == 0
    return synth.make_spectrum(m, seed=seed)


def check_logL(a, b):
    assert np.all(np.isfinite(b))
    assert np.max(np.abs(a - b) / np.abs(b)) <= RTOL_LOGL, (a, b)


@pytest.mark.parametrize("mid", W.ALL_IDS)
@pytest.mark.parametrize("kw", [dict(), dict(asym=25.0), dict(do_amp=True, trunc_c=10000.0), dict(asym=-40.0, do_amp=True, trunc_c=7.0)],
                         ids=["plain", "asym", "amp-notrunc", "asym-amp-c7"])
def test_model_and_logL_every_id(accel_mod, orc, mid, kw):
    w = W.any_model(mid, Nx=5000, **kw)       # 5000 bins: not a multiple of any tile size
    y = spectrum_for(orc, w)
    n = 6
    P = W.perturbed(w, n, scale=0.004)
    T = synth.temperatures(n)
    with accel_mod.Accel(mid, w["plength"], w["x"], y) as acc:
        logL, st, models = acc.eval_batch(P, T, model_rows=list(range(n)))
    rL, rst, rmodels = orc.generate_batch(mid, w["plength"], w["x"], y, P, T, want_models=True)
    assert np.array_equal(st, rst) and np.all(st == 0)
    assert np.max(np.abs(models - rmodels) / rmodels) <= RTOL_MODEL
    check_logL(logL, rL)


@pytest.mark.parametrize("mid", [0, 1, 2, 11])
def test_chi_square_likelihood(accel_mod, orc, mid):
    w = W.any_model(mid, Nx=3000)
    y = spectrum_for(orc, w)
    sig = 0.05 + 0.2 * np.abs(np.sin(np.arange(y.size)))
    P = W.perturbed(w, 4, scale=0.003)
    T = synth.temperatures(4)
    with accel_mod.Accel(mid, w["plength"], w["x"], y, sigma_y=sig, likelihood_case=1) as acc:
        logL, st = acc.eval_batch(P, T)
    rL, rst = orc.generate_batch(mid, w["plength"], w["x"], y, P, T, sigma_y=sig, likelihood_case=1)
    assert np.array_equal(st, rst)
    check_logL(logL, rL)


def test_likelihood_p_is_truncated_like_the_reference(accel_mod, orc):
    w = W.make(2, Nx=2000)
    y = spectrum_for(orc, w)
    P = W.perturbed(w, 2)
    T = np.ones(2)
    with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=2.9) as acc:
        logL, _ = acc.eval_batch(P, T)
    rL, _ = orc.generate_batch(2, w["plength"], w["x"], y, P, T, likelihood_p=2.9)
    check_logL(logL, rL)
    with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=1.0) as acc:
        logL1, _ = acc.eval_batch(P, T)
    assert np.allclose(logL, 2.0 * logL1, rtol=1e-14)


@pytest.mark.parametrize("Nx", [2, 3, 255, 256, 257, 1023, 1024, 1025, 4099])
def test_ragged_sizes(accel_mod, orc, Nx):
    w = W.make_gauss(1, Nx=Nx)
    y = spectrum_for(orc, w)
    P = W.perturbed(w, 3, scale=0.01)
    T = synth.temperatures(3)
    with accel_mod.Accel(1, w["plength"], w["x"], y) as acc:
        logL, st, models = acc.eval_batch(P, T, model_rows=[2, 0])
    rL, rst, rm = orc.generate_batch(1, w["plength"], w["x"], y, P, T, want_models=True)
    check_logL(logL, rL)
    assert np.max(np.abs(models[0] - rm[2]) / rm[2]) <= RTOL_MODEL
    assert np.max(np.abs(models[1] - rm[0]) / rm[0]) <= RTOL_MODEL


@pytest.mark.parametrize("Nx", [300, 1500, 4097])
def test_ragged_sizes_lorentzian(accel_mod, orc, Nx):
    w = W.make(2, Nx=Nx)
    y = spectrum_for(orc, w)
    P = W.perturbed(w, 3, scale=0.003)
    T = synth.temperatures(3)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        logL, st = acc.eval_batch(P, T)
    rL, rst = orc.generate_batch(2, w["plength"], w["x"], y, P, T)
    assert np.array_equal(st, rst)
    check_logL(logL, rL)


def test_status_codes_nan_and_empty_window(accel_mod, orc):
    w = W.make(2, Nx=3000)
    b = W.split(w)
    y = spectrum_for(orc, w)
    P = W.perturbed(w, 4, scale=0.002)
    P[1, b["q"] + 1] = -1.0            # negative trunc_c -> empty window (reference: exit)
    P[2, b["z"] + 9] = np.nan          # NaN white noise -> NaN logL -> "reject"
    T = synth.temperatures(4)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        logL, st = acc.eval_batch(P, T)
    rL, rst = orc.generate_batch(2, w["plength"], w["x"], y, P, T)
    assert list(st) == [0, 2, 1, 0] == list(rst)
    assert np.isnan(logL[1]) and np.isnan(logL[2])
    check_logL(logL[[0, 3]], rL[[0, 3]])


def test_modes_outside_the_grid_and_window_clamps(accel_mod, orc):
    w = W.make(2, Nx=6000)
    b = W.split(w)
    y = spectrum_for(orc, w)
    P = W.perturbed(w, 3, scale=0.001)
    f0 = b["Nmax"] + b["lmax"]
    P[0, f0] = 2000.0                   # l=0 mode far below the grid (pmax reset to x0 + c)
    P[1, f0 + 3 * b["Nmax"] - 1] = 5000.0   # l=2 mode far above the grid (pmin reset to x_last - c)
    P[2, b["w"]:b["w"] + b["Nmax"]] = 0.3   # widths < 1 -> the Gamma <= 1 window branches
    T = np.ones(3)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        logL, st, models = acc.eval_batch(P, T, model_rows=[0, 1, 2])
    rL, rst, rm = orc.generate_batch(2, w["plength"], w["x"], y, P, T, want_models=True)
    assert np.array_equal(st, rst)
    assert np.max(np.abs(models - rm) / rm) <= RTOL_MODEL
    check_logL(logL, rL)


def test_full_size_c2_64_chains(accel_mod, orc):
    """BASELINE config C2: 64 chains x 1e5 bins, model id 2 (and id 3), against the oracle."""
    for mid in (2, 3):
        w = synth.workload_c2(model_case=mid)
        y = spectrum_for(orc, w)
        P = synth.chain_params(w, 64)
        T = synth.temperatures(64)
        with accel_mod.Accel(mid, w["plength"], w["x"], y) as acc:
            logL, st = acc.eval_batch(P, T)
            logL2, _ = acc.eval_batch(P, T)
        rL, rst = orc.generate_batch(mid, w["plength"], w["x"], y, P, T)
        assert np.array_equal(st, rst) and np.all(st == 0)
        check_logL(logL, rL)
        assert np.array_equal(logL, logL2)          # fixed-order reductions: bitwise reproducible


def test_full_size_c4_106_params(accel_mod, orc):
    w = synth.workload_c4()
    y = spectrum_for(orc, w)
    P = synth.chain_params(w, 16)
    T = synth.temperatures(16)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        logL, st = acc.eval_batch(P, T)
    rL, rst = orc.generate_batch(2, w["plength"], w["x"], y, P, T)
    assert np.array_equal(st, rst)
    check_logL(logL, rL)


def test_c1_local_basic(accel_mod, orc):
    w = synth.workload_c1()
    y = spectrum_for(orc, w)
    P = synth.chain_params(w, 8)
    T = synth.temperatures(8)
    with accel_mod.Accel(11, w["plength"], w["x"], y) as acc:
        logL, st = acc.eval_batch(P, T)
    rL, rst = orc.generate_batch(11, w["plength"], w["x"], y, P, T)
    assert np.array_equal(st, rst)
    check_logL(logL, rL)


def test_size_independent_properties_full_size(accel_mod, orc):
    """Properties that need no oracle: tempering is a pure 1/T scale, chains are independent of their
    position in the batch, and the mode part of the model is linear in the heights."""
    w = synth.workload_c2()
    y = spectrum_for(orc, w)
    P = synth.chain_params(w, 32)
    T = synth.temperatures(32)
    b = W.split(w)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        L, _ = acc.eval_batch(P, T)
        L1, _ = acc.eval_batch(P, np.ones(32))
        perm = np.random.default_rng(1).permutation(32)
        Lp, _ = acc.eval_batch(P[perm], T[perm])
        p0 = w["params_true"].copy(); p0[:b["Nmax"]] = 0.0
        p3 = w["params_true"].copy(); p3[:b["Nmax"]] *= 3.0
        m, _ = acc.model_explicit(w["params_true"])
        mb, _ = acc.model_explicit(p0)
        m3, _ = acc.model_explicit(p3)
    assert np.allclose(L, L1 / T, rtol=1e-15)
    assert np.array_equal(Lp, L[perm])
    assert np.allclose(m3 - mb, 3.0 * (m - mb), rtol=1e-11, atol=1e-13)


def test_model_def_mirror(accel_mod, orc):
    """The Model_def-shaped host mirror: generate_model(m) per chain == generate_models() batched."""
    from tamcmc_amd.model_def import ModelDef, Data
    w = W.make(2, Nx=3000)
    y = spectrum_for(orc, w)
    T = synth.temperatures(4)
    md = ModelDef(Data(w["x"], y), 2, w["plength"], w["params_true"], w["relax"], T, prior_fct=lambda p: -0.5)
    md.vars[:] = W.perturbed(w, 4, scale=0.003)[:, md.index_to_relax]
    for m in range(4):
        md.update_params_with_vars(m)
    post = md.generate_models(model_rows=[0]).copy()
    single = np.array([md.generate_model(md.data, m, T) for m in range(4)])
    assert np.array_equal(post, single)
    rL, _ = orc.generate_batch(2, w["plength"], w["x"], y, md.params, T)
    check_logL(md.logLikelihood, rL)
    assert np.allclose(md.logPosterior, md.logLikelihood - 0.5)
    rm, _ = orc.model(2, md.params[0], w["plength"], w["x"])
    assert np.max(np.abs(md.model[0] - rm) / rm) <= RTOL_MODEL
    assert np.max(np.abs(md.call_model(md.data, 0) - rm) / rm) <= RTOL_MODEL
    md.close()


def test_large_grid_and_many_chains(accel_mod, orc):
    """Nx = 1e6 (the reference's own row limit, config.cpp:531): 245 tiles per chain, more than one pass of the
    setup kernel's tile loops; and 256 chains (config C3's total) in one batch."""
    w = synth.workload_c2(Nx=1000000)
    w["x"] = synth.grid(1000000, 2300.0, 840.0 / 1000000)
    y = spectrum_for(orc, w)
    P = synth.chain_params(w, 6)
    T = synth.temperatures(6)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        acc.set_vars(w["index_to_relax"])
        logL, st = acc.eval_batch(P, T)
        logLg, stg, g = acc.eval_batch(P, T, grad=True)
    rL, rst = orc.generate_batch(2, w["plength"], w["x"], y, P, T)
    assert np.array_equal(st, rst) and np.array_equal(stg, rst)
    check_logL(logL, rL)
    check_logL(logLg, rL)
    assert np.all(np.isfinite(g))
    gradcheck.check_against_oracle(None, orc, 2, w, y, P, T, tag="Nx = 1e6", g=g)
    w2 = synth.workload_c2(Nx=20000)
    y2 = spectrum_for(orc, w2)
    P2 = synth.chain_params(w2, 256)
    T2 = synth.temperatures(256)
    with accel_mod.Accel(2, w2["plength"], w2["x"], y2) as acc:
        L2, st2 = acc.eval_batch(P2, T2)
        L2b, _ = acc.eval_batch(P2[:3], T2[:3])        # a smaller batch on the same context afterwards
    rL2, rst2 = orc.generate_batch(2, w2["plength"], w2["x"], y2, P2, T2)
    assert np.array_equal(st2, rst2)
    check_logL(L2, rL2)
    assert np.array_equal(L2b, L2[:3])


def test_launch_order_does_not_change_results(accel_mod, orc, monkeypatch):
    """The eval launch is tile-major and costliest-first (rank table from the setup kernel).  Results must be bitwise
    the same for the chain-major order (TAMCMC_ORDER=0), plain tile-major (1) and ranked (2, default), and for a tile
    count above TM_ORDER_MAX = 1024, where the rank table is the identity and tiles have equal length; and for other
    tile counts, cost models of the balancer and equal-length tiles (agreement to rounding)."""
    w = synth.workload_c2(Nx=30000)
    y = spectrum_for(orc, w)
    P = synth.chain_params(w, 5)
    T = synth.temperatures(5)
    res = []
    for mode in ("0", "1", "2"):
        monkeypatch.setenv("TAMCMC_ORDER", mode)
        with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
            acc.set_vars(w["index_to_relax"])
            L, st = acc.eval_batch(P, T)
            Lg, stg, g = acc.eval_batch(P, T, grad=True)
        res.append((L, Lg, g))
    for r in res[1:]:
        assert np.array_equal(r[0], res[0][0]) and np.array_equal(r[1], res[0][1]) and np.array_equal(r[2], res[0][2])
    rL, _ = orc.generate_batch(2, w["plength"], w["x"], y, P, T)
    check_logL(res[2][0], rL)
    monkeypatch.delenv("TAMCMC_ORDER")
    # other tile boundaries (equal cost instead of equal length; other tile counts; rank priority): other partial sums,
    # same answer to rounding; gradient against the default geometry
    for env in (dict(TAMCMC_EQUAL_COST="1"), dict(TAMCMC_EQUAL_COST="1", TAMCMC_TILES="33", TAMCMC_TILES_GRAD="29", TAMCMC_PRIO="1"),
                dict(TAMCMC_TILES="9", TAMCMC_TILES_GRAD="11"),
                dict(TAMCMC_TILES="40", TAMCMC_TILES_GRAD="59", TAMCMC_COST="10,1,1", TAMCMC_COST_GRAD="500,40,3")):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
            acc.set_vars(w["index_to_relax"])
            L, st = acc.eval_batch(P, T)
            Lg, stg, g = acc.eval_batch(P, T, grad=True)
        assert np.all(st == 0) and np.all(stg == 0)
        check_logL(L, rL)
        check_logL(Lg, rL)
        assert np.max(np.abs(g - res[2][2]) / np.max(np.abs(res[2][2]), axis=1, keepdims=True)) < 1e-11
        for k in env:
            monkeypatch.delenv(k)

    w = synth.workload_c2(Nx=1200000)
    w["x"] = synth.grid(1200000, 2300.0, 840.0 / 1200000)
    y = spectrum_for(orc, w)
    P = synth.chain_params(w, 2)
    T = synth.temperatures(2)
    monkeypatch.setenv("TAMCMC_TILES", "1200")          # more tiles than TM_ORDER_MAX: equal-length tiles, launched in tile order
    monkeypatch.setenv("TAMCMC_TILES_GRAD", "1300")
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        acc.set_vars(w["index_to_relax"])
        assert acc.geometry()["tiles"] == 1200
        L, st = acc.eval_batch(P, T)
        Lg, stg, g = acc.eval_batch(P, T, grad=True)
    rL, rst = orc.generate_batch(2, w["plength"], w["x"], y, P, T)
    assert np.array_equal(st, rst)
    check_logL(L, rL)
    check_logL(Lg, rL)
    assert np.all(np.isfinite(g))
    # the same gradient from the default geometry (293 tiles, ranked launch order)
    monkeypatch.delenv("TAMCMC_TILES")
    monkeypatch.delenv("TAMCMC_TILES_GRAD")
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        acc.set_vars(w["index_to_relax"])
        assert acc.geometry()["tiles"] < 1024
        Ld, std, gd = acc.eval_batch(P, T, grad=True)
    check_logL(Ld, rL)
    assert np.max(np.abs(g - gd) / np.max(np.abs(gd), axis=1, keepdims=True)) < 1e-10


def test_equal_cost_tiles_follow_the_chain_not_the_batch(accel_mod, orc, monkeypatch):
    """With TAMCMC_EQUAL_COST=1 tile boundaries are chosen per chain from that chain's own truncation windows
    (tamcmc_setup_body.h): chains with
    very different window patterns in one batch -- narrow windows (most of the grid is background only), the default,
    and windows that span the whole grid -- each give bit for bit what they give evaluated alone, and all agree with
    the oracle."""
    w = synth.workload_c2(Nx=60000)
    y = spectrum_for(orc, w)
    P = synth.chain_params(w, 9)
    T = synth.temperatures(9)
    q = W.split(w)["cfg"]
    P[0:3, q] = 1.5        # trunc_c: windows of a few hundred bins
    P[6:9, q] = 10000.0    # no truncation
    monkeypatch.setenv("TAMCMC_EQUAL_COST", "1")
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        acc.set_vars(w["index_to_relax"])
        L, st = acc.eval_batch(P, T)
        Lg, stg, g = acc.eval_batch(P, T, grad=True)
        for k in (0, 4, 8):
            L1, st1 = acc.eval_batch(P[k:k + 1], T[k:k + 1])
            Lg1, _, g1 = acc.eval_batch(P[k:k + 1], T[k:k + 1], grad=True)
            assert L1[0] == L[k] and Lg1[0] == Lg[k] and np.array_equal(g1[0], g[k])
    rL, rst = orc.generate_batch(2, w["plength"], w["x"], y, P, T)
    assert np.array_equal(st, rst) and np.array_equal(stg, rst)
    check_logL(L, rL)
    check_logL(Lg, rL)


def test_more_than_64_multiplets(accel_mod, orc):
    """Nmax = 20, l = 0..3: 80 multiplets per chain -- the setup kernel's second pass over its multiplet lanes, the
    eval kernel's long active lists, and 136 gradient variables."""
    w = synth.workload_c4(Nx=30000, Nmax=20)
    y = spectrum_for(orc, w)
    P = synth.chain_params(w, 3)
    T = synth.temperatures(3)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        assert acc.geometry()["n_multiplets"] == 80
        acc.set_vars(w["index_to_relax"])
        L, st = acc.eval_batch(P, T)
        Lg, stg, g = acc.eval_batch(P, T, grad=True)
    rL, rst = orc.generate_batch(2, w["plength"], w["x"], y, P, T)
    assert np.array_equal(st, rst) and np.array_equal(stg, rst)
    check_logL(L, rL)
    check_logL(Lg, rL)
    gradcheck.check_against_oracle(None, orc, 2, w, y, P, T, tag="80 multiplets, 136 variables", g=g)
    # a few gradient entries against central differences of the oracle (all variables would take minutes)
    idx = w["index_to_relax"]
    pick = idx[[0, 21, 45, 80, idx.size - 12, idx.size - 1]]
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        acc.set_vars(pick)
        _, _, gp = acc.eval_batch(P[:1], T[:1], grad=True)
    gfd, st2 = orc.grad_fd(2, w["plength"], w["x"], y, P[0], T[0], pick, rel_step=1e-6)
    assert st2 == 0
    assert np.max(np.abs(gp[0] - gfd)) <= 2e-4 * np.max(np.abs(gfd))       # windows are on (trunc_c = 20): FD sees their edges
    cols = [int(np.flatnonzero(idx == v)[0]) for v in pick]
    assert np.array_equal(gp[0], g[0][cols])


def test_fused_launch_many_chains_changing_params(accel_mod, orc, monkeypatch):
    """The fused launch reads the records it has just written through the scalar cache, and neighbouring chains' records
    share cache lines (tamcmc_fused.hip): thousands of one-tile chains, parameters changing from call to call, must
    stay bit-identical to the two-launch path (which has a kernel boundary between writer and reader)."""
    w = W.any_model(11, Nx=600, trunc_c=20.0)
    y = spectrum_for(orc, w)
    n = 4096
    T = np.tile(synth.temperatures(8), n // 8)
    batches = [W.perturbed(w, n, scale=0.002 * (k + 1), seed=50 + k) for k in range(3)]
    res = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("TAMCMC_FUSED", fused)
        with accel_mod.Accel(11, w["plength"], w["x"], y) as acc:
            assert acc.geometry()["tiles"] == 1
            acc.set_vars(w["index_to_relax"])
            out = []
            for P in batches:                       # same context: the records of the previous call are still in memory
                L, st = acc.eval_batch(P, T)
                Lg, stg, g = acc.eval_batch(P, T, grad=True)
                out.append((L, st, Lg, stg, g))
        res[fused] = out
    for a, b in zip(res["1"], res["0"]):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    sel = np.arange(0, n, 257)
    rL, rst = orc.generate_batch(11, w["plength"], w["x"], y, batches[2][sel], T[sel])
    assert np.array_equal(res["1"][2][1][sel], rst)
    check_logL(res["1"][2][0][sel], rL)


@pytest.mark.parametrize("Nx", [973, 2048, 400])
def test_fused_small_grid_launch_equals_two_launches(accel_mod, orc, monkeypatch, Nx):
    """Grids of <= 2048 bins are one tile per chain, and the prologue and the evaluation then share a launch
    (tamcmc_fused.hip).  Same code, same arithmetic: bit-identical to the two-launch path (TAMCMC_FUSED=0)."""
    w = W.any_model(11, Nx=Nx, trunc_c=20.0)
    y = spectrum_for(orc, w)
    P = W.perturbed(w, 7, scale=0.002, seed=3)
    T = synth.temperatures(7)
    res = []
    for fused in ("1", "0"):
        monkeypatch.setenv("TAMCMC_FUSED", fused)
        with accel_mod.Accel(11, w["plength"], w["x"], y) as acc:
            assert acc.geometry()["tiles"] == 1
            acc.set_vars(w["index_to_relax"])
            L, st = acc.eval_batch(P, T)
            Lg, stg, g = acc.eval_batch(P, T, grad=True)
        res.append((L, st, Lg, stg, g))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    rL, rst = orc.generate_batch(11, w["plength"], w["x"], y, P, T)
    assert np.array_equal(res[0][1], rst)
    check_logL(res[0][0], rL)
    check_logL(res[0][2], rL)


def test_one_tile_by_hand_on_a_grid_longer_than_the_fused_kernel(accel_mod, orc, monkeypatch):
    """TAMCMC_TILES=1 on a grid of 9..16 units (4609..8192 bins): one likelihood tile per chain is legal there (tiles of up
    to 16 units) but the fused setup + evaluation launch holds at most 8 units -- the call must take the two-launch
    path (it used to return TAMCMC_E_HIP), same logL as the default geometry to rounding; logL and gradient of the gradient path too."""
    w = W.make(2, Nx=6000)                    # 12 units
    y = spectrum_for(orc, w)
    P = W.perturbed(w, 5, scale=0.003)
    T = synth.temperatures(5)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        acc.set_vars(w["index_to_relax"])
        L0, st0 = acc.eval_batch(P, T)
        Lg0, _, g0 = acc.eval_batch(P, T, grad=True)
    monkeypatch.setenv("TAMCMC_TILES", "1")
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        acc.set_vars(w["index_to_relax"])
        L1, st1 = acc.eval_batch(P, T)
        assert acc.geometry()["tiles"] == 1
        Lg1, _, g1 = acc.eval_batch(P, T, grad=True)
    rL, rst = orc.generate_batch(2, w["plength"], w["x"], y, P, T)
    assert np.array_equal(st1, rst) and np.array_equal(st0, rst)
    check_logL(L1, rL)
    check_logL(L0, rL)
    assert np.array_equal(Lg0, Lg1) and np.array_equal(g0, g1)      # the gradient launch's tiles are not touched by TAMCMC_TILES


def test_likelihood_and_gradient_paths_return_the_same_logL_bits(accel_mod, orc, monkeypatch):
    """With the same tile geometry the in-launch finalize of the likelihood kernel and the backward kernel's finalize add
    the same partials in the same order with the same arithmetic (tm_tile_logsum, tamcmc_dev.h): identical bits."""
    w = synth.workload_c2(Nx=30000)
    y = spectrum_for(orc, w)
    P = synth.chain_params(w, 7)
    T = synth.temperatures(7)
    monkeypatch.setenv("TAMCMC_TILES", "10")
    monkeypatch.setenv("TAMCMC_TILES_GRAD", "10")
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        acc.set_vars(w["index_to_relax"])
        L, st = acc.eval_batch(P, T)
        Lg, stg, g = acc.eval_batch(P, T, grad=True)
    assert np.all(st == 0) and np.array_equal(L, Lg)


def test_armed_batches_equal_plain_batches(accel_mod, orc):
    """tamcmc_eval_batch_arm / _fire / _disarm: the launches of the next batch wait in the stream behind a gate while the
    current one is evaluated, and run on the parameters handed to _fire -- results bit for bit those of a plain batch,
    over many rounds with changing parameters (the gate value wraps nothing, buffers are reused); an armed batch that is
    never fired is disarmed (explicitly, and by destroying the context) without a hang; misuse is refused."""
    w = synth.workload_c2(Nx=40000)
    y = spectrum_for(orc, w)
    n = 16
    T = synth.temperatures(n)
    P = [synth.chain_params(w, n, seed=300 + k) for k in range(10)]
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        ref = [acc.eval_batch(Pk, T) for Pk in P]
        acc.begin(P[0], T)
        for k in range(1, len(P)):
            acc.arm(n)                                   # under batch k-1, still in flight
            L, st = acc.end()
            assert np.array_equal(L, ref[k - 1][0]) and np.array_equal(st, ref[k - 1][1])
            acc.fire(P[k], T)
        # results arrive chain by chain: poll() hands each one out once it is there (None before), _end is still due
        got, tries = {}, 0
        while len(got) < n and tries < 10 ** 7:
            for m in range(n):
                if m not in got:
                    r = acc.poll(m)
                    if r is not None:
                        got[m] = r
            tries += 1
        assert len(got) == n
        assert np.array_equal(np.array([got[m][0] for m in range(n)]), ref[-1][0])
        assert np.array_equal(np.array([got[m][1] for m in range(n)], dtype=np.int32), ref[-1][1])
        with pytest.raises(accel_mod.AccelError):
            acc.poll(n)                                  # not a chain of the batch
        acc.arm(n)
        for bad in (lambda: acc.begin(P[0], T), lambda: acc.eval_batch(P[0], T), lambda: acc.arm(n), lambda: acc.reserve(4 * n),
                    lambda: acc.set_stream(0), lambda: acc.synchronize(),        # (would wait for the gate)
                    lambda: acc.disarm()):              # (a batch is in flight: collect it first)
            with pytest.raises(accel_mod.AccelError):
                bad()
        L, st = acc.end()
        assert np.array_equal(L, ref[-1][0]) and np.array_equal(st, ref[-1][1])
        with pytest.raises(accel_mod.AccelError):
            acc.fire(P[0][:8], T[:8])                    # not the armed size
        acc.disarm()                                     # never fired: runs on the previous parameters, nothing handed out
        acc.disarm()                                     # (idempotent)
        L, st = acc.eval_batch(P[3], T)                  # the context is fine afterwards
        assert np.array_equal(L, ref[3][0])
        rL, _ = orc.generate_batch(2, w["plength"], w["x"], y, P[3], T)
        check_logL(L, rL)
        acc.arm(n)                                       # ... and a context destroyed with a batch armed does not hang


def test_an_expired_gate_costs_time_not_results(accel_mod, orc, monkeypatch):
    """The gate of an armed batch gives up after TAMCMC_GATE_PATIENCE polls (a wave must not outlive its host).  A host
    that fires later than that must still get the right answer: _fire sees the expiry, lets the stale launches drain and
    evaluates the batch the plain way; _disarm of an expired batch just lets it retire."""
    import time
    monkeypatch.setenv("TAMCMC_GATE_PATIENCE", "2000")          # ~4 ms
    w = synth.workload_c2(Nx=20000)
    y = spectrum_for(orc, w)
    n = 8
    T = synth.temperatures(n)
    P = [synth.chain_params(w, n, seed=400 + k) for k in range(4)]
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        ref = [acc.eval_batch(Pk, T) for Pk in P]
        acc.begin(P[0], T)
        acc.arm(n)
        L, st = acc.end()
        assert np.array_equal(L, ref[0][0])
        time.sleep(0.3)                                          # far beyond the gate's patience
        acc.fire(P[1], T)
        L, st = acc.end()
        assert np.array_equal(L, ref[1][0]) and np.array_equal(st, ref[1][1])
        acc.arm(n)                                               # in time: the normal path again
        acc.fire(P[2], T)
        L, st = acc.end()
        assert np.array_equal(L, ref[2][0])
        acc.arm(n)
        time.sleep(0.3)
        acc.disarm()                                             # expired and never fired
        L, st = acc.eval_batch(P[3], T)
        assert np.array_equal(L, ref[3][0]) and np.array_equal(st, ref[3][1])
