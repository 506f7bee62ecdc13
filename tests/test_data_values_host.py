"""CPU proof that the cases of tests/datacases.py are what they claim (the GPU file compares the device with the oracle at
exactly these cases): the scaled parameter sets are the same star in other units, the special data / temperatures /
exponents give the oracle the statuses and the kinds of logL the suite expects of the device on this platform's libm,
and the oracle's gradient on a grid that starts at x = 0 is finite and right."""
import numpy as np
import pytest

import datacases as D
import workloads as W
from gradcheck import entrywise_error

EPS = np.finfo(np.float64).eps


def identity_bound(L_s, L_1, T, Nx, log_s, models):
    """What the oracle's own roundings can leave of L(s) + Nx ln(s)/T - L(1): its two results are rounded to double (and
    its two sums once more before, likelihoods.cpp:25) -- 4 ulp of the largest of the three terms --, every ln M_i is a
    double (eps/2 |ln M_i| each) and with an s that is no power of two every M_i(s) and y_i(s) carry a rounding of their
    own (a few eps of y_i/M_i ~ 1 and of ln M_i each).  Worst case, no cancellation assumed, per chain."""
    big = np.maximum(np.maximum(np.abs(L_s), np.abs(L_1)), abs(Nx * log_s) / np.abs(T))
    lnM = max(float(np.max(np.abs(np.log(models)))) + abs(log_s), 1.0)
    return 4 * np.spacing(big) + Nx * EPS * (lnM + 8.0) / np.abs(T)


@pytest.mark.parametrize("scale", list(D.SCALES))
@pytest.mark.parametrize("kind", D.POWER_KINDS)
def test_scaled_case_is_the_same_star_in_other_units(orc, kind, scale):
    """A: chi(2,2p): L(s) + p Nx ln(s) / T == L(1); chi-square: L(s) == L(1).  Every model row is s times the base row."""
    s, k = D.SCALES[scale]
    base, case = D.power_case(orc, kind, "fused"), D.power_case(orc, kind, "fused", scale)
    a1, a = D.answers(orc, ("A", kind, "fused", None), base, grad=False), D.answers(orc, ("A", kind, "fused", scale), case, grad=False)
    assert np.all(a1["st"] == 0) and np.all(a["st"] == 0) and np.all(np.isfinite(a["L"])) and np.all(np.isfinite(a1["L"]))
    Nx = base["y"].size
    assert np.all(np.abs(a["models"] - s * a1["models"]) <= 4 * EPS * s * a1["models"])
    if k is not None:
        assert np.array_equal(a["models"], np.ldexp(a1["models"], k))
    if base["like"] == 1:
        assert np.all(np.abs(a["L"] - a1["L"]) <= (0 if k is not None else 8 * EPS) * np.abs(a1["L"]))   # (terms of one sign)
        return
    log_s = k * D.LN2 if k is not None else np.log(np.longdouble(s))
    res = D.identity_residual(a["L"], a1["L"], base["T"], 1, Nx, log_s)
    bound = identity_bound(a["L"], a1["L"], base["T"], Nx, float(log_s), a1["models"])
    print(f"{case['tag']}: residual of the scaling identity {float(np.max(res)):.2e} ({float(np.max(res / bound)):.2f} of its bound) at |L| = {np.max(np.abs(a['L'])):.3e}")
    assert np.all(res <= bound), (res, bound)


def test_a_forgotten_linear_entry_is_caught(orc):
    """The id-13 height block left unscaled: the identity misses by orders of magnitude more than its bound."""
    base = D.power_case(orc, "id13", "fused")
    pl = base["w"]["plength"]
    q = int(pl[:9].sum())
    wrong = D.scaled(base, 2.0 ** 200, scale_params=np.array([i for i in base["lin"] if not q <= i < q + int(pl[9])]))
    a1 = D.answers(orc, ("A", "id13", "fused", None), base, grad=False)
    L, st = orc.generate_batch(13, base["w"]["plength"], base["w"]["x"], wrong["y"], wrong["P"], wrong["T"])
    res = D.identity_residual(L, a1["L"], base["T"], 1, base["y"].size, 200 * D.LN2)
    bound = identity_bound(L, a1["L"], base["T"], base["y"].size, float(200 * D.LN2), a1["models"])
    assert np.all(st == 0) and np.all(res > 1e6 * bound)


def expected_of_batch(case, batch):
    return [(0, "finite") if case["what"][s][0] in ("base", "all-zero") else D.expected_kind(case["what"][s][2]) for s in batch["smap"]]


@pytest.mark.parametrize("kind", list(D.SPECIAL_KINDS))
def test_special_data_give_the_expected_kinds_of_result(orc, kind):
    """B: 0, a negative value, 5e-324, 1e300 and an all-zero spectrum: status 0, finite logL and gradient; +inf: -inf,
    status 0; NaN: status 1.  The damaged bins are where they claim to be."""
    case = D.special_data_case(orc, kind)
    bins = case["bins"]
    assert len(set(bins.values())) == 4 and len(case["spectra"]) == 2 + 4 * len(D.DATA_VALUES)
    seen = set()
    for b, batch in enumerate(case["batches"]):
        ans = D.batch_answers(orc, ("B", kind, b), case, batch)
        want = expected_of_batch(case, batch)
        assert D.classify(ans["L"], ans["st"]) == want
        fin = np.array([k == "finite" for _, k in want])
        assert np.all(np.isfinite(ans["g"][fin])) and np.all(ans["gst"][fin] == 0)
        assert np.any(batch["smap"] == 0) and batch["smap"][0] == 0 and batch["smap"][-1] == 0
        seen |= set(batch["smap"].tolist())
    assert seen == set(range(len(case["spectra"])))


def test_special_sigma_give_the_expected_kinds_of_result(orc):
    """B, chi-square: sigma = 0 and 1e-200 (sigma^2 underflows): -inf; negative, inf, 1e200: finite; NaN: status 1."""
    case = D.sigma_case(orc)
    batch = case["batches"][0]
    ans = D.batch_answers(orc, ("B", "sigma", 0), case, batch)
    want = {0.0: (0, "-inf"), -0.3: (0, "finite"), np.inf: (0, "finite"), 1e-200: (0, "-inf"), 1e200: (0, "finite")}
    exp = [(0, "finite") if s == 0 else (1, "nan") if D.SIGMA_VALUES[s - 1] != D.SIGMA_VALUES[s - 1] else want[D.SIGMA_VALUES[s - 1]]
           for s in batch["smap"]]
    assert D.classify(ans["L"], ans["st"]) == exp
    fin = np.array([k == "finite" for _, k in exp])
    assert np.all(np.isfinite(ans["g"][fin]))


@pytest.mark.parametrize("grid", ["fused", "tiled"])
def test_negative_model_values_give_nan(orc, grid):
    """B: id 0 with a negative amplitude and constant (every model value negative; the builder asserts the counts) or a
    negative constant alone: log of a negative number, NaN and status 1; the chains between them are healthy."""
    case = D.negative_model_case(orc, grid)
    ans = D.answers(orc, ("B", "negM", grid), case)
    assert D.classify(ans["L"], ans["st"]) == [(0, "finite"), (1, "nan"), (0, "finite"), (1, "nan")]
    assert np.all(np.isfinite(ans["g"][[0, 2]])) and np.all(ans["gst"][[0, 2]] == 0)


@pytest.mark.parametrize("kind", list(D.SPECIAL_KINDS))
def test_special_temperatures_give_the_expected_kinds_of_result(orc, kind):
    """B: T = 0 and 5e-324: an infinity of logL's sign, T = inf: a zero of logL's sign -- for id 2, whose logL is negative,
    -inf and -0; NaN: status 1; 1e-300, 1e300, -2: finite logL and gradient."""
    case = D.special_data_case(orc, kind)
    batch = D.temperature_batch(case)
    ans = D.batch_answers(orc, ("B", kind, "T"), case, batch)
    got = D.classify(ans["L"], ans["st"])
    w = case["w"]
    L1, _ = orc.generate_batch(case["mid"], w["plength"], w["x"], case["y"], batch["P"], np.ones(len(batch["T"])))
    assert np.all(L1 < 0) if kind == "id2" else np.all(L1 > 0)
    sg = "-" if kind == "id2" else "+"
    want = {0.0: (0, sg + "inf"), 5e-324: (0, sg + "inf"), 1e-300: (0, "finite"), 1e300: (0, "finite"), np.inf: (0, sg + "0"),
            -2.0: (0, "finite")}
    for t, g, grow in zip(batch["T"], got, ans["g"]):
        assert g == ((1, "nan") if t != t else want.get(t, (0, "finite"))), (t, g)
        if g == (0, "finite"):
            assert np.all(np.isfinite(grow)), t
    assert set(D.T_VALUES) - {np.nan} <= set(batch["T"].tolist()) and np.isnan(batch["T"]).sum() == 1


@pytest.mark.parametrize("p", D.P_VALUES)
def test_likelihood_p_is_truncated(orc, p):
    """B: likelihood_p = 0 and 0.9 are p = 0 (logL is a zero), -1 and 3 are themselves."""
    case = D.special_data_case(orc, "id11")
    w = case["w"]
    L1, st1 = orc.generate_batch(11, w["plength"], w["x"], case["y"], case["P"], case["T"])
    L, st = orc.generate_batch(11, w["plength"], w["x"], case["y"], case["P"], case["T"], likelihood_p=p)
    g, gabs, _, gst = orc.grad_analytic(11, w["plength"], w["x"], case["y"], case["P"], case["T"], w["index_to_relax"], likelihood_p=p)
    assert np.all(st == 0) and np.all(gst == 0) and np.all(np.isfinite(g))
    if int(p) == 0:
        assert np.all(L == 0) and np.all(g == 0)
    else:
        assert np.all(np.abs(L - int(p) * L1) <= 2 * EPS * np.abs(L))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", D.ZERO_KINDS)
def test_gradient_on_a_grid_that_starts_at_zero(orc, kind):
    """C: the oracle's analytic gradient is finite with x[0] = 0; its Harvey entries agree with finite differences
    (bar of tests/test_oracle_grad.py; the windows do not depend on them) and with the same case without bin 0: tau and
    p entries unchanged (t = 0 there: the limit of t ln(sx) is 0), every H entry less the weight of that bin (u = 1)."""
    case = D.zero_grid_case(orc, kind)
    w, mid, P, T, y = case["w"], case["mid"], case["P"], case["T"], case["y"]
    idx = w["index_to_relax"]
    hv = D.harvey_entries(w)
    for name in ("H", "tau", "p"):
        assert set(hv[name]) <= set(idx.tolist())       # every active H, tau and p is a variable
    g, gabs, L, st = orc.grad_analytic(mid, w["plength"], w["x"], y, P, T, idx)
    assert np.all(st == 0) and np.all(np.isfinite(L)) and np.all(np.isfinite(g)) and np.all(np.isfinite(gabs))
    if kind == "id2-tiled":
        with np.errstate(divide="ignore"):
            assert W.poly_cells(w) == (0, 7)                # every cell takes the exp path, the first with log x = -inf in it
    if not hv["H"]:
        return
    noise_vars = np.array(sorted(hv["H"] + hv["tau"] + hv["p"]), dtype=np.int32)
    worst = entrywise_error(orc, mid, w, y, P[:1], T[:1], noise_vars)
    # the same case with bin 0 dropped
    w1 = dict(w, x=w["x"][1:])
    _, _, rm = orc.generate_batch(mid, w["plength"], w["x"], y, P, T, want_models=True)
    _, _, rm1 = orc.generate_batch(mid, w["plength"], w1["x"], y[1:], P, T, want_models=True)
    assert np.array_equal(rm[:, 1:], rm1)                   # (same windows: nothing but bin 0 differs)
    g1, gabs1, _, st1 = orc.grad_analytic(mid, w["plength"], w1["x"], y[1:], P, T, idx)
    col = {int(v): j for j, v in enumerate(idx)}
    for name in ("tau", "p"):
        for i in hv[name]:
            assert np.all(np.abs(g[:, col[i]] - g1[:, col[i]]) <= 2 * EPS * gabs[:, col[i]]), (name, i)
    w0 = (y[0] / rm[:, 0] ** 2 - 1.0 / rm[:, 0]) / T        # d(logL/T)/dM_0
    for i in hv["H"]:
        d = g[:, col[i]] - g1[:, col[i]]
        assert np.all(np.abs(d - np.sign(P[:, i]) * w0) <= 1e-12 * gabs[:, col[i]]), ("H", i, d, w0)
    print(f"{case['tag']}: Harvey entries within {worst:.1e} of finite differences; p entries {g[0, [col[i] for i in hv['p']]]}")
