"""Data-side suite of the three launches (likelihood, likelihood with a model row, gradient launch + backward) against
the oracle: the data a context is created with, the temperatures and likelihood_p at values outside the one decade of
synth.make_spectrum -- tests/datacases.py builds the cases, tests/test_data_values_host.py proves them on the CPU.

  A  the same star in other units of power (s = 1e-12, 1e12, 2^-200, 2^200; ids 2, 13, 11, 1 and chi-square; fused grid,
     tiled grid with tiles of equal length and of equal cost).  With s = 2^k the device's own arithmetic must scale: model
     rows and gradient entries bit for bit, chi-square logL bit for bit, chi(2,2p) logL up to the exponent sums;
  B  one datum 0 / negative / 5e-324 / 1e300 / +inf / NaN (in a window, outside every window, in a tile's first row, in
     the partial last unit), an all-zero spectrum, one sigma_y 0 / negative / inf / NaN / 1e-200 / 1e200, one temperature
     0 / 5e-324 / 1e-300 / 1e300 / inf / -2 / NaN, likelihood_p 0 / 0.9 / -1 / 3 -- damaged and healthy spectra in one
     batch of a multi-spectrum context, healthy chains bit for bit what they are alone, all contexts in one fit group;
     id 0 with negative model values (an even number in every tile: only the collected sign bits give the NaN);
  C  grids that start at x = 0 (ids 2 fused and tiled, 1, 11) with every active Harvey H, tau and p a variable;
  D  tamcmc_eval_batch_device with a gradient buffer: bit for bit eval_batch(grad=True).

Rules: status identical to the oracle's in every launch; logL NaN exactly where the oracle's is, +-inf with its sign, a
zero where it has a zero of either sign, else 1e-10 relative (1e-12 between the device's launches); model rows 1e-12 per
bin; gradient rows (tests/gradcheck.py, unchanged) where the oracle's logL and whole row are finite.

Every test prints its worst figures (logL, model bin, gradient entry in S_k and relative; part A also the residual of the
scaling identity in ulp of |L(s)|)."""
import numpy as np
import pytest

import datacases as D
from support import in_torch_process
from test_edges_gpu import Worst, check_grad, check_rows

pytestmark = pytest.mark.gpu

RTOL_LOGL = 1e-10
RTOL_PATHS = 1e-12


def same_bits(a, b):
    """Bit for bit; a NaN equals a NaN (no payload is promised)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))


def logL_mismatch(L, ref, rtol):
    """(mask of the chains that break the rule, worst relative error of those that are compared by value and keep it)."""
    L, ref = np.asarray(L, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nan, inf, zero = np.isnan(ref), np.isinf(ref), ref == 0
    val = ~(nan | inf | zero)
    bad = np.zeros(L.shape, dtype=bool)
    bad[nan] = ~np.isnan(L[nan])
    bad[inf] = L[inf] != ref[inf]
    bad[zero] = L[zero] != 0
    with np.errstate(all="ignore"):
        err = np.abs(L[val] - ref[val]) / np.abs(ref[val])
    good = err <= rtol
    bad[val] = ~good
    return bad, float(np.max(err[good], initial=0.0))


def check_logL(L, st, ref_L, ref_st, tag, worst, failures, rtol=RTOL_LOGL):
    if not np.array_equal(st, ref_st):
        k = np.flatnonzero(np.asarray(st) != np.asarray(ref_st))
        failures.append(f"{tag}: status of chain {k[0]} is {st[k[0]]}, expected {ref_st[k[0]]} ({k.size} chains differ)")
        return False
    bad, err = logL_mismatch(L, ref_L, rtol)
    if np.any(bad):
        k = int(np.flatnonzero(bad)[0])
        failures.append(f"{tag}: logL of chain {k} is {L[k]!r}, expected {ref_L[k]!r} ({int(bad.sum())} chains differ)")
        return False
    if rtol == RTOL_LOGL:
        worst.L = max(worst.L, err)
    return True


def comparable_rows(ans):
    """Rows whose gradient is compared: the oracle's logL finite and its whole row finite."""
    return (ans["st"] == 0) & (ans["gst"] == 0) & np.isfinite(ans["L"]) & np.all(np.isfinite(ans["g"]), axis=1) & \
        np.all(np.isfinite(ans["gabs"]), axis=1)


def all_launches(acc, P, T, ans, tag, worst, failures, row=None, model=None):
    """The three launches against the oracle and against each other.  Returns (L, st, g) of the likelihood / gradient launch."""
    L, st = acc.eval_batch(P, T)
    check_logL(L, st, ans["L"], ans["st"], tag + " [likelihood]", worst, failures)
    if row is not None:
        Lr, str_, rows = acc.eval_batch(P, T, model_rows=[row])
        if check_logL(Lr, str_, ans["L"], ans["st"], tag + " [model row]", worst, failures):
            check_rows(rows, model, tag + " [model row]", worst, failures)
        check_logL(Lr, str_, L, st, tag + " [model-row launch against the likelihood launch]", worst, failures, RTOL_PATHS)
    else:
        rows = None
    Lg, stg, g = acc.eval_batch(P, T, grad=True)
    if check_logL(Lg, stg, ans["L"], ans["st"], tag + " [gradient]", worst, failures):
        ok = comparable_rows(ans)
        if np.any(ok):
            check_grad(g[ok], ans["g"][ok], ans["gabs"][ok], tag + " [gradient]", worst, failures)
    check_logL(Lg, stg, L, st, tag + " [gradient launch against the likelihood launch]", worst, failures, RTOL_PATHS)
    worst.cases += 1
    worst.chains += len(P)
    return dict(L=L, st=st, Lg=Lg, g=g, rows=rows)


def open_accel(accel_mod, case, p=1.0):
    acc = accel_mod.Accel(case["mid"], case["w"]["plength"], case["w"]["x"], case["y"], sigma_y=case["sigma"],
                          likelihood_case=case["like"], likelihood_p=p)
    acc.set_vars(case["w"]["index_to_relax"])
    return acc


def run_case(accel_mod, case, ans, worst, failures):
    with open_accel(accel_mod, case, case["p"]) as acc:
        return all_launches(acc, case["P"], case["T"], ans, case["tag"], worst, failures, row=case["row"], model=ans["models"])


# ---------------------------------------------------------------------------------------------------------------------
# A. power units

GRID_MODES = [("fused", None), ("tiled", 0), ("tiled", 1)]


@pytest.mark.parametrize("grid,balanced", GRID_MODES, ids=["fused", "tiled-equal-length", "tiled-equal-cost"])
@pytest.mark.parametrize("kind", D.POWER_KINDS)
def test_power_units(accel_mod, orc, monkeypatch, kind, grid, balanced):
    """A.  Every factor: the comparison rules against the oracle at the scaled values.  s = 2^k: the model row is
    ldexp(base row, k), the gradient entries of the scaled parameters ldexp(base, -k), all other entries the base's, the
    chi-square logL the base's -- bit for bit -- and chi(2,2p) obeys L(s) + p Nx k ln2 / T = L(1) within 8 x max(the
    oracle's residual of that identity on the case, 1 ulp of |L(s)|): the device's sum of y/M is unchanged, only its
    exponent sums move, and 8 covers the roundings of at most 7 tile log-sums, the final sum, product and division."""
    if balanced is not None:
        monkeypatch.setenv("TAMCMC_EQUAL_COST", str(balanced))
    worst, failures = Worst(), []
    base = D.power_case(orc, kind, grid)
    ans1 = D.answers(orc, ("A", kind, grid, None), base)
    assert np.all(ans1["st"] == 0) and np.all(comparable_rows(ans1))
    r1 = run_case(accel_mod, base, ans1, worst, failures)
    idx = base["w"]["index_to_relax"]
    lin_cols = np.isin(idx, base["lin"])
    assert lin_cols.sum() >= 2 and (~lin_cols).sum() >= 2
    Nx, T = base["y"].size, base["T"]
    ulps = 0.0
    for scale, (s, k) in D.SCALES.items():
        case = D.power_case(orc, kind, grid, scale)
        ans = D.answers(orc, ("A", kind, grid, scale), case)
        assert np.all(ans["st"] == 0) and np.all(comparable_rows(ans)), case["tag"]
        r = run_case(accel_mod, case, ans, worst, failures)
        if k is None:
            continue
        if not same_bits(r["rows"], np.ldexp(r1["rows"], k)):
            failures.append(f"{case['tag']}: the model row is not ldexp(base row, {k}) "
                            f"({int(np.sum(r['rows'] != np.ldexp(r1['rows'], k)))} bins differ)")
        if not same_bits(r["g"][:, lin_cols], np.ldexp(r1["g"][:, lin_cols], -k)):
            j = np.argwhere(r["g"][:, lin_cols] != np.ldexp(r1["g"][:, lin_cols], -k))
            failures.append(f"{case['tag']}: gradient entries of scaled parameters are not ldexp(base, {-k}): {len(j)} entries, "
                            f"first chain {j[0][0]} variable {idx[lin_cols][j[0][1]]}")
        if not same_bits(r["g"][:, ~lin_cols], r1["g"][:, ~lin_cols]):
            j = np.argwhere(r["g"][:, ~lin_cols] != r1["g"][:, ~lin_cols])
            failures.append(f"{case['tag']}: gradient entries of unscaled parameters differ from the base's: {len(j)} entries, "
                            f"first chain {j[0][0]} variable {idx[~lin_cols][j[0][1]]}: {r['g'][:, ~lin_cols][tuple(j[0])]!r}, "
                            f"base {r1['g'][:, ~lin_cols][tuple(j[0])]!r}")
        if base["like"] == 1:
            if not (same_bits(r["L"], r1["L"]) and same_bits(r["Lg"], r1["Lg"])):
                failures.append(f"{case['tag']}: chi-square logL {r['L']!r} is not the base's {r1['L']!r} bit for bit")
            continue
        ref_res = D.identity_residual(ans["L"], ans1["L"], T, 1, Nx, k * D.LN2)
        for name in ("L", "Lg"):
            res = D.identity_residual(r[name], r1[name], T, 1, Nx, k * D.LN2)
            ulp = np.spacing(np.abs(r[name])).astype(np.longdouble)
            bound = 8 * np.maximum(ref_res, ulp)
            ulps = max(ulps, float(np.max(res / ulp)))
            if not np.all(res <= bound):
                failures.append(f"{case['tag']} [{name}]: scaling identity off by {np.asarray(res / ulp, dtype=float)} ulp of |L(s)|, "
                                f"oracle {np.asarray(ref_res / ulp, dtype=float)} ulp")
    print(worst.line(f"data A, {kind} {grid}" + ("" if balanced is None else f" {('equal-length', 'equal-cost')[balanced]} tiles")) +
          (f"; scaling identity of s = 2^+-200 within {ulps:.2f} ulp of |L(s)|" if base["like"] == 0 else ""))
    assert not failures, failures[:20]


# ---------------------------------------------------------------------------------------------------------------------
# B. special data, temperatures and likelihood_p

def open_multi(accel_mod, case):
    acc = open_accel(accel_mod, case)
    acc.set_spectra(case["spectra"], case.get("sigmas"))
    return acc


def healthy_chains_alone(solo, batch, r, tag, failures):
    """The chains on the base spectrum: bit for bit what a context that holds only that spectrum returns."""
    h = np.flatnonzero(batch["smap"] == 0)
    L, st = solo.eval_batch(batch["P"][h], batch["T"][h])
    Lg, stg, g = solo.eval_batch(batch["P"][h], batch["T"][h], grad=True)
    if not (np.array_equal(st, r["st"][h]) and same_bits(L, r["L"][h]) and same_bits(Lg, r["Lg"][h]) and same_bits(g, r["g"][h])):
        failures.append(f"{tag}: chains on the healthy spectrum differ from a context of that spectrum alone: "
                        f"{L!r} / {r['L'][h]!r}")


@pytest.mark.parametrize("kind", list(D.SPECIAL_KINDS))
def test_special_data_and_temperatures(accel_mod, orc, monkeypatch, kind):
    """B: damaged spectra and healthy ones in one batch; then special temperatures on the healthy spectrum."""
    for name in ("TAMCMC_EQUAL_COST", "TAMCMC_TILES", "TAMCMC_TILES_GRAD"):     # the tiles of 'tile-first-row' are the default ones
        monkeypatch.delenv(name, raising=False)
    case = D.special_data_case(orc, kind)
    worst, failures = Worst(), []
    model = orc.model(case["mid"], case["P"][0], case["w"]["plength"], case["w"]["x"])[0][None, :]
    with open_multi(accel_mod, case) as acc, open_accel(accel_mod, case) as solo:
        if kind == "id2":
            # 'tile-first-row' is one: 55 units in 11 tiles of equal length (geometry's bins_per_tile is the bound, not the
            # length).  geometry() reports the likelihood launch; below 70 units the gradient launch has the same tile count
            # (tm_tiles takes no account of the launch, the tail shaping of tamcmc_api.cpp starts at 70 units), so bin
            # 3 * 2560 + 7 is in the first row of tile 3 in all three launches.
            assert acc.geometry()["tiles"] * D.TILE_BINS == 55 * 512 and acc.Nx > 54 * 512
        for b, batch in enumerate(case["batches"] + [D.temperature_batch(case)]):
            name = "T" if b == len(case["batches"]) else b
            ans = D.batch_answers(orc, ("B", kind, name), case, batch)
            acc.set_chain_spectrum(batch["smap"])
            tag = f"data B {kind} batch {name}"
            r = all_launches(acc, batch["P"], batch["T"], ans, tag, worst, failures, row=0, model=model)
            healthy_chains_alone(solo, batch, r, tag, failures)
    print(worst.line(f"data B, {kind}: spectra with one special datum, special temperatures"))
    assert not failures, failures[:20]


def test_special_sigma(accel_mod, orc):
    """B, chi-square: one sigma_y 0 / negative / inf / NaN / 1e-200 / 1e200."""
    case = D.sigma_case(orc)
    batch = case["batches"][0]
    ans = D.batch_answers(orc, ("B", "sigma", 0), case, batch)
    worst, failures = Worst(), []
    model = orc.model(case["mid"], case["P"][0], case["w"]["plength"], case["w"]["x"])[0][None, :]
    with open_multi(accel_mod, case) as acc, open_accel(accel_mod, case) as solo:
        acc.set_chain_spectrum(batch["smap"])
        r = all_launches(acc, batch["P"], batch["T"], ans, "data B sigma", worst, failures, row=0, model=model)
        healthy_chains_alone(solo, batch, r, "data B sigma", failures)
    print(worst.line("data B, chi-square with one special sigma_y"))
    assert not failures, failures


@pytest.mark.parametrize("p", D.P_VALUES)
def test_likelihood_p(accel_mod, orc, p):
    """B: likelihood_p = 0 and 0.9 (p = 0: logL and every gradient entry a zero), -1 and 3."""
    case = dict(D.special_data_case(orc, "id11"), p=p)
    ans = D.answers(orc, ("B", "p", p), case)
    worst, failures = Worst(), []
    r = run_case(accel_mod, case, ans, worst, failures)
    if int(p) == 0:
        assert np.all(ans["L"] == 0) and np.all(r["L"] == 0) and np.all(r["g"] == 0)
    print(worst.line(f"data B, likelihood_p = {p}"))
    assert not failures, failures


@pytest.mark.parametrize("grid", ["fused", "tiled"])
def test_negative_model_values(accel_mod, orc, grid):
    """B: id 0 with every model value negative (an even number in every tile, so the tile's mantissa product is positive)
    and with some negative, between healthy chains: NaN and status 1 as the reference's log of a negative number."""
    case = D.negative_model_case(orc, grid)
    ans = D.answers(orc, ("B", "negM", grid), case)
    assert ans["st"].tolist() == [0, 1, 0, 1] and np.isnan(ans["L"]).tolist() == [False, True, False, True]
    worst, failures = Worst(), []
    run_case(accel_mod, case, ans, worst, failures)
    print(worst.line(f"data B, id 0 {grid}: negative model values"))
    assert not failures, failures


def test_special_contexts_in_one_group(accel_mod, orc):
    """B: one tamcmc_group_eval over the part's contexts returns each member's own bits, the -inf, -0 and NaN slots of the
    group's mapped host path included."""
    members = []
    try:
        for kind in D.SPECIAL_KINDS:
            case = D.special_data_case(orc, kind)
            for batch in case["batches"] + [D.temperature_batch(case)]:      # every datum, the +inf and NaN ones included
                acc = open_multi(accel_mod, case)
                acc.set_chain_spectrum(batch["smap"])
                members.append((acc, batch["P"], batch["T"]))
        case = D.sigma_case(orc)
        acc = open_multi(accel_mod, case)
        acc.set_chain_spectrum(case["batches"][0]["smap"])
        members.append((acc, case["batches"][0]["P"], case["batches"][0]["T"]))
        case = D.special_data_case(orc, "id11")
        for p in D.P_VALUES:
            members.append((open_accel(accel_mod, case, p), case["P"], case["T"]))
        solo = [m[0].eval_batch(m[1], m[2]) for m in members]
        with accel_mod.Group([m[0] for m in members]) as grp:
            GL, Gst = grp.eval([m[1] for m in members], [m[2] for m in members])
        kinds = set()
        for k, (L, st) in enumerate(solo):
            assert np.array_equal(Gst[k], st) and same_bits(GL[k], L), (k, GL[k], L)
            kinds |= {c[1] for c in D.classify(L, st)}
        assert {"-inf", "-0", "nan", "finite"} <= kinds, kinds
    finally:
        for m in members:
            m[0].close()


# ---------------------------------------------------------------------------------------------------------------------
# C. grids that start at x = 0

@pytest.mark.parametrize("kind", D.ZERO_KINDS)
def test_grid_that_starts_at_zero(accel_mod, orc, kind):
    """C: log x = -inf in the first bin.  The model there is H (t = 0, u = 1) and d/dp of every Harvey profile takes the
    limit t ln(sx) -> 0: every gradient entry is finite and the oracle's."""
    case = D.zero_grid_case(orc, kind)
    ans = D.answers(orc, ("C", kind), case)
    assert np.all(ans["st"] == 0) and np.all(comparable_rows(ans))
    worst, failures = Worst(), []
    r = run_case(accel_mod, case, ans, worst, failures)
    hv = D.harvey_entries(case["w"])
    cols = np.isin(case["w"]["index_to_relax"], hv["p"])
    print(worst.line(f"data C, {case['tag']}") + f"; d/dp of the Harvey profiles {r['g'][:, cols].tolist()}")
    assert np.all(np.isfinite(r["g"])), (case["tag"], "non-finite gradient entries of variables",
                                         case["w"]["index_to_relax"][np.any(~np.isfinite(r["g"]), axis=0)].tolist())
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# D. device-pointer entry with a gradient buffer

DEVICE_CASES = [("id2", "fused", "2^200"), ("id13", "tiled", "1e-12")]


def _device_grad_check():
    """Body of test_device_entry_with_gradient, in a process where torch owns the device first (as bench.py)."""
    import torch
    import tamcmc_amd as accel_mod
    from oracle import pyoracle as orc
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    for kind, grid, scale in DEVICE_CASES:
        case = D.power_case(orc, kind, grid, scale)
        P, T, n = case["P"], case["T"], len(case["P"])
        with open_accel(accel_mod, case) as acc:
            L, st, g = acc.eval_batch(P, T, grad=True)
            assert np.all(st == 0) and np.all(np.isfinite(g))
            dP, dT = torch.from_numpy(np.ascontiguousarray(P)).to(dev), torch.from_numpy(np.ascontiguousarray(T)).to(dev)

            def fresh():
                return (torch.full((n,), 7.0, dtype=torch.float64, device=dev), torch.full((n, acc.Nvars), 7.0, dtype=torch.float64, device=dev),
                        torch.full((n,), -9, dtype=torch.int32, device=dev))

            # without a status buffer, then with one
            dL, dG, dS = fresh()
            torch.cuda.synchronize()
            acc.eval_batch_device(n, dP.data_ptr(), dT.data_ptr(), dL.data_ptr(), dG.data_ptr(), 0)
            acc.synchronize()
            assert same_bits(dL.cpu().numpy(), L) and same_bits(dG.cpu().numpy(), g), (case["tag"], "no status buffer")
            assert np.all(dS.cpu().numpy() == -9)
            dL, dG, dS = fresh()
            torch.cuda.synchronize()
            acc.eval_batch_device(n, dP.data_ptr(), dT.data_ptr(), dL.data_ptr(), dG.data_ptr(), dS.data_ptr())
            acc.synchronize()
            assert same_bits(dL.cpu().numpy(), L) and same_bits(dG.cpu().numpy(), g) and np.array_equal(dS.cpu().numpy(), st), case["tag"]
            # right behind a likelihood-only device call on the same context, nothing waited for in between
            dL0 = torch.full((n,), 5.0, dtype=torch.float64, device=dev)
            dL, dG, dS = fresh()
            torch.cuda.synchronize()
            acc.eval_batch_device(n, dP.data_ptr(), dT.data_ptr(), dL0.data_ptr(), 0, 0)
            acc.eval_batch_device(n, dP.data_ptr(), dT.data_ptr(), dL.data_ptr(), dG.data_ptr(), dS.data_ptr())
            acc.synchronize()
            L0, st0 = acc.eval_batch(P, T)
            assert same_bits(dL0.cpu().numpy(), L0), (case["tag"], "likelihood-only call")
            assert same_bits(dL.cpu().numpy(), L) and same_bits(dG.cpu().numpy(), g) and np.array_equal(dS.cpu().numpy(), st), \
                (case["tag"], "gradient call behind a likelihood-only call")
    print("device gradient path ok")


def test_device_entry_with_gradient():
    """D: tamcmc_eval_batch_device with d_grad set (one fused and one tiled case of part A) equals eval_batch(grad=True) bit
    for bit in logL, status and every gradient entry: without and with a status buffer, and right behind a
    likelihood-only device call on the same context."""
    in_torch_process("test_data_values_gpu", "_device_grad_check", "device gradient path ok")
