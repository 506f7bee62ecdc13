"""Directed edge suite of the three launches (likelihood: specialised body; likelihood with model rows: generic body;
gradient launch + backward kernel) against the oracle -- tests/edgecases.py builds the cases, tests/test_edges_host.py
proves on the CPU that they hit their targets.

  A  327 grids: every unit count 1 ... 80, then 95-97, 128, 195-197, each at 512u - 1, 512u, 512u + 1 bins (a global id with
     l = 0 ... 2, 4 chains), and an asymmetric chi_square case and local id 11 at the unit counts around the thresholds of
     the tile rules (4/5, 9/10, 69/70 ... 73, 196); all contexts of a tile mode then form ONE fit group (330 members,
     three of them without chains), which must return its members' own results bit for bit;
  B  a window edge on, before and behind every unit boundary of a 100 000-bin and a 30 000-bin grid (and Nx itself, ten row
     boundaries, one-bin windows, the clamps, adjacent doubles of fc on either side of a step of imin / imax, chains that
     do not evaluate among healthy ones): 1705 and 598 chains in one batch each, every healthy chain also alone;
  C  16 ... 256 multiplets (ids 2 and 13); 255 and 256 multiplets have no gradient (refused by set_vars), 258 no context.

Tolerances as everywhere in the suite: status codes identical, logL 1e-10 relative, model rows 1e-12 per bin, gradient
entries 1e-10 |g_k| + 3e-14 S_k (tests/gradcheck.py).  A and B run with tiles of equal length and of equal cost.

Observed (MI355X; every test prints its own figures): A logL 2.1e-15, model bin 8.8e-15, gradient entries 1.2e-14 S_k (5.1e-12
relative); B logL 4.2e-14, model bin 7.6e-16, gradient entries 3.6e-11 S_k, the worst on an entry without
cancellation (S_k = |g_k|, so this is its relative error: a third of the 1e-10 bar); C logL 2.1e-15, model bin 1.1e-15,
gradient entries 1.0e-15 S_k.  The file takes 27 s."""
import numpy as np
import pytest

import edgecases as E
import gradcheck
import workloads as W

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("balanced", [0, 1], ids=["equal-length-tiles", "equal-cost-tiles"])


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


class Worst:
    """Largest observed errors of one test (printed; the assertions are made case by case)."""

    def __init__(self):
        self.L = self.M = self.gS = self.gR = 0.0
        self.cases = self.chains = 0

    def line(self, what):
        return (f"{what}: {self.cases} cases, {self.chains} chains; worst logL error {self.L:.2e} relative, model bin {self.M:.2e} "
                f"relative, gradient entry {self.gS:.2e} of its sum|terms| ({self.gR:.2e} relative)")


def check_logL(L, st, ref_L, ref_st, tag, worst, failures):
    """Status codes identical; logL within 1e-10 relative where the oracle evaluates, NaN where it gives NaN."""
    if not np.array_equal(st, ref_st):
        k = np.flatnonzero(st != ref_st)
        failures.append(f"{tag}: status of chain {k[0]} is {st[k[0]]}, oracle {ref_st[k[0]]} ({k.size} chains differ)")
        return False
    good = (ref_st == 0) & np.isfinite(ref_L)
    ok = bool(np.all(np.isnan(L[~good]) == np.isnan(ref_L[~good])))
    if not ok:
        failures.append(f"{tag}: NaN pattern of the chains that do not evaluate differs")
    if np.any(good):
        err = np.abs(L[good] - ref_L[good]) / np.abs(ref_L[good])
        if not np.all(err <= 1e-10):           # (NaN fails too)
            k = np.flatnonzero(good)[int(np.nanargmax(np.where(np.isnan(err), np.inf, err)))]
            failures.append(f"{tag}: logL of chain {k} is {L[k]!r}, oracle {ref_L[k]!r}")
            ok = False
        else:
            worst.L = max(worst.L, float(err.max()))
    return ok


def check_rows(models, ref_models, tag, worst, failures):
    err = np.abs(models - ref_models) / np.abs(ref_models)
    if not np.all(err <= 1e-12):
        r, i = np.unravel_index(int(np.argmax(np.where(np.isnan(err), np.inf, err))), err.shape)
        failures.append(f"{tag}: model row {r} bin {i} is {models[r, i]!r}, oracle {ref_models[r, i]!r}")
        return False
    worst.M = max(worst.M, float(err.max()))
    return True


def check_grad(g, ref, ref_abs, tag, worst, failures):
    try:
        ec, er = gradcheck.assert_grad_entrywise(g, ref, ref_abs, tag=tag)
    except AssertionError as e:
        failures.append(str(e))
        return False
    worst.gS, worst.gR = max(worst.gS, ec), max(worst.gR, er)
    return True


def all_launches(acc, case, ans, worst, failures, tag):
    """eval_batch alone, with model rows, with the gradient -- each against the oracle.  Returns the logL of the first."""
    P, T = case["P"], case["T"]
    L, st = acc.eval_batch(P, T)
    check_logL(L, st, ans["L"], ans["st"], tag + " [likelihood]", worst, failures)
    Lr, str_, rows = acc.eval_batch(P, T, model_rows=ans["rows"])
    if check_logL(Lr, str_, ans["L"], ans["st"], tag + " [model rows]", worst, failures):
        check_rows(rows, ans["models"], tag + " [model rows]", worst, failures)
    Lg, stg, g = acc.eval_batch(P, T, grad=True)
    if check_logL(Lg, stg, ans["L"], ans["st"], tag + " [gradient]", worst, failures):
        assert np.all(ans["gst"] == 0)
        check_grad(g, ans["g"], ans["gabs"], tag + " [gradient]", worst, failures)
    worst.cases += 1
    worst.chains += len(P)
    return L, st


def open_accel(accel_mod, case):
    acc = accel_mod.Accel(case["mid"], case["w"]["plength"], case["w"]["x"], case["y"], sigma_y=case["sigma"],
                          likelihood_case=case["like"])
    acc.set_vars(case["w"]["index_to_relax"])
    return acc


# ---------------------------------------------------------------------------------------------------------------------
@MODES
def test_grid_length_sweep(accel_mod, orc, monkeypatch, balanced):
    """A: every unit count through the thresholds of the tile rules, all launches; then all contexts as one fit group."""
    monkeypatch.setenv("TAMCMC_EQUAL_COST", str(balanced))
    mode = ("equal-length", "equal-cost")[balanced]
    worst, failures, members = Worst(), [], []
    try:
        for kind, Nx in E.sweep_list():
            case = E.sweep_case(orc, kind, Nx)
            ans = E.oracle_answers(orc, ("A", kind, Nx), case)
            assert np.all(ans["st"] == 0) and np.all(np.isfinite(ans["L"])) and np.all(np.isfinite(ans["g"])), case["tag"]
            acc = open_accel(accel_mod, case)
            L, st = all_launches(acc, case, ans, worst, failures, f"{case['tag']} {mode} tiles")
            members.append((acc, case["P"], case["T"], L, st))
        print(worst.line(f"edges A, {mode} tiles"))
        assert not failures, failures[:20]
        # one group of every context of this tile mode, members without chains first, in the middle and last
        for pos, Nx in ((len(members), 20000), (len(members) // 2, 3000), (0, 1000)):
            case = E.sweep_case(orc, "main", Nx)
            n = int(case["w"]["plength"].sum())
            members.insert(pos, (open_accel(accel_mod, case), np.empty((0, n)), np.empty(0), np.empty(0), np.empty(0, dtype=np.int32)))
        assert [k for k, m in enumerate(members) if len(m[1]) == 0] == [0, 164, 329] and len(members) == 330
        with accel_mod.Group([m[0] for m in members]) as grp:
            GL, Gst = grp.eval([m[1] for m in members], [m[2] for m in members])
        for k, m in enumerate(members):
            assert np.array_equal(Gst[k], m[4]) and bits_equal(GL[k], m[3]), (f"group member {k} ({m[0].Nx} bins, {mode} tiles)", GL[k], m[3])
    finally:
        for m in members:
            m[0].close()


# ---------------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("Nx", E.EDGE_GRIDS + E.CLAMP_GRIDS)
def test_window_edge_on_every_unit_boundary(accel_mod, orc, monkeypatch, Nx, balanced):
    """B: the probe's window edge on / one before / one behind every unit boundary, one-bin windows, clamps, adjacent
    doubles, chains that do not evaluate -- all chains of a grid in one batch; rows in blocks of 128 chains."""
    monkeypatch.setenv("TAMCMC_EQUAL_COST", str(balanced))
    mode = ("equal-length", "equal-cost")[balanced]
    case = E.edge_case(orc, Nx)
    ans = E.edge_logL(orc, case)
    chains, P, T, w = case["chains"], case["P"], case["T"], case["w"]
    ok = ans["ok"]
    assert np.array_equal(ans["st"], [r["status"] for r in chains]) and np.all(ans["gst"] == 0)
    worst, failures = Worst(), []

    def name(i):
        r = chains[i]
        return f"B Nx={Nx} chain {i} ({r['kind']} at boundary {r['b']}, window target {r['edge']}={r['v']}) {mode} tiles"

    def first_bad(bad):
        return "; first: " + name(int(np.flatnonzero(bad)[0])) if np.any(bad) else ""

    with accel_mod.Accel(2, w["plength"], case["x"], case["y"]) as acc:
        acc.set_vars(w["index_to_relax"])
        # specialised likelihood body: the whole batch at once
        L, st = acc.eval_batch(P, T)
        bad = (st != ans["st"]) | (ok & ~(np.abs(L - ans["L"]) <= 1e-10 * np.abs(ans["L"])))
        check_logL(L, st, ans["L"], ans["st"], f"B Nx={Nx} {mode} tiles [likelihood]" + first_bad(bad), worst, failures)
        # gradient launch + backward: the whole batch at once
        Lg, stg, g = acc.eval_batch(P, T, grad=True)
        bad = (stg != ans["st"]) | (ok & ~(np.abs(Lg - ans["L"]) <= 1e-10 * np.abs(ans["L"])))
        if check_logL(Lg, stg, ans["L"], ans["st"], f"B Nx={Nx} {mode} tiles [gradient]" + first_bad(bad), worst, failures):
            tol = gradcheck.GRAD_RTOL * np.abs(ans["g"]) + gradcheck.GRAD_COND * ans["gabs"]
            badrow = np.zeros(len(P), dtype=bool)
            badrow[np.flatnonzero(ok)] = np.any(~(np.abs(g[ok] - ans["g"]) <= tol), axis=1)
            check_grad(g[ok], ans["g"], ans["gabs"], f"B Nx={Nx} {mode} tiles [gradient]" + first_bad(badrow), worst, failures)
            share = np.max(np.abs(g[ok] - ans["g"]) / np.maximum(ans["gabs"], 1e-300), axis=1)
            narrow = np.array([chains[i]["c"] < 1.0 for i in np.flatnonzero(ok)])     # one-bin windows, the c = 0 chains
            print(f"edges B, {Nx} bins, {mode} tiles: worst gradient entry of the chains with trunc_c = 20 and more "
                  f"{share[~narrow].max():.2e} of its sum|terms|, of the chains with windows of one or two bins {share[narrow].max():.2e}")
        # generic body: logL and every bin of every chain's model, 128 chains per call
        for i0 in range(0, len(P), 128):
            sl = slice(i0, min(i0 + 128, len(P)))
            rows = np.flatnonzero(ok[sl])
            # (the oracle's rows are computed again in the other tile mode: 1705 rows of 100 000 bins are 1.4 GB to keep)
            _, _, rm = orc.generate_batch(2, w["plength"], case["x"], case["y"], P[sl], T[sl], want_models=True)
            Lr, str_, models = acc.eval_batch(P[sl], T[sl], model_rows=rows)
            bad = np.zeros(len(P), dtype=bool)
            bad[sl] = (str_ != ans["st"][sl]) | (ok[sl] & ~(np.abs(Lr - ans["L"][sl]) <= 1e-10 * np.abs(ans["L"][sl])))
            check_logL(Lr, str_, ans["L"][sl], ans["st"][sl], f"B Nx={Nx} {mode} tiles [model rows]" + first_bad(bad), worst, failures)
            err = np.abs(models - rm[rows]) / np.abs(rm[rows])
            badrow = ~np.all(err <= 1e-12, axis=1)
            if np.any(badrow):
                r = int(np.flatnonzero(badrow)[0])
                i = int(np.argmax(np.where(np.isnan(err[r]), np.inf, err[r])))
                failures.append(f"{name(i0 + int(rows[r]))} [model rows]: bin {i} is {models[r, i]!r}, oracle {rm[rows[r], i]!r} "
                                f"({int(badrow.sum())} rows of this block differ)")
            else:
                worst.M = max(worst.M, float(err.max()))
        # a chain's result does not depend on its neighbours: every healthy chain alone, bit for bit
        alone_bad = []
        for i in np.flatnonzero(ok):
            L1, st1 = acc.eval_batch(P[i:i + 1], T[i:i + 1])
            if st1[0] != 0 or not bits_equal(L1, L[i:i + 1]):
                alone_bad.append(f"{name(int(i))}: alone {L1[0]!r} (status {st1[0]}), in the batch {L[i]!r}")
        if alone_bad:
            failures.append(f"{len(alone_bad)} chains differ alone; first ten: " + " | ".join(alone_bad[:10]))
    worst.cases, worst.chains = 1, len(P)
    print(worst.line(f"edges B, {Nx} bins, {mode} tiles"))
    assert not failures, failures[:20]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mid", E.MULT_IDS)
@pytest.mark.parametrize("Nmax,lmax", E.MULT_SHAPES, ids=[f"{n}x{l + 1}" for n, l in E.MULT_SHAPES])
def test_multiplet_count_edges(accel_mod, orc, mid, Nmax, lmax):
    """C: 16 / 17, 32 / 33, 64 / 65 multiplets (lane groups of the setup kernel's tile pass), 255 and 256 (TM_MAXMULT).

    The backward kernel keeps 45 doubles of tile sums and adjoints, 12 pair values and 12 pair indices per multiplet in
    LDS -- 504 bytes, 126 KB at 256 multiplets -- beside 72 bytes per variable and 12 per parameter; with every entry a
    variable (396 ... 776 of them here) the 255- and 256-multiplet layouts need 159 ... 191 KB, more than the 150 KB of
    dynamic LDS a workgroup can have (160 KB less the static tables).  Their variables are refused by set_vars (E_NOGRAD)
    and their likelihood launches run as before; every layout up to 65 multiplets (at most 73 KB here with the staged
    records) must have its gradient.  The other launchers hold per multiplet 12 bytes of LDS (setup: windows) and
    none (eval), and buffers of n_mult records per chain and tile: no limit below 256."""
    case = E.mult_case(orc, mid, Nmax, lmax)
    ans = E.oracle_answers(orc, ("C", mid, Nmax, lmax), case, rows=[0, 1, 2])
    assert np.all(ans["st"] == 0) and np.all(ans["gst"] == 0) and np.all(np.isfinite(ans["g"]))
    worst, failures = Worst(), []
    w, P, T = case["w"], case["P"], case["T"]
    with accel_mod.Accel(mid, w["plength"], w["x"], case["y"]) as acc:
        assert acc.geometry()["n_multiplets"] == case["n_mult"]
        if case["n_mult"] >= 255:
            with pytest.raises(accel_mod.capi.AccelError) as e:
                acc.set_vars(w["index_to_relax"])
            assert e.value.code == accel_mod.capi.E_NOGRAD
            with pytest.raises(accel_mod.capi.AccelError) as e:       # ... and the context has no variables
                acc.eval_batch(P, T, grad=True)
            assert e.value.code == accel_mod.capi.E_NOVARS
            L, st = acc.eval_batch(P, T)
            check_logL(L, st, ans["L"], ans["st"], case["tag"] + " [likelihood]", worst, failures)
            Lr, str_, rows = acc.eval_batch(P, T, model_rows=ans["rows"])
            if check_logL(Lr, str_, ans["L"], ans["st"], case["tag"] + " [model rows]", worst, failures):
                check_rows(rows, ans["models"], case["tag"] + " [model rows]", worst, failures)
            worst.cases, worst.chains = 1, len(P)
        else:
            acc.set_vars(w["index_to_relax"])
            all_launches(acc, case, ans, worst, failures, case["tag"])
    print(worst.line("edges " + case["tag"]))
    assert not failures, failures


LIMIT_SHAPES = [sh for sh in E.MULT_SHAPES if sh[0] * (sh[1] + 1) >= 255]


@pytest.mark.parametrize("mid", E.MULT_IDS)
@pytest.mark.parametrize("Nmax,lmax", LIMIT_SHAPES, ids=[f"{n}x{l + 1}" for n, l in LIMIT_SHAPES])
def test_gradient_at_the_multiplet_limit(accel_mod, orc, mid, Nmax, lmax):
    """C, gradient launch + backward at 255 and 256 multiplets with variables that fit: 96 of them -- eta, a3, the
    asymmetry, a1 or the inclination pair, the noise block, heights, frequencies and widths spread over the orders.  The
    backward kernel's tables then take 138 ... 143 KB of LDS and its per-multiplet records (88 KB) are read in place."""
    case = E.mult_case(orc, mid, Nmax, lmax)
    w, P, T = case["w"], case["P"], case["T"]
    idx = E.spread_vars(w, 96)
    b = W.split(w)
    assert {b["s"] + 1, b["s"] + 2, b["s"] + 5, b["z"] + 9} <= set(idx.tolist())
    assert E.backward_lds_bytes(w, idx.size) <= E.BW_LDS_MAX
    ref, ref_abs, rL, rst = orc.grad_analytic(mid, w["plength"], w["x"], case["y"], P, T, idx)
    assert np.all(rst == 0) and np.all(np.isfinite(ref))
    worst, failures = Worst(), []
    with accel_mod.Accel(mid, w["plength"], w["x"], case["y"]) as acc:
        acc.set_vars(idx)
        Lg, stg, g = acc.eval_batch(P, T, grad=True)
    if check_logL(Lg, stg, rL, rst, case["tag"] + f" [gradient, {idx.size} variables]", worst, failures):
        check_grad(g, ref, ref_abs, case["tag"] + f" [gradient, {idx.size} variables]", worst, failures)
    worst.cases, worst.chains = 1, len(P)
    print(worst.line(f"edges {case['tag']}, {idx.size} variables"))
    assert not failures, failures


@pytest.mark.parametrize("mid", E.MULT_IDS)
def test_every_entry_a_variable_near_the_lds_limit(accel_mod, orc, mid):
    """C, all launches at 180 multiplets with every entry a variable (311 / 488 variables, 115 / 130 KB of tables): the
    largest of the suite's layouts whose full gradient fits; records read in place, and for id 13 more variables than
    the backward kernel has staging threads."""
    case = E.mult_case(orc, mid, *E.NEAR_LIMIT_SHAPE)
    ans = E.oracle_answers(orc, ("C", mid) + E.NEAR_LIMIT_SHAPE, case, rows=[0, 1, 2])
    assert np.all(ans["st"] == 0) and np.all(ans["gst"] == 0) and np.all(np.isfinite(ans["g"]))
    worst, failures = Worst(), []
    with open_accel(accel_mod, case) as acc:
        all_launches(acc, case, ans, worst, failures, case["tag"])
    print(worst.line("edges " + case["tag"] + f", {case['w']['index_to_relax'].size} variables"))
    assert not failures, failures


def test_variable_count_at_the_lds_bound(accel_mod, orc):
    """256 multiplets: the largest number of variables whose tables fit is accepted and its gradient is the oracle's; one
    more is refused (E_NOGRAD) and the context keeps the variables it had."""
    case = E.mult_case(orc, 2, 64, 3)
    w, P, T = case["w"], case["P"], case["T"]
    full = w["index_to_relax"]
    n = max(k for k in range(1, full.size) if E.backward_lds_bytes(w, k) <= E.BW_LDS_MAX)
    assert 200 < n < full.size - 1 and E.backward_lds_bytes(w, n + 1) > E.BW_LDS_MAX
    ref, ref_abs, rL, rst = orc.grad_analytic(2, w["plength"], w["x"], case["y"], P, T, full[:n])
    assert np.all(rst == 0)
    worst, failures = Worst(), []
    with accel_mod.Accel(2, w["plength"], w["x"], case["y"]) as acc:
        acc.set_vars(full[:n])
        L1, st1, g1 = acc.eval_batch(P, T, grad=True)
        if check_logL(L1, st1, rL, rst, f"{n} variables [gradient]", worst, failures):
            check_grad(g1, ref, ref_abs, f"{n} variables [gradient]", worst, failures)
        with pytest.raises(accel_mod.capi.AccelError) as e:
            acc.set_vars(full[:n + 1])
        assert e.value.code == accel_mod.capi.E_NOGRAD
        L2, st2, g2 = acc.eval_batch(P, T, grad=True)
        assert np.array_equal(st1, st2) and bits_equal(L1, L2) and bits_equal(g1, g2)
    worst.cases, worst.chains = 1, len(P)
    print(worst.line(f"edges C, 256 multiplets, {n} variables (one more is refused)"))
    assert not failures, failures


def test_more_than_256_multiplets_are_refused(accel_mod, orc):
    Nmax, lmax = E.MULT_REFUSED
    w = W.layout(2, lmax, Nmax=Nmax, Nx=20000)
    with pytest.raises(accel_mod.capi.AccelError) as e:
        accel_mod.Accel(2, w["plength"], w["x"], np.ones(20000))
    assert e.value.code == accel_mod.capi.E_INVALID
