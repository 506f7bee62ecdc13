"""Long grids: all three launches (likelihood, gradient launch, backward kernel) and the fit group on either side of every
point between 1.2e6 bins and the documented limit of Nx at which the library changes behaviour -- tests/longgrids.py
lists the points and builds the cases, tests/test_long_grids_host.py proves on the CPU that each case stands where it is
meant to stand, and every test here asserts that again through the library's own accessors (Accel.geometry(): tiles and
tiles_grad) before it looks at a result.

  B  2.1e6 ... 4.2e6 bins at the default geometry: 4095 / 4096 / 4097 units with tiles of equal length and of equal cost,
     1024 / 1025 tiles in the likelihood launch (8192 / 8193 units) and in the gradient launch (7124 / 7125 units), a
     window that spans all 1178 gradient tiles;
  C  2560 bins with tile counts given by hand: 65535 / 65536 / 70001 likelihood tiles (the chain-major fallback of the
     launch), and gradient tile counts at the three LDS switches of the backward kernel -- the 48 KB attribute path, the
     100 KB staging switch, and T*, the largest count tamcmc_ctx_set_vars accepts;
  D  one fit group of a 4.2e6-bin member and a 65536-tile member.

Bars as everywhere in the suite: status codes identical to the oracle's, logL 1e-10 relative (test_parity_gpu.check_logL),
model rows 1e-12 per bin, gradient entries 1e-10 |g_k| + 3e-14 S_k (tests/gradcheck.py); a repeated call, a chain evaluated in
a smaller batch and a group member give the same bits; equal-cost and equal-length tiles agree to 1e-10 of a gradient
row's largest entry (as tests/test_fuzz_gpu.py asks).  No case is selected by its status: np.all(status == 0) is asserted.

Observed (MI355X; every test prints its own figures): B logL 8.9e-16, gradient entries 6.4e-16 S_k (whole-grid windows;
8.5e-17 S_k for the star), equal-cost against equal-length tiles 1.4e-16 of the row's largest entry; C logL 1.5e-15, gradient
entries 8.7e-16 S_k at every tile count, T* = 34 593 (benchmark layout, 44 variables) and 36 489 (9 multiplets, 26
variables).  The file takes 37 s, all but a second of it the CPU oracle (2 s per 2.1e6-bin grid, 4 s per 4.2e6-bin grid,
8 s for the whole-grid windows)."""
import time

import numpy as np
import pytest

import gradcheck
import longgrids as G
from test_parity_gpu import RTOL_MODEL, check_logL

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def set_env(monkeypatch, env):
    for k in ("TAMCMC_TILES", "TAMCMC_TILES_GRAD", "TAMCMC_EQUAL_COST", "TAMCMC_PRIO", "TAMCMC_ORDER", "TAMCMC_TAIL",
              "TAMCMC_COST", "TAMCMC_COST_GRAD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def open_accel(accel_mod, case, idx=None):
    w = case["w"]
    acc = accel_mod.Accel(case["mid"], w["plength"], w["x"], case["y"])
    try:
        acc.set_vars(w["index_to_relax"] if idx is None else idx)
    except Exception:
        acc.close()
        raise
    return acc


def figures(L, ref_L, g, ref_g, ref_abs):
    eL = float(np.max(np.abs(L - ref_L) / np.abs(ref_L)))
    nz = ref_abs > 0
    eg = float(np.max(np.abs(g - ref_g)[nz] / ref_abs[nz]))
    return eL, eg


_GRAD_EQUAL_LENGTH = {}      # grid -> gradient of the equal-length tiles (the EQUAL_COST=0 case of item 1 runs first)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.CASES))
def test_long_grid_at_the_default_geometry(accel_mod, orc, monkeypatch, name):
    """B: likelihood launch, gradient launch and backward kernel against the oracle; the same bits from a second call and
    from a batch with one chain more."""
    t0 = time.time()
    case = G.build(orc, name)
    ans = G.oracle_answers(orc, case)
    t_oracle = time.time() - t0
    assert case["truth_ok"] and np.all(ans["st"] == 0) and np.all(np.isfinite(ans["L"])) and np.all(np.isfinite(ans["g"]))
    n, P, T, w = case["n_eval"], case["P"], case["T"], case["w"]
    tl, tg, bal_l, bal_g = G.expected_geometry(name)
    set_env(monkeypatch, case["env"])
    with open_accel(accel_mod, case) as acc:
        geo = acc.geometry()
        # the side of the threshold, by the library's own account
        assert (geo["tiles"], geo["tiles_grad"]) == (tl, tg), (name, geo)
        assert geo["bins_per_tile"] == 512 * G.likelihood_max_units(case["units"], tl, int(case["env"].get("TAMCMC_EQUAL_COST", "0")))
        assert geo["bins_per_tile_grad"] == 512 * G.TILE_MAXU
        for key in ("tiles", "tiles_grad"):
            if key in case["side"]:
                assert geo[key] == case["side"][key] and geo[key] in (G.ORDER_MAX, G.ORDER_MAX + 1)
        L, st = acc.eval_batch(P[:n], T[:n])
        assert acc.geometry()["tiles"] == tl
        Lg, stg, g = acc.eval_batch(P[:n], T[:n], grad=True)
        # status, logL of both launches, gradient entry by entry
        assert np.array_equal(st, ans["st"]) and np.array_equal(stg, ans["st"]) and np.all(st == 0)
        eL, eg = figures(L, ans["L"], g, ans["g"], ans["gabs"])
        eLg = float(np.max(np.abs(Lg - ans["L"]) / np.abs(ans["L"])))
        print(f"long grids {name}: {case['Nx']} bins, {tl} / {tg} tiles, balanced {bal_l} / {bal_g}; logL error {eL:.2e} "
              f"(gradient path {eLg:.2e}) relative, worst gradient entry {eg:.2e} of its sum|terms|", flush=True)
        check_logL(L, ans["L"])
        check_logL(Lg, ans["L"])
        gradcheck.assert_grad_entrywise(g, ans["g"], ans["gabs"], tag=name)
        # item 6: a second identical call gives the same bits
        L2, st2 = acc.eval_batch(P[:n], T[:n])
        Lg2, stg2, g2 = acc.eval_batch(P[:n], T[:n], grad=True)
        assert np.array_equal(st2, st) and bits_equal(L2, L), (name, L, L2)
        assert np.array_equal(stg2, stg) and bits_equal(Lg2, Lg) and bits_equal(g2, g), name
        # a chain's result does not depend on the batch: one chain more, the first n the same bits
        L3, st3 = acc.eval_batch(P, T)
        Lg3, stg3, g3 = acc.eval_batch(P, T, grad=True)
        assert np.array_equal(st3[:n], st) and bits_equal(L3[:n], L), (name, L, L3)
        assert np.array_equal(stg3[:n], stg) and bits_equal(Lg3[:n], Lg) and bits_equal(g3[:n], g), name
        assert np.all(st3 == 0) and np.all(stg3 == 0) and np.all(np.isfinite(L3)) and np.all(np.isfinite(g3))
    if "balanced" in case["side"]:
        # equal-cost tiles give other partial sums, the same gradient to rounding
        if case["env"]["TAMCMC_EQUAL_COST"] == "0":
            _GRAD_EQUAL_LENGTH[case["key"]] = g
        else:
            g0 = _GRAD_EQUAL_LENGTH.get(case["key"])
            if g0 is None:                                      # (this case selected alone: evaluate the other mode now)
                set_env(monkeypatch, dict(case["env"], TAMCMC_EQUAL_COST="0"))
                with open_accel(accel_mod, case) as acc:
                    _, _, g0 = acc.eval_batch(P[:n], T[:n], grad=True)
            d = float(np.max(np.abs(g - g0) / np.max(np.abs(g0), axis=1, keepdims=True)))
            print(f"long grids {name}: equal-cost against equal-length tiles {d:.2e} of the row's largest entry")
            assert d <= 1e-10, (name, d)
    print(f"long grids {name}: {time.time() - t0:.1f} s, {t_oracle:.1f} s of them the oracle (shared by the cases of a grid)")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", G.HAND_TILES)
def test_more_likelihood_tiles_than_the_launch_grid_has_rows(accel_mod, orc, monkeypatch, tiles):
    """C, item 3: above 65535 tiles the eval launch is chain-major with the slot rotation.  5 units under 65535, 65536
    and 70001 tiles: the first five tiles hold a unit each, the rest are empty, and the finalize sums all of them."""
    case = G.short_case(orc, "nine")
    ans = G.short_oracle(orc, case)
    assert case["truth_ok"] and np.all(ans["st"] == 0)
    P, T = case["P"], case["T"]
    set_env(monkeypatch, {})
    with open_accel(accel_mod, case) as acc:
        assert acc.geometry()["tiles"] == 5
        Ld, std = acc.eval_batch(P, T)
    out = {}
    for order in (None, "1"):
        set_env(monkeypatch, dict({"TAMCMC_TILES": str(tiles)}, **({"TAMCMC_ORDER": order} if order else {})))
        with open_accel(accel_mod, case) as acc:
            L, st = acc.eval_batch(P, T)
            assert acc.geometry()["tiles"] == tiles and acc.geometry()["tiles_grad"] == 5
            Lr, str_, rows = acc.eval_batch(P, T, model_rows=ans["rows"])
            L2, st2 = acc.eval_batch(P, T)
            L1, st1 = acc.eval_batch(P[1:2], T[1:2])
        assert np.array_equal(st, ans["st"]) and np.array_equal(str_, ans["st"]) and np.all(st == 0)
        check_logL(L, ans["L"])
        check_logL(Lr, ans["L"])
        assert np.max(np.abs(rows - ans["models"]) / ans["models"]) <= RTOL_MODEL
        assert np.array_equal(st2, st) and bits_equal(L2, L), (tiles, order, L, L2)
        assert st1[0] == 0 and bits_equal(L1, L[1:2])
        out[order] = L
    # the launch order does not change a bit; the default geometry cuts the 5 units alike but sums the tiles in another
    # tree (lane-strided over all tiles): agreement to the bar of the oracle comparison, not bit for bit
    assert bits_equal(out[None], out["1"])
    check_logL(Ld, ans["L"])
    assert np.array_equal(std, ans["st"])
    assert np.max(np.abs(out[None] - Ld) / np.abs(Ld)) <= 1e-10
    print(f"long grids C: {tiles} likelihood tiles on 5 units, logL error {np.max(np.abs(out[None] - ans['L']) / np.abs(ans['L'])):.2e} relative "
          f"(default geometry {np.max(np.abs(Ld - ans['L']) / np.abs(ans['L'])):.2e})")


def _accepts(accel_mod, monkeypatch, case, tiles, idx=None):
    """Whether tamcmc_ctx_set_vars accepts the variables under TAMCMC_TILES_GRAD = tiles (context and set_vars only)."""
    set_env(monkeypatch, {"TAMCMC_TILES_GRAD": str(tiles)})
    w = case["w"]
    with accel_mod.Accel(case["mid"], w["plength"], w["x"], case["y"]) as acc:
        assert acc.geometry()["tiles_grad"] == tiles
        try:
            acc.set_vars(w["index_to_relax"] if idx is None else idx)
        except accel_mod.capi.AccelError as e:
            assert e.code == accel_mod.capi.E_NOGRAD, e
            return False
    return True


def _gradient_under(accel_mod, orc, monkeypatch, case, tiles, tag):
    ans = G.short_oracle(orc, case)
    set_env(monkeypatch, {"TAMCMC_TILES_GRAD": str(tiles)})
    with open_accel(accel_mod, case) as acc:
        assert acc.geometry()["tiles_grad"] == tiles
        Lg, stg, g = acc.eval_batch(case["P"], case["T"], grad=True)
        Lg2, stg2, g2 = acc.eval_batch(case["P"], case["T"], grad=True)
    assert np.array_equal(stg, ans["st"]) and np.all(stg == 0)
    check_logL(Lg, ans["L"])
    ec, _ = gradcheck.assert_grad_entrywise(g, ans["g"], ans["gabs"], tag=tag)
    assert np.array_equal(stg2, stg) and bits_equal(Lg2, Lg) and bits_equal(g2, g), tag
    return ec


@pytest.mark.parametrize("layout", G.SHORT_LAYOUTS)
def test_gradient_tile_count_at_the_lds_bound(accel_mod, orc, monkeypatch, layout):
    """C, item 4: the backward kernel keeps the first unit of every gradient tile in LDS, 4 bytes per tile beside the
    tables of the layout.  tamcmc_ctx_set_vars accepts up to T* tiles -- the count the restated sum predicts, found
    here by bisection -- the gradient at T* is the oracle's, and T* + 1 tiles are refused with the earlier variables kept."""
    case = G.short_case(orc, layout)
    w = case["w"]
    full = w["index_to_relax"]
    t_star = G.lds_points(w, full.size)[0]
    t0 = time.time()
    lo, hi = 5, G.TILES_ENV_MAX                                     # accepted (the default count) / refused
    assert _accepts(accel_mod, monkeypatch, case, lo) and not _accepts(accel_mod, monkeypatch, case, hi)
    probes = 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _accepts(accel_mod, monkeypatch, case, mid):
            lo = mid
        else:
            hi = mid
        probes += 1
    assert lo == t_star, (layout, lo, t_star)
    # ... and flips there only: counts on either side of the bound, near and far
    for t in (t_star - 3, t_star - 2, t_star - 1, 2 * t_star // 3, 1000):
        assert _accepts(accel_mod, monkeypatch, case, t), t
    for t in (t_star + 1, t_star + 2, t_star + 3, t_star + 1001, 2 * t_star, G.GRID_Y_MAX, G.GRID_Y_MAX + 1):
        assert not _accepts(accel_mod, monkeypatch, case, t), t
    t_bisect = time.time() - t0
    ec = _gradient_under(accel_mod, orc, monkeypatch, case, t_star, f"{layout} at T* = {t_star} gradient tiles")
    # one tile more: refused, the earlier list stays in force and its gradient is still the oracle's
    fewer = full[:-1]
    ans = G.short_oracle(orc, case, idx=fewer)
    set_env(monkeypatch, {"TAMCMC_TILES_GRAD": str(t_star + 1)})
    with open_accel(accel_mod, case, idx=fewer) as acc:
        with pytest.raises(accel_mod.capi.AccelError) as e:
            acc.set_vars(full)
        assert e.value.code == accel_mod.capi.E_NOGRAD and acc.Nvars == fewer.size
        Lg, stg, g = acc.eval_batch(case["P"], case["T"], grad=True)
    assert g.shape == (3, fewer.size) and np.array_equal(stg, ans["st"]) and np.all(stg == 0)
    check_logL(Lg, ans["L"])
    gradcheck.assert_grad_entrywise(g, ans["g"], ans["gabs"], tag=f"{layout} at T* + 1 with the earlier variables")
    print(f"long grids C: {layout} layout ({full.size} variables): T* = {t_star} gradient tiles ({probes} contexts, {t_bisect:.1f} s); "
          f"worst gradient entry at T* {ec:.2e} of its sum|terms|")


@pytest.mark.parametrize("layout", G.SHORT_LAYOUTS)
@pytest.mark.parametrize("switch", ["records-staged-100KB", "attribute-48KB"])
def test_gradient_tile_count_at_the_lds_switches(accel_mod, orc, monkeypatch, layout, switch):
    """C, item 4: the largest gradient tile count at which the backward kernel still stages the per-multiplet records in
    LDS (tables + records within 100 KB) and the count above it (records read in place); the largest count that stays
    within 48 KB of dynamic LDS and the one above it (the launch raises the kernel's limit first)."""
    case = G.short_case(orc, layout)
    nv = int(case["w"]["index_to_relax"].size)
    t = G.lds_points(case["w"], nv)[1 if switch.startswith("records") else 2]
    for tiles in (t, t + 1):
        ec = _gradient_under(accel_mod, orc, monkeypatch, case, tiles, f"{layout} at {tiles} gradient tiles ({switch})")
        print(f"long grids C: {layout} layout at {tiles} gradient tiles ({switch}): worst gradient entry {ec:.2e} of its sum|terms|")


# ---------------------------------------------------------------------------------------------------------------------
def test_fit_group_of_a_long_member_and_a_many_tile_member(accel_mod, orc, monkeypatch):
    """D: a 4.2e6-bin member (1025 tiles: unranked) and a 2560-bin member created under TAMCMC_TILES=65536 (chain-major
    inside the group's 1-D launch) in one group: every chain equals its member's own eval_batch bit for bit."""
    long_case, short = G.build(orc, G.WINDOW_CASE), G.short_case(orc, "nine")
    set_env(monkeypatch, {})
    a_long = open_accel(accel_mod, long_case)
    set_env(monkeypatch, {"TAMCMC_TILES": str(G.GRID_Y_MAX + 1)})
    a_short = open_accel(accel_mod, short)
    set_env(monkeypatch, {})
    try:
        n = long_case["n_eval"]
        Pl, Tl, Ps, Ts = long_case["P"][:n], long_case["T"][:n], short["P"], short["T"]
        solo = [a_long.eval_batch(Pl, Tl), a_short.eval_batch(Ps, Ts)]
        assert a_long.geometry()["tiles"] == 1025 and a_short.geometry()["tiles"] == G.GRID_Y_MAX + 1
        assert all(np.all(s[1] == 0) for s in solo)
        check_logL(solo[0][0], G.oracle_answers(orc, long_case)["L"])
        check_logL(solo[1][0], G.short_oracle(orc, short)["L"])
        for members, Ps_, Ts_, want in (((a_long, a_short), [Pl, Ps], [Tl, Ts], solo), ((a_short, a_long), [Ps, Pl], [Ts, Tl], solo[::-1])):
            with accel_mod.Group(list(members)) as grp:
                GL, Gst = grp.eval(Ps_, Ts_)
                grp.begin(Ps_, Ts_)
                BL, Bst = grp.end()
            for k in range(2):
                assert np.array_equal(Gst[k], want[k][1]) and bits_equal(GL[k], want[k][0]), (k, GL[k], want[k][0])
                assert np.array_equal(Bst[k], want[k][1]) and bits_equal(BL[k], want[k][0]), (k, BL[k], want[k][0])
    finally:
        a_long.close()
        a_short.close()
