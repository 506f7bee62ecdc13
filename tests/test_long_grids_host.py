"""The cases of the long-grid suite (tests/longgrids.py) checked on the CPU: the oracle evaluates every chain of every
case (status 0, a finite positive truth model) -- the GPU tests assert that again instead of selecting -- the restated
geometry rules put every grid on the intended side of its threshold, and the windows of the 8193-unit cases span the
numbers of gradient tiles they are meant to span."""
import numpy as np
import pytest

import edgecases as E
import longgrids as G


def test_restated_rules_at_their_thresholds():
    # tm_tiles: 8-unit tiles from 70 units on; the balancer's slack D = tiles * 8 - units
    assert [G.tiles_of(u) for u in (4, 5, 69, 70, 4095, 4096, 4097, 8192, 8193)] == [1, 5, 12, 9, 512, 512, 513, 1024, 1025]
    assert 512 * 8 - 4095 == 1 and 512 * 8 - 4096 == 0
    assert G.balances(4095, 512, 1) and not G.balances(4096, 512, 1) and not G.balances(4097, 513, 1) and not G.balances(4095, 512, 0)
    assert G.balances(4096, 513, 1) and not G.balances(4097, 1024, 1)      # (slack by hand: the unit bound alone refuses)
    assert G.balances(8184, 1024, 1) is False and G.balances(4000, 1024, 1) and not G.balances(4000, 1025, 1)
    # the tail rule: 7124 units are the last grid whose gradient launch ranks its tiles
    assert G.grad_geometry(7124) == (1024, 757, 8, 4) and G.grad_geometry(7125) == (1025, 757, 8, 4)
    assert all(G.grad_geometry(u)[0] <= 1024 for u in range(7000, 7125)) and all(G.grad_geometry(u)[0] > 1024 for u in range(7125, 7200))
    assert G.grad_geometry(7124, equal_cost=1) == (891, 0, 0, 0) and G.grad_geometry(69) == (12, 0, 0, 0)
    # every unit lies in the tile the rule names, tiles in order, none longer than 8 units
    for u in (4095, 7124, 7125, 8193):
        tiles = G.grad_geometry(u)[0]
        t = np.array([G.grad_tile_of_unit(u, k) for k in range(u)])
        assert t[0] == 0 and t[-1] == tiles - 1 and np.all(np.diff(t) >= 0) and np.all(np.diff(t) <= 1)
        assert np.bincount(t).max() == 8 and np.bincount(t)[-2] == 4
    # the generalised LDS sum is the edge suite's at the edge suite's tile counts (its asserts stay where they are)
    for Nx in (3000, 20000, 35000):
        w = G.W.layout(2, 2, Nmax=5, Nx=Nx)
        assert E.backward_lds_bytes(w, 17) == G.backward_lds_bytes(w, 17, E.grad_tiles(Nx))
    w = G.W.layout(2, 2, Nmax=5, Nx=3000)
    assert G.backward_lds_bytes(w, 17, 1001) - G.backward_lds_bytes(w, 17, 1) == 4000
    assert G.backward_lds_bytes(w, 17, 10) == G.backward_lds_bytes(w, 17, 11) == G.backward_lds_bytes(w, 17, 9) + 8


def test_gradient_geometry_accessor_is_exported(accel_mod):
    """tamcmc_ctx_geometry_grad: what the GPU tests read the gradient launch's tile count from."""
    lib = accel_mod.load_library()
    assert hasattr(lib, "tamcmc_ctx_geometry_grad") and "tamcmc_ctx_geometry_grad" in accel_mod.capi.EXPORTS
    assert lib.tamcmc_ctx_geometry_grad(None, None, None) == accel_mod.capi.E_INVALID      # no context: no device touched


@pytest.mark.parametrize("name", list(G.CASES))
def test_long_grid_case_stands_where_it_is_meant_to(orc, name):
    case = G.build(orc, name)
    c = G.CASES[name]
    assert case["Nx"] == G.Nx_of(c["units"], c["exact"]) and G.units_of(case["Nx"]) == c["units"]
    assert (case["Nx"] % 512 == 0) == c["exact"] and case["w"]["x"].size == case["Nx"]
    assert case["truth_ok"], name                               # status 0, finite and positive in every bin
    n = case["n_eval"]
    assert len(case["P"]) == n + 1 and len(set(case["T"].tolist())) == n + 1 and np.all(case["T"] > 1.0)
    L, st = orc.generate_batch(2, case["w"]["plength"], case["w"]["x"], case["y"], case["P"], case["T"])
    assert np.all(st == 0) and np.all(np.isfinite(L)), (name, st)
    # the restated rules put the grid on its side of the threshold
    tl, tg, bal_l, bal_g = G.expected_geometry(name)
    side = c["side"]
    if "tiles" in side:
        assert tl == side["tiles"] and (tl <= G.ORDER_MAX) == (side["tiles"] == 1024)
    if "tiles_grad" in side:
        assert tg == side["tiles_grad"] and (tg <= G.ORDER_MAX) == (side["tiles_grad"] == 1024) and tl < G.ORDER_MAX
    if "balanced" in side:
        assert bal_l == bal_g == side["balanced"] and tl <= G.ORDER_MAX and tg <= G.ORDER_MAX
        ec = int(c["env"]["TAMCMC_EQUAL_COST"])
        slack = tl * G.TILE_MAXU - c["units"]
        assert {4095: slack == 1, 4096: slack == 0, 4097: slack == 7 and c["units"] > G.EQ_MAXU}[c["units"]]
        assert tg == (tl if ec else G.grad_geometry(c["units"])[0]) and (ec or tg > tl)
    assert tl < G.GRID_Y_MAX and tg < G.GRID_Y_MAX              # (item 3 is reached by hand only: part C)


def test_both_sides_of_every_default_threshold_are_cases():
    sides = {(c["units"], c["env"].get("TAMCMC_EQUAL_COST")) for c in G.CASES.values() if c["item"] == 1}
    assert sides == {(u, ec) for u in (4095, 4096, 4097) for ec in ("0", "1")}
    assert {c["exact"] for c in G.CASES.values() if c["units"] in (4096, 8192)} == {False, True}
    assert {c["side"].get("tiles") for c in G.CASES.values() if c["item"] == 2} >= {1024, 1025}
    assert {c["side"].get("tiles_grad") for c in G.CASES.values() if c["item"] == 2} >= {1024, 1025}
    assert any(c["env"].get("TAMCMC_PRIO") == "1" for c in G.CASES.values() if c["item"] == 2)
    assert sorted((t - 1) & 7 for t in G.HAND_TILES) == [0, 6, 7] and G.HAND_TILES[0] == G.GRID_Y_MAX == G.HAND_TILES[1] - 1


def test_windows_span_many_gradient_tiles(orc):
    """Item 5: backward phase 1a sums a multiplet's partials over the tiles its window meets -- at most about six on the
    grids of the other suites."""
    case = G.build(orc, G.WINDOW_CASE)
    tiles = G.grad_geometry(case["units"])[0]
    spans = []
    for k in range(case["n_eval"]):
        for lo, hi in G.l0_windows(orc, case, case["P"][k]):
            spans.append(G.grad_tile_of_unit(case["units"], (hi - 1) >> 9) - G.grad_tile_of_unit(case["units"], lo >> 9) + 1)
    print(f"{G.WINDOW_CASE}: the l = 0 windows span {min(spans)} ... {max(spans)} of {tiles} gradient tiles")
    assert max(spans) >= 20 and max(spans) < tiles
    wide = G.build(orc, G.WIDE_CASE)
    assert wide["units"] == case["units"] and wide["n_eval"] == 1
    assert float(wide["P"][0, G.W.split(wide["w"])["cfg"]]) == 10000.0
    for lo, hi in G.l0_windows(orc, wide, wide["P"][0]):
        assert (lo, hi) == (0, wide["Nx"])
        assert G.grad_tile_of_unit(wide["units"], (hi - 1) >> 9) - G.grad_tile_of_unit(wide["units"], lo >> 9) + 1 == tiles


@pytest.mark.parametrize("layout", G.SHORT_LAYOUTS)
def test_short_cases_and_their_lds_points(orc, layout):
    case = G.short_case(orc, layout)
    w = case["w"]
    nv = int(w["index_to_relax"].size)
    assert case["truth_ok"] and G.units_of(case["Nx"]) == 5 and G.tiles_of(5) == 5
    assert (nv, int(w["plength"][0]) * (int(w["plength"][1]) + 1)) == {"nine": (26, 9), "star": (44, 21)}[layout]
    ans = G.short_oracle(orc, case)
    assert np.all(ans["st"] == 0) and np.all(ans["gst"] == 0) and np.all(np.isfinite(ans["L"])) and np.all(np.isfinite(ans["g"]))
    assert np.all(np.isfinite(ans["models"])) and np.all(ans["models"] > 0)
    t_star, t_aux, t_attr = G.lds_points(w, nv)
    print(f"short {layout}: tables without tiles {G.backward_lds_bytes(w, nv, 0) - 8} bytes, records {G.records_bytes(w)}; "
          f"T* = {t_star}, records staged up to {t_aux} tiles, attribute path above {t_attr}")
    assert 5 < t_attr < t_aux < t_star < G.GRID_Y_MAX and t_star + 1 <= G.TILES_ENV_MAX
    assert G.backward_lds_bytes(w, nv, t_star) <= G.BW_LDS_MAX < G.backward_lds_bytes(w, nv, t_star + 1)
    assert G.backward_lds_bytes(w, nv, t_aux) + G.records_bytes(w) <= G.BW_AUX_STAGED < G.backward_lds_bytes(w, nv, t_aux + 1) + G.records_bytes(w)
    # one variable fewer fits at T* + 1: the earlier list of the refusal test
    assert G.backward_lds_bytes(w, nv - 1, t_star + 1) <= G.BW_LDS_MAX
    if layout == "star":
        assert G.backward_lds_bytes(w, nv, 0) - 8 == 15224          # the sum is 15 224 + 4 bytes per tile (rounded up to two tiles)
