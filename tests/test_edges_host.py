"""The builders of the edge suite (tests/edgecases.py) checked against the oracle on the CPU: every chain of part B hits
its target window exactly, evaluates with the expected status, and would show one mislaid bin at its edge in logL
(the teeth condition); no case kind is empty; the grid lengths of part A and the multiplet counts of part C are the
ones that cross the thresholds of the tile rules and lane groups."""
import collections

import numpy as np
import pytest

import edgecases as E


def test_sweep_lengths_cross_every_threshold(orc):
    main = E.lengths(E.SWEEP_UNITS)
    assert len(main) == 261 and main[0] == 511 and main[-1] == 512 * 197 + 1
    units = {(Nx + 511) // 512 for Nx in main}
    assert set(range(1, 82)) <= units and {4, 5, 9, 10, 69, 70, 196} <= units
    assert all(512 * u in main and 512 * u - 1 in main and 512 * u + 1 in main for u in range(1, 81))
    # tail shaping (grids of 70 units or more): every remainder of the short tiles' share mod 4 is met
    rests = {(u - 8 * ((u * 85 // 100 + 4) // 8)) % 4 for u in units if u >= 70}
    assert rests == {0, 1, 2, 3}
    assert len(E.sweep_list()) == 261 + 2 * len(E.lengths(E.SHORT_UNITS)) == 327
    for kind, Nx in E.sweep_list():
        case = E.sweep_case(orc, kind, Nx)
        L, st = orc.generate_batch(case["mid"], case["w"]["plength"], case["w"]["x"], case["y"], case["P"], case["T"],
                                   sigma_y=case["sigma"], likelihood_case=case["like"])
        assert np.all(st == 0) and np.all(np.isfinite(L)), case["tag"]


@pytest.mark.parametrize("Nx", E.EDGE_GRIDS + E.CLAMP_GRIDS)
def test_every_edge_chain_hits_its_target(orc, Nx):
    case = E.edge_case(orc, Nx)
    full = Nx in E.EDGE_GRIDS
    w, ix, x, chains = case["w"], case["ix"], case["x"], case["chains"]
    p0 = w["params_true"]
    assert case["missing"] == []
    assert float(np.log2(x[1] - x[0])) % 1.0 != 0.0          # the step is not a power of two
    # every target that exists on the grid was built, per case kind; none is empty
    bs = case["boundaries"]
    if full:
        assert {512 * k for k in range(Nx // 512 + 1)} <= set(bs) and Nx in bs and sum(b % 512 == 256 for b in bs) == 10
    count = collections.Counter(r["kind"] for r in chains)
    for kind in E.KINDS:
        edge, d = kind[:4], {"b": 0, "b-1": -1, "b+1": 1}[kind[6:]]
        want = sum(E.target_exists(edge, b + d, Nx) for b in bs)
        assert count[kind] == want and (want > 0 or not full), (kind, count[kind], want)
        assert want >= len(bs) - 2
    assert count[E.ONE_BIN] == sum(0 <= lo <= Nx - 2 for b in bs for lo in (b - 1, b)) > 0
    for k in ("clamp-below", "clamp-above", "clamp-whole", "empty-all", "nan"):
        assert count[k] >= 1, k
    if full:
        assert count["empty-one"] >= 1
        assert all(count[f"ulp-{e}-{s}"] == 10 for e in ("imin", "imax") for s in ("below", "at"))
        assert len(chains) >= 500                         # hundreds of chains per call
    # the window of every chain, as the oracle reports it
    for i, r in enumerate(chains):
        st, a, b = E._Win(orc, x, w, ix)(case["P"][i, ix["fc"]], case["P"][i, ix["c"]])
        if r["kind"] in ("empty-one", "empty-all"):
            assert st == orc.EMPTY_WINDOW, r
            continue
        assert st == 0, r
        if r["edge"] is not None:
            assert (a if r["edge"] == "imin" else b) == r["v"], (r, a, b)
            assert 0 <= a < b <= Nx
        if r["win"] is not None:
            assert (a, b) == tuple(r["win"]), (r, a, b)
        if r["kind"] == E.ONE_BIN:
            assert b - a == 1 and (a == r["b"] or b == r["b"])
    by = {r["kind"]: r for r in chains}
    assert by["clamp-below"]["win"][0] == 0 and 1 <= by["clamp-below"]["win"][1] < Nx // 2          # pmax := x0 + c
    assert by["clamp-above"]["win"][1] == Nx and by["clamp-above"]["win"][0] > Nx // 2               # pmin := x_last - c
    assert by["clamp-whole"]["win"] == (0, Nx)
    assert any(r["edge"] == "imax" and r["v"] == Nx for r in chains)                                # imax == Nx
    # adjacent doubles: one ulp of fc apart, the edge one bin apart
    for e in ("imin", "imax"):
        lo = [r for r in chains if r["kind"] == f"ulp-{e}-below"]
        hi = [r for r in chains if r["kind"] == f"ulp-{e}-at"]
        for a, b in zip(lo, hi):
            assert np.nextafter(a["fc"], np.inf) == b["fc"] and a["v"] + 1 == b["v"] == a["b"]
    # statuses: as expected for every chain, and the chains that do not evaluate are spread through the batch
    ans = E.edge_logL(orc, case)
    assert np.array_equal(ans["st"], [r["status"] for r in chains])
    assert np.all(np.isfinite(ans["L"][ans["ok"]])) and np.all(ans["gst"] == 0) and np.all(np.isfinite(ans["g"]))
    bad = np.flatnonzero(~ans["ok"])
    if full:
        assert bad.size >= 6 and bad[0] < len(chains) // 4 and bad[-1] > len(chains) // 2
    # the probe's value at the edge bins, as the teeth condition uses it: the oracle's model with and without the probe
    i = next(k for k, r in enumerate(chains) if r["edge"] is not None and r["e_in"] >= 0)
    p = case["P"][i].copy()
    m1, _ = orc.model(2, p, w["plength"], x)
    p[ix["H"]] = 0.0
    m0, _ = orc.model(2, p, w["plength"], x)
    e = chains[i]["e_in"]
    assert abs((m1[e] - m0[e]) - chains[i]["h_in"]) <= 1e-9 * chains[i]["h_in"] and abs(m1[e] - chains[i]["M_in"]) <= 1e-14 * m1[e]
    e = chains[i]["e_out"]
    assert e < 0 or m1[e] == m0[e]
    # teeth: one mislaid bin at the targeted edge costs every chain at least ten times the logL tolerance
    idx, share = E.teeth(case, ans["L"])
    assert idx.size == sum(count[k] for k in count if k.startswith(("imin", "imax", "ulp")))
    worst = int(np.argmin(share))
    print(f"edge chains at {Nx} bins: {len(chains)}, {idx.size} with a targeted edge, smallest cost of one mislaid bin "
          f"{share[worst]:.2e} |logL| ({chains[idx[worst]]['kind']} at {chains[idx[worst]]['b']})")
    assert share[worst] >= 10 * 1e-10, (chains[idx[worst]], share[worst])


def test_shared_noise_draw_is_make_spectrum():
    from tamcmc_amd import synth
    m = 0.5 + np.arange(3000.0) % 7.0
    assert np.array_equal(synth.make_spectrum(m), m * E._noise(m.size))


def test_lds_preconditions_of_the_gradient_cases(orc):
    """The layouts and variable counts of the gradient cases at the multiplet limit sit where they are meant to sit."""
    for mid in E.MULT_IDS:
        for Nmax, lmax in E.MULT_SHAPES:
            w = E.mult_case(orc, mid, Nmax, lmax)["w"]
            full = E.backward_lds_bytes(w, w["index_to_relax"].size)
            if Nmax * (lmax + 1) >= 255:
                some = E.backward_lds_bytes(w, E.spread_vars(w, 96).size)
                assert full > E.BW_LDS_MAX >= some and some + E.records_bytes(w) > E.BW_AUX_STAGED
            else:
                assert full + E.records_bytes(w) <= E.BW_AUX_STAGED
        w = E.mult_case(orc, mid, *E.NEAR_LIMIT_SHAPE)["w"]
        full = E.backward_lds_bytes(w, w["index_to_relax"].size)
        assert full <= E.BW_LDS_MAX and full + E.records_bytes(w) > E.BW_AUX_STAGED
    assert w["index_to_relax"].size > 384          # id 13: more variables than the backward kernel's staging threads


def test_multiplet_count_cases_evaluate_in_the_oracle(orc):
    counts = sorted({n * (l + 1) for n, l in E.MULT_SHAPES})
    assert counts == [16, 17, 32, 33, 64, 65, 255, 256]
    assert E.MULT_REFUSED[0] * (E.MULT_REFUSED[1] + 1) == 258
    for mid in E.MULT_IDS:
        for Nmax, lmax in E.MULT_SHAPES:
            case = E.mult_case(orc, mid, Nmax, lmax)
            L, st = orc.generate_batch(mid, case["w"]["plength"], case["w"]["x"], case["y"], case["P"], case["T"])
            assert np.all(st == 0) and np.all(np.isfinite(L)), case["tag"]
