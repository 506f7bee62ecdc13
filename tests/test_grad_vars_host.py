"""The reference of the variable-list suite must hold alone before the kernel is judged by it (CPU only).

tests/test_grad_vars_gpu.py compares the HIP gradient under many variable lists with the oracle's analytic row.  Many of
those entries are in nobody's `relax` flags, so neither derivative was ever compared with anything.  Here the oracle's
row over EVERY parameter is pinned against Richardson central differences of the oracle's own log-likelihood
(orc_grad_fd_wide) by the rule and the four steps of tests/test_oracle_grad.py (gradcheck.entrywise_error, unchanged).

Left out of the difference quotients: trunc_c and the do_amp flag, and nothing else -- a difference quotient moves every
window or flips the flag.  Their analytic entries must be exactly 0.  (The Gaussian ids 0 and 1 have neither entry: their
whole row is compared.)"""
import numpy as np
import pytest

import edgecases as E
import layouts
import varlists as V
import workloads as W
from gradcheck import entrywise_error
from tamcmc_amd import synth

WORKLOAD_IDS = [V.case_id(mid, v) for (mid, v) in V.WORKLOADS]


def _data(orc, w, seed):
    mid = w["model_case"]
    m, st = orc.model(mid, w["params_true"], w["plength"], w["x"])
    assert st == 0
    return synth.make_spectrum(m, seed=seed), W.perturbed(w, 2, scale=0.002, seed=5), np.array([1.0, 3.7])


@pytest.mark.parametrize("mid,variant", V.WORKLOADS, ids=WORKLOAD_IDS)
def test_full_row_against_finite_differences_window_off(orc, mid, variant):
    """Every entry of the row but trunc_c and do_amp, no truncation window (trunc_c = 10000: logL is smooth)."""
    w = V.workload(mid, variant, "fused", trunc_c=10000.0)
    y, P, T = _data(orc, w, 67 + mid)
    n = P.shape[1]
    full = np.arange(n, dtype=np.int32)
    cfg = V.blocks(w).get("config", np.zeros(0, dtype=int))
    assert cfg.size == (0 if mid in (0, 1) else 2)
    idx = np.setdiff1d(full, cfg).astype(np.int32)
    assert idx.size == n - cfg.size                 # Nparams - 2: nothing else is skipped
    g, gabs, _, st = orc.grad_analytic(mid, w["plength"], w["x"], y, P, T, full)
    assert np.all(st == 0) and np.all(np.isfinite(g)) and np.all(np.isfinite(gabs))
    assert np.all(g[:, cfg] == 0.0) and np.all(gabs[:, cfg] == 0.0)
    worst = entrywise_error(orc, mid, w, y, P, T, idx)
    print(f"{V.case_id(mid, variant)}: {idx.size} of {n} entries compared, worst {worst:.2e} of the bar's 1e-6")


def _window_free(w):
    """Entries that move no truncation window: heights, visibilities, eta, a3, the asymmetry, the noise and the
    inclination / m-height block (tests/test_oracle_grad.py).  In id 9 heights and visibilities move numax, hence every
    width, hence every window: left out there."""
    b = V.blocks(w)
    mid = w["model_case"]
    if mid in (0, 1):
        return np.arange(int(w["plength"].sum()), dtype=np.int32)
    s = int(b["splitting"][0])
    keep = [np.array([s + 1, s + 2, s + 5])]
    names = ["white", "harvey0", "harvey1", "harvey2", "inclination"] + ([] if mid == 9 else ["heights", "visibilities"])
    keep += [b[k] for k in names if k in b]
    return np.unique(np.concatenate(keep)).astype(np.int32)


@pytest.mark.parametrize("mid,variant", V.WORKLOADS, ids=WORKLOAD_IDS)
def test_full_row_against_finite_differences_window_on(orc, mid, variant):
    """The workloads as the GPU suite runs them (trunc_c = 20): the entries that move no window."""
    w = V.workload(mid, variant, "fused")
    y, P, T = _data(orc, w, 71 + mid)
    idx = _window_free(w)
    assert idx.size >= 4
    entrywise_error(orc, mid, w, y, P, T, idx)


@pytest.mark.parametrize("mid,variant", V.WORKLOADS, ids=WORKLOAD_IDS)
def test_row_of_a_list_is_the_gather_of_the_full_row(orc, mid, variant):
    """Bit for bit, for every list of the suite, for a list with repeats, and with an out-of-range index (NaN there)."""
    c = V.case(orc, mid, variant, "fused")
    w, n = c["w"], c["full"].size
    some = dict(V.lists(w))
    some["singleton-last"] = V.singletons(w)[-1]
    some["repeats"] = np.array([n - 1, 0, n - 1, 0, 0], dtype=np.int32)
    for name, lst in some.items():
        g, gabs, L, st = orc.grad_analytic(mid, w["plength"], w["x"], c["y"], c["P"], c["T"], lst)
        assert np.array_equal(st, c["st"]) and np.array_equal(L.view(np.int64), c["L"].view(np.int64)), name
        assert np.array_equal(g.view(np.int64), c["g"][:, lst].view(np.int64)), name
        assert np.array_equal(gabs.view(np.int64), c["gabs"][:, lst].view(np.int64)), name
    bad = np.array([0, n, 1, -1], dtype=np.int32)
    g, gabs, _, st = orc.grad_analytic(mid, w["plength"], w["x"], c["y"], c["P"], c["T"], bad)
    assert np.all(st == 0)
    assert np.all(np.isnan(g[:, [1, 3]])) and np.all(np.isnan(gabs[:, [1, 3]]))
    assert np.array_equal(g[:, [0, 2]], c["g"][:, [0, 1]])


@pytest.mark.parametrize("mid,variant,grid", V.CASES, ids=[V.case_id(*k) for k in V.CASES])
def test_unaddressed_parameters_are_the_oracles_zero_columns(orc, mid, variant, grid):
    """varlists.unaddressed (written down per id) against the columns whose sum of |terms| is 0 in every chain."""
    c = V.case(orc, mid, variant, grid)
    zero = np.flatnonzero(np.all(c["gabs"] == 0.0, axis=0))
    assert np.array_equal(zero, V.unaddressed(c["w"])), (zero, V.unaddressed(c["w"]))
    assert np.all(c["g"][:, zero] == 0.0)
    some = np.any(c["gabs"] == 0.0, axis=0)
    assert np.array_equal(np.flatnonzero(some), zero)      # no column is 0 in one chain only


@pytest.mark.parametrize("mid,variant,grid", V.CASES, ids=[V.case_id(*k) for k in V.CASES])
def test_case_lists_are_well_formed(mid, variant, grid):
    w = V.workload(mid, variant, grid)
    n = int(w["plength"].sum())
    assert layouts.launch(w) == grid
    assert w["x"].size == V.GRIDS[grid]
    a = V.asym_index(w)
    assert V.asym_value(w) == (25.0 if variant == "asym-amp" else 0.0)
    if mid not in (0, 1):
        cfg = V.blocks(w)["config"]
        assert w["params_true"][cfg[0]] == 20.0 and w["params_true"][cfg[1]] == (1.0 if variant == "asym-amp" else 0.0)
        assert layouts.degrees(w) == [0, 1, 2, 3]
    L = V.lists(w)
    for name, lst in L.items():
        assert lst.dtype == np.int32 and lst.size >= 1, name
        assert np.unique(lst).size == lst.size and lst.min() >= 0 and lst.max() < n, name
    assert np.array_equal(L["full"], np.arange(n)) and np.array_equal(L["full-reversed"], np.arange(n)[::-1])
    assert not np.array_equal(L["shuffle-101"], L["shuffle-202"])
    for name in ("shuffle-101", "shuffle-202"):
        assert np.any(np.diff(L[name]) < 0) and np.array_equal(np.sort(L[name]), np.arange(n))
    assert np.array_equal(L["canonical-reversed"][::-1], w["index_to_relax"])
    # every parameter appears in a singleton, and every block of the row is a kind or the config block
    assert np.array_equal(np.concatenate(V.singletons(w)), np.arange(n))
    cover = np.concatenate(list(V.kinds(w).values()) + [V.blocks(w).get("config", np.zeros(0, dtype=int))])
    assert np.array_equal(np.sort(cover), np.arange(n))
    for name, idx in V.kinds(w).items():
        assert not set(idx.tolist()) & set(L[f"all-but-{name}"].tolist())
        assert L[f"all-but-{name}"].size == n - idx.size
    if mid not in (0, 1):
        assert {"all-but-heights", "all-but-splitting", "all-but-widths", "all-but-white", "all-but-inclination",
                "all-but-freq-l0", "all-but-freq-l3", "unaddressed-only"} <= set(L)
        assert not V.has_asym(w, L["all-but-splitting"]) and V.has_asym(w, L["all-but-heights"]) and a == V.blocks(w)["splitting"][0] + 5
    if mid in V.GLOBAL_IDS:
        assert {"all-but-harvey0", "all-but-harvey1", "all-but-harvey2"} <= set(L)
        z = int(V.blocks(w)["harvey0"][0])
        assert np.all(w["params_true"][z:z + 9] != 0.0)      # three active profiles, non-zero exponents
    if mid in V.PAIR_IDS:
        s = a - 5
        assert L["pair-cos"].tolist() == [s + 3] and L["pair-sin"].tolist() == [s + 4] and L["pair-swapped"].tolist() == [s + 4, s + 3]
    if mid == 9:
        assert L["heights-only"].tolist() == list(range(5)) and L["frequencies-only"].size == 20
    # the refusal cases are the only lists with a repeat or an index out of range
    for name, lst in V.refusals(w).items():
        assert np.unique(lst).size < lst.size or lst.min() < 0 or lst.max() >= n or lst.size > n, name
    R = V.refusals(w)
    assert R["repeat-ends-of-a-shuffle"].size == n and R["repeat-ends-of-a-shuffle"][0] == R["repeat-ends-of-a-shuffle"][-1]
    assert R["repeat-ends-of-a-shuffle"].min() >= 0 and R["repeat-ends-of-a-shuffle"].max() < n


def test_length_edges_reach_both_sides_of_the_kernels_switches():
    """The prefix lengths stand on both sides of the 64-variable blocks and of the 384 staging threads, and the records
    are staged in LDS in some cases and read in place in others (bookkeeping of edgecases: the 180-multiplet layouts
    always read them in place -- tables and records together take 158 KB and more -- so a 102-multiplet layout supplies
    the switch itself, between 149 and 150 variables)."""
    staged = set()
    seen = set()
    for mid, shape, lengths in V.LENGTH_LAYOUTS:
        w = V.length_workload(mid, shape)
        n = int(w["plength"].sum())
        assert lengths[-1] == n and layouts.launch(w) == "tiled"
        L = V.length_lists(w, lengths)
        for k, lst in L.items():
            assert lst.size == k and np.unique(lst).size == k and lst.min() >= 0 and lst.max() < n
            assert E.backward_lds_bytes(w, k) <= E.BW_LDS_MAX
            staged.add((shape, V.records_staged(w, k)))
            seen.add(k)
        assert np.any(np.diff(L[n]) < 0)
    assert {1, 2, 63, 64, 65, 127, 128, 129, 383, 384, 385, 488, 311} <= seen
    assert (E.NEAR_LIMIT_SHAPE, True) not in staged
    assert (V.STAGING_SHAPE, True) in staged and (V.STAGING_SHAPE, False) in staged
    w = V.length_workload(13, V.STAGING_SHAPE)
    assert V.records_staged(w, 149) and not V.records_staged(w, 150)
    # the small workloads stage their records whatever the list
    for mid in (2, 13):
        w = V.workload(mid, "sym", "tiled")
        assert V.records_staged(w, int(w["plength"].sum()))
