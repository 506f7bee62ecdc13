"""CPU checks of the layout matrix of tests/test_layouts_gpu.py (case list: tests/layouts.py): the oracle accepts every
case, and the cases together reach every kernel specialisation -- each (ncomp, asymmetric) shape of tm_accum_mult /
tm_grad_mult in the fused and in the tiled launch, of the likelihood and of the gradient -- every global id at lmax 0..3,
and a chain whose grid holds both polynomial and exact background cells.  The C ABI checks a layout only after it has
found a device (tamcmc_ctx_create), so the library's acceptance of each case is asserted in the GPU file."""
import numpy as np
import pytest

import layouts as LY
import workloads as W


@pytest.mark.parametrize("name,mid,lmax,variant,grid", LY.matrix_cases(), ids=[c[0] for c in LY.matrix_cases()])
def test_oracle_accepts_every_matrix_case(orc, name, mid, lmax, variant, grid):
    w = LY.matrix_case(mid, lmax, variant, grid)
    m, st = orc.model(mid, w["params_true"], w["plength"], w["x"])
    assert st == 0 and np.all(np.isfinite(m)) and np.all(m > 0), name
    assert sorted(LY.degrees(w)) == ([0, 1, 2, 3] if mid in LY.LOCAL_IDS else list(range(lmax + 1)))
    assert LY.launch(w) == grid


@pytest.mark.parametrize("name,mid,bg", LY.background_cases(), ids=[c[0] for c in LY.background_cases()])
def test_oracle_accepts_every_background_case(orc, name, mid, bg):
    w = LY.background_case(mid, bg)
    m, st = orc.model(mid, w["params_true"], w["plength"], w["x"])
    assert st == 0 and np.all(np.isfinite(m)) and np.all(m > 0), name
    z = int(w["plength"][:8].sum())
    active = [k for k in range(3) if w["params_true"][z + 3 * k + 1] != 0]
    assert len(active) == len(LY.BACKGROUNDS[bg])


def test_matrix_reaches_every_specialisation():
    hit = set()
    lmax_by_id = {mid: set() for mid in LY.GLOBAL_IDS}
    for (_, mid, lmax, variant, grid) in LY.matrix_cases():
        w = LY.matrix_case(mid, lmax, variant, grid)
        hit |= LY.reached(w)
        if mid in lmax_by_id:
            lmax_by_id[mid].add(int(w["plength"][1]))
    want = {(launch, kind, nc, asym) for launch in ("fused", "tiled") for kind in ("likelihood", "gradient")
            for nc in (1, 3, 5, 7) for asym in (False, True)}
    assert want <= hit, sorted(want - hit)
    assert all(v == {0, 1, 2, 3} for v in lmax_by_id.values()), lmax_by_id
    # l = 3 modes on the local ids too
    assert {mid for (_, mid, *_r) in LY.matrix_cases() if mid in LY.LOCAL_IDS} == set(LY.LOCAL_IDS)


def test_background_list_holds_a_mixed_cell_chain():
    """Both kinds of background cells in ONE chain (and in every chain the GPU test perturbs), the flip inside the grid,
    and a tile that meets a cell of each kind (tiles of 5 units, cells of 8)."""
    assert "mixed" in LY.BACKGROUNDS
    for mid in LY.BACKGROUND_IDS:
        w = LY.background_case(mid, "mixed")
        for p in W.perturbed(w, LY.NCHAINS, scale=0.003, seed=5):
            npoly, cells = W.poly_cells(w, p)
            assert 2 <= npoly <= cells - 2, (npoly, cells)
        units = (w["x"].size + 511) // 512
        assert LY.launch(w) == "tiled" and 30 <= units < 70 and (units // 10) % 8 != 0
    # the cell rule helper itself: no active profile -> every cell polynomial; p = 4 on a coarse grid -> none
    w = LY.background_case(2, "no-profile")
    assert W.poly_cells(w) == (7, 7)
    w = W.layout(2, 3, noise=((1.0, 50.0, 4.0),), Nx=28000, grid=(2330.0, 0.05))
    assert W.poly_cells(w)[0] == 0
