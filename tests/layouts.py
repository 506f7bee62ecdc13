"""Case list of the layout / specialisation matrix (tests/test_layouts_gpu.py) and what each case reaches on the device.
Test helper only: tests/test_layout_matrix.py reads the same list on the CPU and checks its coverage, so that an edit to
the matrix cannot silently drop a kernel specialisation.

Device rules restated here (precondition bookkeeping, not a model of the device):
  * a multiplet of degree l is a (2l+1)-component shape; it takes the asymmetric variant when the chain's asymmetry is
    not 0 or, in the gradient launch, when the asymmetry is one of the variables (tamcmc_setup_body.h: asym_bit);
  * a grid of at most 4 units of 512 bins is one tile, and one tile is evaluated by the fused launch (tamcmc_dev.h:
    tm_tiles, tamcmc_host.h: `tm_takes_fused`); longer grids are tiled."""
import workloads as W

GLOBAL_IDS = (2, 3, 6, 7, 8, 9, 10, 12, 13)
LOCAL_IDS = (11, 14)

# (model id, lmax): every global id at lmax 0..3; the local ids carry modes of every degree 0..3 (lmax unused)
LAYOUTS = [(mid, lmax) for mid in GLOBAL_IDS for lmax in range(4)] + [(mid, 3) for mid in LOCAL_IDS]

VARIANTS = {
    "sym": dict(),
    "asym-amp": dict(asym=25.0, do_amp=True),
    "neg-asym-c7": dict(asym=-40.0, trunc_c=7.0),
}

# grid lengths: one tile (fused launch) and a tiled grid of 55 units -- tiles of 5 units, so tiles straddle the
# 8-unit cells of the background polynomials
GRIDS = {"fused": 1900, "tiled": 28000}

NCHAINS = 3

# Harvey backgrounds, run on id 2 and id 13 at lmax = 3 (tiled grid); "mixed" also picks its grid (see mixed_grid)
BACKGROUNDS = {
    "three-profiles": ((11.049588, 49.669854, 4.0), (0.93569041, 1.3516447, 2.0), (0.4, 8.0, 3.0)),
    "p-zero": ((11.049588, 49.669854, 4.0), (0.9, 1.3516447, 0.0)),
    "non-integer-p": ((11.049588, 49.669854, 3.3), (0.93569041, 1.3516447, 1.7), (0.3, 6.0, 2.45)),
    "negative-entries": ((-11.049588, 49.669854, 4.0), (0.93569041, -1.3516447, 2.0), (0.4, 8.0, -3.0)),
    "no-profile": (),
    "mixed": ((11.049588, 49.669854, 4.0), (0.93569041, 1.3516447, 2.0), (0.4, 8.0, 3.0)),
}
BACKGROUND_IDS = (2, 13)


def mixed_grid(Nx, pmax=4.0, x0=2330.0):
    """(x0, step) such that the largest power's flip between exact and polynomial cells (|p| * span = 0.04 with
    span ~ 2048 step / x) falls in the middle of the grid."""
    step = x0 / (2048.0 * pmax / 0.04 - Nx / 2.0)
    return (x0, step)


def matrix_case(mid, lmax, variant, grid):
    """The workload of one matrix case."""
    return W.layout(mid, lmax, Nx=GRIDS[grid], **VARIANTS[variant])


def background_case(mid, name):
    Nx = GRIDS["tiled"]
    g = mixed_grid(Nx) if name == "mixed" else None
    return W.layout(mid, 3, noise=BACKGROUNDS[name], Nx=Nx, grid=g)


def matrix_cases():
    """(id string, mid, lmax, variant, grid) of every matrix case."""
    return [(f"id{mid}-l{lmax}-{v}-{g}", mid, lmax, v, g) for (mid, lmax) in LAYOUTS for v in VARIANTS for g in GRIDS]


def background_cases():
    return [(f"id{mid}-{name}", mid, name) for mid in BACKGROUND_IDS for name in BACKGROUNDS]


def degrees(w):
    pl = w["plength"]
    if w["model_case"] in (11, 14):
        return [l for l in range(4) if pl[2 + l] > 0]
    return list(range(int(pl[1]) + 1))


def launch(w):
    units = (w["x"].size + 511) // 512
    return "fused" if units <= 4 else "tiled"


def reached(w):
    """{(launch, kind, ncomp, asymmetric)} the workload's chains reach (kind: 'likelihood' or 'gradient')."""
    pl = w["plength"]
    s = int(pl[0] + pl[1] + pl[2:6].sum())
    asym = w["params_true"][s + 5] != 0.0
    asym_var = s + 5 in set(int(i) for i in w["index_to_relax"])
    out = set()
    for l in degrees(w):
        out.add((launch(w), "likelihood", 2 * l + 1, bool(asym)))
        out.add((launch(w), "gradient", 2 * l + 1, bool(asym or asym_var)))
    return out
