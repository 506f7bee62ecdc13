"""Case lists of the variable-list suites (tests/test_grad_vars_host.py, tests/test_grad_vars_gpu.py): which lists
`tamcmc_ctx_set_vars` is given, on which workloads.  Test helper only: no GPU, and no oracle arithmetic of its own (the
oracle is called for the data and for the reference rows, nothing is restated here).

The list is the one input of the gradient path the other suites never vary: they pass np.flatnonzero(relax) -- ascending,
free of repeats, nearly the whole row.  Here, per workload:
  full, full reversed, two shuffles of full, the canonical index_to_relax reversed, every singleton, "everything except
  one kind" (heights, visibilities, the frequencies of one degree, the splitting block, the widths / AppWidth block, each
  Harvey profile, the white noise, the inclination block), "only the parameters no pair addresses", and for the ids with
  the sqrt(a1) cos i / sin i pair each of the pair alone and the pair swapped; for id 9 heights only and frequencies only.
Length edges (prefixes of a shuffle of full): 1, 2, 63 / 64 / 65, 127 / 128 / 129 (phase 3 of the backward kernel gathers in
blocks of 64 variables), 383 / 384 / 385 (its 384 staging threads), 488 / 311 and the whole row, on the 180-multiplet layouts of
edgecases.NEAR_LIMIT_SHAPE; and, on a 102-multiplet layout, the two lengths between which the per-multiplet records stop
being staged in LDS."""
import numpy as np

import edgecases as E
import layouts
import workloads as W
from tamcmc_amd import synth

IDS = tuple(W.ALL_IDS)                       # the 13 live ids
GLOBAL_IDS = layouts.GLOBAL_IDS
GRIDS = {"fused": 1900, "tiled": 9000}       # 4 units of 512 bins: one tile, fused launch; 18 units: tiled
NCHAINS = 3
TEMPERATURES = np.array([1.0, 2.0, 3.0])
NOISE = layouts.BACKGROUNDS["three-profiles"]    # all three Harvey profiles active, exponents 4, 2, 3
VARIANTS = {"sym": dict(), "asym-amp": dict(asym=25.0, do_amp=True)}
ASYM_IDS = (2, 11)                           # run a second time with asym = 25 and the amplitude form
PAIR_IDS = (2, 9, 10, 11)                    # a1 and the inclination both come from the pair at s + 3, s + 4
SHUFFLE_SEEDS = (101, 202)

WORKLOADS = [(mid, "sym") for mid in IDS] + [(mid, "asym-amp") for mid in ASYM_IDS]
CASES = [(mid, v, g) for (mid, v) in WORKLOADS for g in GRIDS]


def case_id(mid, variant, grid=None):
    return f"id{mid}-{variant}" + (f"-{grid}" if grid else "")


def workload(mid, variant="sym", grid="fused", trunc_c=20.0):
    """The workload of one case: global ids at lmax = 3 with 5 radial orders, local ids with modes of every degree 0..3."""
    Nx = GRIDS[grid]
    if mid in (0, 1):
        return W.make_gauss(mid, Nx=Nx)
    return W.layout(mid, 3, noise=NOISE, Nmax=5, Nx=Nx, trunc_c=trunc_c, **VARIANTS[variant])


def blocks(w):
    """name -> parameter indices of every block of the row."""
    pl = [int(v) for v in w["plength"]]
    o = np.concatenate([[0], np.cumsum(pl)]).astype(int)
    mid = w["model_case"]
    b = {}
    if mid == 0:                              # A, sigma, centre, white noise: one block of four
        return {"profile": np.arange(3), "white": np.array([3])}
    b["profile" if mid == 1 else "heights"] = np.arange(o[0], o[1])
    b["visibilities"] = np.arange(o[1], o[2])
    for l in range(4):
        b[f"freq-l{l}"] = np.arange(o[2 + l], o[3 + l])
    b["splitting"] = np.arange(o[6], o[7])
    b["widths"] = np.arange(o[7], o[8])
    z, nn = o[8], pl[8]
    for k in range((nn - 1) // 3):
        b[f"harvey{k}"] = np.arange(z + 3 * k, z + 3 * k + 3)
    b["white"] = np.array([z + nn - 1])
    b["inclination"] = np.arange(o[9], o[10])
    b["config"] = np.arange(o[10], o[11])     # trunc_c, do_amp
    return {k: v.astype(int) for k, v in b.items() if v.size}


def asym_index(w):
    """Index of the asymmetry (s + 5), or None for the Gaussian ids."""
    if w["model_case"] in (0, 1):
        return None
    return int(blocks(w)["splitting"][0]) + 5


def has_asym(w, lst):
    a = asym_index(w)
    return a is not None and a in set(int(i) for i in lst)


def asym_value(w):
    a = asym_index(w)
    return 0.0 if a is None else float(w["params_true"][a])


def unaddressed(w):
    """The parameters no (index, value) pair of the backward kernel addresses -- the oracle's zero columns (S_k = 0), written
    down per id.  tests/test_grad_vars_host.py holds this list against the oracle's rows.
      every Lorentzian id   trunc_c and the do_amp flag
      2, 9, 10, 11          the raw a1 (s): a1 comes from the pair at s + 3, s + 4; and the inclination entry
      7, 8                  the raw a1 (s): a1 is given per radial order; and the pair
      3, 6, 12, 13, 14      the pair: a1 is given directly
      13                    the visibilities: the m-heights are given directly
      14                    the inclination entry, and the entries of the heights block that the reference's overlapping
                            indexing off_l + (l + 1) n + |m| never reads"""
    mid = w["model_case"]
    if mid in (0, 1):
        return np.zeros(0, dtype=np.int32)
    b = blocks(w)
    s = int(b["splitting"][0])
    out = set(int(i) for i in b["config"])
    if mid in (2, 9, 10, 11):
        out |= {s} | set(int(i) for i in b["inclination"])
    if mid in (7, 8):
        out |= {s, s + 3, s + 4}
    if mid in (3, 6, 12, 13, 14):
        out |= {s + 3, s + 4}
    if mid == 13:
        out |= set(int(i) for i in b["visibilities"])
    if mid == 14:
        out |= set(int(i) for i in b["inclination"])
        pl = [int(v) for v in w["plength"]]
        read, off = set(), 0
        for l in range(4):
            for n in range(pl[2 + l]):
                read |= {n} if l == 0 else {off + (l + 1) * n + am for am in range(l + 1)}
            off += pl[2 + l]
        out |= set(range(pl[0])) - read
    return np.array(sorted(out), dtype=np.int32)


def kinds(w):
    """The kinds of "everything except one kind": name -> indices (only kinds the id has)."""
    b = blocks(w)
    names = ["heights", "profile", "visibilities", "freq-l0", "freq-l1", "freq-l2", "freq-l3", "splitting", "widths",
             "harvey0", "harvey1", "harvey2", "white", "inclination"]
    return {k: b[k] for k in names if k in b}


def lists(w):
    """name -> list (int32) of every non-singleton list of a workload."""
    n = int(w["plength"].sum())
    full = np.arange(n, dtype=np.int32)
    out = {"full": full, "full-reversed": full[::-1].copy()}
    for seed in SHUFFLE_SEEDS:
        out[f"shuffle-{seed}"] = np.random.default_rng(seed).permutation(full).astype(np.int32)
    out["canonical-reversed"] = np.asarray(w["index_to_relax"], dtype=np.int32)[::-1].copy()
    for name, idx in kinds(w).items():
        out[f"all-but-{name}"] = np.setdiff1d(full, idx).astype(np.int32)
    un = unaddressed(w)
    if un.size:
        out["unaddressed-only"] = un
    mid = w["model_case"]
    if mid in PAIR_IDS:
        s = int(blocks(w)["splitting"][0])
        out["pair-cos"] = np.array([s + 3], dtype=np.int32)
        out["pair-sin"] = np.array([s + 4], dtype=np.int32)
        out["pair-swapped"] = np.array([s + 4, s + 3], dtype=np.int32)
    if mid == 9:
        b = blocks(w)
        out["heights-only"] = b["heights"].astype(np.int32)
        out["frequencies-only"] = np.concatenate([b[f"freq-l{l}"] for l in range(4)]).astype(np.int32)
    return out


def singletons(w):
    return [np.array([i], dtype=np.int32) for i in range(int(w["plength"].sum()))]


def refusals(w):
    """name -> list that tamcmc_ctx_set_vars must refuse with TAMCMC_E_INVALID."""
    n = int(w["plength"].sum())
    full = np.arange(n, dtype=np.int32)
    return {
        "repeat-adjacent": np.array([0, 1, 1, 2], dtype=np.int32),
        "repeat-far-apart": np.concatenate([full, full[:1]]).astype(np.int32),      # also Nvars > Nparams
        "repeat-ends-of-a-shuffle": np.concatenate([[n - 2], np.random.default_rng(7).permutation(full[:n - 2]), [n - 2]]).astype(np.int32),
        "more-than-Nparams": np.concatenate([full, full]).astype(np.int32),
        "index-minus-one": np.array([0, -1], dtype=np.int32),
        "index-Nparams": np.array([n, 0], dtype=np.int32),
    }


# ---------------------------------------------------------------------------------------------------------------------
# data and reference rows, made once per case and left unchanged

_DATA = {}


def case(orc, mid, variant, grid):
    """w, y, P, T and the oracle's row over `full` (g, gabs, L, st) of one case."""
    key = (mid, variant, grid)
    if key not in _DATA:
        w = workload(mid, variant, grid)
        m, st = orc.model(mid, w["params_true"], w["plength"], w["x"])
        assert st == 0 and np.all(np.isfinite(m)) and np.all(m > 0)
        y = synth.make_spectrum(m, seed=61 + mid)
        P = W.perturbed(w, NCHAINS, scale=0.003, seed=13)
        full = np.arange(P.shape[1], dtype=np.int32)
        g, gabs, L, gst = orc.grad_analytic(mid, w["plength"], w["x"], y, P, TEMPERATURES, full)
        assert np.all(gst == 0) and np.all(np.isfinite(g))
        for a in (y, P, g, gabs, L):
            a.setflags(write=False)
        _DATA[key] = dict(mid=mid, w=w, y=y, P=P, T=TEMPERATURES, full=full, g=g, gabs=gabs, L=L, st=gst,
                          tag=case_id(mid, variant, grid))
    return _DATA[key]


# ---------------------------------------------------------------------------------------------------------------------
# length edges

LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 383, 384, 385)
STAGING_SHAPE = (34, 2)       # id 13, 102 multiplets, 292 entries: records staged in LDS up to 149 variables, read in place from 150
# (488 and 311 are the sizes of the canonical lists of the two 180-multiplet layouts, the largest lists run before; 500 and
# 321 are their whole rows)
LENGTH_LAYOUTS = [(13, E.NEAR_LIMIT_SHAPE, LENGTHS + (488, 500)),
                  (2, E.NEAR_LIMIT_SHAPE, tuple(n for n in LENGTHS if n <= 129) + (311, 321)),
                  (13, STAGING_SHAPE, (1, 64, 149, 150, 292))]
LENGTH_CHAINS = 2
LENGTH_SEED = 303


def length_workload(mid, shape):
    return W.layout(mid, shape[1], Nmax=shape[0], Nx=20000)


def length_lists(w, lengths):
    n = int(w["plength"].sum())
    sh = np.random.default_rng(LENGTH_SEED).permutation(n).astype(np.int32)
    return {k: sh[:k].copy() for k in lengths}


def records_staged(w, nvars):
    """Whether the backward kernel stages the per-multiplet records in LDS for this many variables (precondition
    bookkeeping from edgecases, not a model of the device)."""
    return E.backward_lds_bytes(w, nvars) + E.records_bytes(w) <= E.BW_AUX_STAGED
