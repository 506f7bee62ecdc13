"""The gradient under every kind of variable list (tests/varlists.py): tamcmc_ctx_set_vars is the one input of the
gradient path that the other suites never vary -- they pass np.flatnonzero(relax), ascending and nearly the whole row.

  a  against the oracle: status and logL by the bars of tests/test_parity_gpu.py (identical; 1e-10 relative), the gradient
     by gradcheck.assert_grad_entrywise against orc.grad_analytic CALLED WITH THE SAME LIST; a column whose parameter no
     pair addresses has S_k = 0 and must be exactly 0.  (Singletons: the gather of the oracle's full row, which
     tests/test_grad_vars_host.py shows to be the same bits.)
  b  against itself, bit for bit: column k under list V is column V[k] of the gradient under `full` from a fresh context,
     logL and status are those of the `full` batch.  The backward kernel sums a variable's pairs in pair order within a
     wave and the waves in wave order, and its chunk ranges depend on the layout only.  At asym == 0 the list decides the
     forward code path (TmLayout::asym_var: the asymmetric path when s + 5 is a variable), so there the law holds between
     lists that agree on containing s + 5: lists without it are held, bit for bit, to a fresh context given `full` without
     s + 5, and the two references' logL to 1e-12 relative.
  c  every singleton on ONE context by repeated set_vars, ascending and then descending
  d  switching on one context: with the asymmetry -> without -> likelihood only -> with -> full
  e  list lengths at the kernel's edges (blocks of 64 variables in phase 3, 384 staging threads, the staging of the records)
  f  per-chain tile boundaries (TAMCMC_EQUAL_COST=1: the backward kernel searches the tile starts)
  g  refusals: a repeated index, an index out of range, more variables than parameters, a batch in flight or armed;
     no variables at all.
Measured on an MI355X: see DESIGN.md, "Variable lists"."""
import numpy as np
import pytest

import edgecases as E
import gradcheck
import varlists as V

pytestmark = pytest.mark.gpu

RTOL_LOGL = 1e-10       # HIP against the oracle (tests/test_parity_gpu.py)
RTOL_LAUNCH = 1e-12     # logL of one chain between two launches that take different code paths

CASE_IDS = [V.case_id(*k) for k in V.CASES]
FIGURES = dict(ratio=0.0, dlogL=0.0, lists=0, contexts=0)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def open_ctx(accel_mod, c):
    FIGURES["contexts"] += 1
    return accel_mod.Accel(c["mid"], c["w"]["plength"], c["w"]["x"], c["y"])


def fresh(accel_mod, c, lst):
    """(logL, status, grad) of the case's batch from a new context given `lst`."""
    with open_ctx(accel_mod, c) as acc:
        acc.set_vars(lst)
        return acc.eval_batch(c["P"], c["T"], grad=True)


def against_oracle(c, lst, out, ref, tag):
    """(a).  ref = (g, gabs, L, st) of the oracle for this list.  Returns the worst error / tolerance."""
    L, st, g = out
    rg, rabs, rL, rst = ref
    assert np.array_equal(st, rst) and np.all(st == 0), tag
    assert np.all(np.isfinite(rL)) and np.max(np.abs(L - rL) / np.abs(rL)) <= RTOL_LOGL, (tag, L, rL)
    assert g.shape == (c["P"].shape[0], len(lst)), tag
    err = np.abs(g - rg)
    tol = gradcheck.GRAD_RTOL * np.abs(rg) + gradcheck.GRAD_COND * rabs
    ratio = float(np.max(err[tol > 0] / tol[tol > 0])) if np.any(tol > 0) else 0.0
    print(f"  {tag}: {len(lst)} variables, gradient error / tolerance {ratio:.3f}")
    gradcheck.assert_grad_entrywise(g, rg, rabs, tag)
    assert np.all(g[rabs == 0.0] == 0.0), tag             # nobody's pair: exactly 0
    FIGURES["ratio"] = max(FIGURES["ratio"], ratio)
    FIGURES["lists"] += 1
    return ratio


def oracle_row(orc, c, lst):
    return orc.grad_analytic(c["mid"], c["w"]["plength"], c["w"]["x"], c["y"], c["P"], c["T"], lst)


class Reference:
    """The gradient under a reference list from a fresh context: the bits every other list's columns must have."""

    def __init__(self, accel_mod, c, lst):
        self.L, self.st, self.g = fresh(accel_mod, c, lst)
        self.pos = {int(p): k for k, p in enumerate(lst)}

    def same_bits(self, lst, out, tag):
        L, st, g = out
        assert np.array_equal(st, self.st) and bits_equal(L, self.L), (tag, L, self.L)
        want = self.g[:, [self.pos[int(i)] for i in lst]]
        if not bits_equal(g, want):
            bad = np.argwhere(g.view(np.int64) != np.ascontiguousarray(want).view(np.int64))
            raise AssertionError(f"{tag}: {len(bad)} entries differ in bits from the reference list's columns; first "
                                 f"chain {bad[0][0]} variable {bad[0][1]} (parameter {int(lst[bad[0][1]])}): "
                                 f"{g[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


def references(accel_mod, c):
    """{list contains s + 5 or asym != 0: Reference}.  One reference where the list cannot change the code path."""
    w, full = c["w"], c["full"]
    with_asym = Reference(accel_mod, c, full)
    a = V.asym_index(w)
    if a is None or V.asym_value(w) != 0.0:
        return {True: with_asym, False: with_asym}
    without = Reference(accel_mod, c, np.setdiff1d(full, [a]).astype(np.int32))
    assert np.array_equal(without.st, with_asym.st)
    d = float(np.max(np.abs(without.L - with_asym.L) / np.abs(with_asym.L)))
    assert d <= RTOL_LAUNCH, (c["tag"], without.L, with_asym.L)
    FIGURES["dlogL"] = max(FIGURES["dlogL"], d)
    return {True: with_asym, False: without}


def reference_for(R, w, lst):
    return R[V.has_asym(w, lst) or V.asym_value(w) != 0.0]


@pytest.mark.parametrize("mid,variant,grid", V.CASES, ids=CASE_IDS)
def test_every_list_against_the_oracle_and_the_full_list(accel_mod, orc, mid, variant, grid):
    """(a) and (b) for every non-singleton list, each on a fresh context."""
    c = V.case(orc, mid, variant, grid)
    w = c["w"]
    R = references(accel_mod, c)
    worst = 0.0
    for name, lst in V.lists(w).items():
        tag = f"{c['tag']} [{name}]"
        out = fresh(accel_mod, c, lst)
        worst = max(worst, against_oracle(c, lst, out, oracle_row(orc, c, lst), tag))
        reference_for(R, w, lst).same_bits(lst, out, tag)
    print(f"{c['tag']}: {len(V.lists(w))} lists, worst gradient error / tolerance {worst:.3f}")


@pytest.mark.parametrize("mid,variant,grid", V.CASES, ids=CASE_IDS)
def test_every_singleton_on_one_context(accel_mod, orc, mid, variant, grid):
    """(c): Nparams singletons by repeated set_vars on one context, then once more in descending order."""
    c = V.case(orc, mid, variant, grid)
    w = c["w"]
    R = references(accel_mod, c)
    singles = V.singletons(w)
    worst = 0.0
    with open_ctx(accel_mod, c) as acc:
        for order in (singles, singles[::-1]):
            for lst in order:
                i = int(lst[0])
                tag = f"{c['tag']} [singleton {i}]"
                acc.set_vars(lst)
                out = acc.eval_batch(c["P"], c["T"], grad=True)
                ref = (c["g"][:, lst], c["gabs"][:, lst], c["L"], c["st"])
                err = np.abs(out[2] - ref[0])
                tol = gradcheck.GRAD_RTOL * np.abs(ref[0]) + gradcheck.GRAD_COND * ref[1]
                gradcheck.assert_grad_entrywise(out[2], ref[0], ref[1], tag)
                assert np.all(out[2][ref[1] == 0.0] == 0.0), tag
                assert np.array_equal(out[1], c["st"]) and np.max(np.abs(out[0] - c["L"]) / np.abs(c["L"])) <= RTOL_LOGL, tag
                if np.any(tol > 0):
                    worst = max(worst, float(np.max(err[tol > 0] / tol[tol > 0])))
                reference_for(R, w, lst).same_bits(lst, out, tag)
    FIGURES["ratio"] = max(FIGURES["ratio"], worst)
    FIGURES["lists"] += len(singles)
    print(f"{c['tag']}: {len(singles)} singletons twice on one context, worst gradient error / tolerance {worst:.3f}")


def switching_sequence(w):
    L = V.lists(w)
    a = V.asym_index(w)
    if a is None:
        return [L["shuffle-101"], L["all-but-white"], None, np.array([0], dtype=np.int32), L["full"]]
    return [L["all-but-heights"], L["all-but-splitting"], None, np.array([a], dtype=np.int32), L["full"]]


@pytest.mark.parametrize("mid,variant,grid", V.CASES, ids=CASE_IDS)
def test_switching_lists_on_one_context(accel_mod, orc, mid, variant, grid):
    """(d): a list with the asymmetry, one without it, a likelihood-only batch, a list with it again, `full` -- d_relax is
    reallocated and TmLayout::asym_var goes on, off and on.  Every gradient batch has the bits of a fresh context given
    that list; the likelihood-only batch has its bits from before any set_vars."""
    c = V.case(orc, mid, variant, grid)
    w = c["w"]
    seq = switching_sequence(w)
    a = V.asym_index(w)
    if a is not None:
        assert [None if l is None else V.has_asym(w, l) for l in seq] == [True, False, None, True, True]
    want = [None if lst is None else fresh(accel_mod, c, lst) for lst in seq]
    with open_ctx(accel_mod, c) as acc:
        L0, st0 = acc.eval_batch(c["P"], c["T"])
        for k, lst in enumerate(seq):
            if lst is None:
                L, st = acc.eval_batch(c["P"], c["T"])
                assert np.array_equal(st, st0) and bits_equal(L, L0), (c["tag"], k)
                continue
            acc.set_vars(lst)
            L, st, g = acc.eval_batch(c["P"], c["T"], grad=True)
            assert np.array_equal(st, want[k][1]) and bits_equal(L, want[k][0]) and bits_equal(g, want[k][2]), (c["tag"], k)
    against_oracle(c, seq[3], want[3], oracle_row(orc, c, seq[3]), f"{c['tag']} [switching, step 3]")


# ---------------------------------------------------------------------------------------------------------------------
_LENGTH = {}


def length_case(orc, mid, shape):
    if (mid, shape) not in _LENGTH:
        case = E.mult_case(orc, mid, *shape, nchains=V.LENGTH_CHAINS)
        w = case["w"]
        full = np.arange(int(w["plength"].sum()), dtype=np.int32)
        _LENGTH[(mid, shape)] = dict(mid=mid, w=w, y=case["y"], P=case["P"], T=case["T"], full=full,
                                     tag=f"id{mid}-{shape[0]}x{shape[1] + 1}")
    return _LENGTH[(mid, shape)]


@pytest.mark.parametrize("mid,shape,lengths", V.LENGTH_LAYOUTS, ids=[f"id{m}-{s[0]}x{s[1] + 1}" for m, s, _ in V.LENGTH_LAYOUTS])
def test_list_lengths_at_the_kernels_edges(accel_mod, orc, mid, shape, lengths):
    """(e): prefixes of a shuffle of `full` on the 180-multiplet layouts (and the 102-multiplet one that has the records'
    staging switch between 149 and 150 variables), 2 chains, by (a) and (b)."""
    c = length_case(orc, mid, shape)
    w = c["w"]
    assert V.asym_value(w) == 0.0
    R = references(accel_mod, c)
    for n, lst in V.length_lists(w, lengths).items():
        tag = f"{c['tag']} [{n} variables, records {'staged' if V.records_staged(w, n) else 'in place'}]"
        out = fresh(accel_mod, c, lst)
        against_oracle(c, lst, out, oracle_row(orc, c, lst), tag)
        reference_for(R, w, lst).same_bits(lst, out, tag)


@pytest.mark.parametrize("mid", [2, 9])
def test_per_chain_tile_boundaries(accel_mod, orc, monkeypatch, mid):
    """(f): TAMCMC_EQUAL_COST=1 -- every chain has its own tile boundaries and the backward kernel finds a window's tiles
    by a search over the tile starts (uniform_su == 0) instead of a division."""
    monkeypatch.setenv("TAMCMC_EQUAL_COST", "1")
    c = V.case(orc, mid, "sym", "tiled")
    w = c["w"]
    L = V.lists(w)
    names = ["full", "full-reversed"] + (["heights-only"] if mid == 9 else [])
    R = references(accel_mod, c)
    for name in names:
        tag = f"{c['tag']} equal-cost [{name}]"
        out = fresh(accel_mod, c, L[name])
        against_oracle(c, L[name], out, oracle_row(orc, c, L[name]), tag)
        reference_for(R, w, L[name]).same_bits(L[name], out, tag)


# ---------------------------------------------------------------------------------------------------------------------
def refused(accel_mod, acc, lst, code):
    nv = acc.Nvars
    with pytest.raises(accel_mod.capi.AccelError) as e:
        acc.set_vars(lst)
    assert e.value.code == code, (lst, e.value.code)
    assert acc.Nvars == nv


@pytest.mark.parametrize("mid,variant", V.WORKLOADS, ids=[V.case_id(*k) for k in V.WORKLOADS])
def test_refused_lists_leave_the_context_as_it_was(accel_mod, orc, mid, variant):
    """(g): a repeated index (adjacent, far apart), more variables than parameters, index -1 and index Nparams:
    TAMCMC_E_INVALID, and the next gradient batch has the bits of the one before."""
    c = V.case(orc, mid, variant, "tiled")
    w = c["w"]
    canon = V.lists(w)["canonical-reversed"]
    E_INVALID = accel_mod.capi.E_INVALID
    with open_ctx(accel_mod, c) as acc:
        for name, lst in V.refusals(w).items():       # a context without variables stays without
            refused(accel_mod, acc, lst, E_INVALID)
        with pytest.raises(accel_mod.capi.AccelError) as e:
            acc.eval_batch(c["P"], c["T"], grad=True)
        assert e.value.code == accel_mod.capi.E_NOVARS
        acc.set_vars(canon)
        L1, st1, g1 = acc.eval_batch(c["P"], c["T"], grad=True)
        for name, lst in V.refusals(w).items():
            refused(accel_mod, acc, lst, E_INVALID)
            L2, st2, g2 = acc.eval_batch(c["P"], c["T"], grad=True)
            assert g2.shape == g1.shape and np.array_equal(st1, st2) and bits_equal(L1, L2) and bits_equal(g1, g2), name
    against_oracle(c, canon, (L1, st1, g1), oracle_row(orc, c, canon), f"{c['tag']} [canonical-reversed]")


@pytest.mark.parametrize("mid", [2, 13])
def test_no_variables_and_busy_contexts(accel_mod, orc, mid):
    """(g): set_vars([]) takes the variables away (a gradient request is E_NOVARS, a likelihood batch is unaffected);
    set_vars with a batch in flight or armed is E_INVALID and changes nothing."""
    c = V.case(orc, mid, "sym", "tiled")
    w, P, T = c["w"], c["P"], c["T"]
    L = V.lists(w)
    capi = accel_mod.capi
    with open_ctx(accel_mod, c) as acc:
        L0, st0 = acc.eval_batch(P, T)
        acc.set_vars(L["shuffle-101"])
        L1, st1, g1 = acc.eval_batch(P, T, grad=True)
        acc.set_vars(np.zeros(0, dtype=np.int32))
        assert acc.Nvars == 0
        with pytest.raises(capi.AccelError) as e:
            acc.eval_batch(P, T, grad=True)
        assert e.value.code == capi.E_NOVARS
        Lb, stb = acc.eval_batch(P, T)
        assert np.array_equal(stb, st0) and bits_equal(Lb, L0)
        acc.set_vars(L["shuffle-101"])
        L2, st2, g2 = acc.eval_batch(P, T, grad=True)
        assert np.array_equal(st1, st2) and bits_equal(L1, L2) and bits_equal(g1, g2)
        # a batch in flight
        acc.begin(P, T)
        try:
            refused(accel_mod, acc, L["full"], capi.E_INVALID)
            refused(accel_mod, acc, np.zeros(0, dtype=np.int32), capi.E_INVALID)
        finally:
            Lb, stb = acc.end()
        assert np.array_equal(stb, st0) and bits_equal(Lb, L0)
        L2, st2, g2 = acc.eval_batch(P, T, grad=True)
        assert g2.shape == g1.shape and np.array_equal(st1, st2) and bits_equal(L1, L2) and bits_equal(g1, g2)
        # an armed batch
        acc.arm(P.shape[0])
        try:
            refused(accel_mod, acc, L["full"], capi.E_INVALID)
        finally:
            acc.fire(P, T)
            Lb, stb = acc.end()
        assert np.array_equal(stb, st0) and bits_equal(Lb, L0)
        L2, st2, g2 = acc.eval_batch(P, T, grad=True)
        assert g2.shape == g1.shape and np.array_equal(st1, st2) and bits_equal(L1, L2) and bits_equal(g1, g2)


def test_zz_figures_of_this_file():
    """Prints what the tests above measured (nothing to assert: every bar was held where it was measured)."""
    print(f"variable lists: {FIGURES['lists']} lists on {FIGURES['contexts']} contexts, worst gradient error / tolerance "
          f"{FIGURES['ratio']:.3f}, worst relative logL difference between the two code paths at asym == 0 {FIGURES['dlogL']:.2e}")
