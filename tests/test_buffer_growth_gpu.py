"""Buffers that grow during an object's life (tamcmc_host.h: TmPinned; tamcmc_api.cpp: tm_ensure_capacity, ensure_host):
a context's slab, its pinned staging and its model rows, a fit group's staging and its two mapped buffers, a summary's
context.  Every call below makes something grow (or, with fewer variables, shrink and move), and after every call the
results must equal, bit for bit, what fresh objects return for that call alone -- the documented invariant that a chain's
result depends neither on the batch nor on the object's history.  One likelihood call and one gradient call per grid are
also held against the oracle, with the bars of tests/test_parity_gpu.py and tests/test_grad_gpu.py.

Grids: 1024 bins = 2 units, one tile, the fused launch; 2560 bins = 5 units, 5 tiles, setup + eval."""
import functools

import numpy as np
import pytest

import workloads as W
from summary_support import same
from support import bits
from tamcmc_amd import capi, synth
from test_grad_gpu import gradcheck
from test_parity_gpu import check_logL, spectrum_for

pytestmark = pytest.mark.gpu

GRIDS = {1024: 1, 2560: 5}      # Nx: tiles per chain
NMAX = 12


@functools.lru_cache(maxsize=None)
def case(Nx):
    """Workload, spectrum, 12 chain rows and temperatures of one grid (computed once, never changed)."""
    from oracle import pyoracle
    pyoracle.lib()
    w = W.make(2, Nx=Nx)
    y = spectrum_for(pyoracle, w)
    P = W.perturbed(w, NMAX, scale=0.003)
    T = synth.temperatures(NMAX)
    for a in (y, P, T):
        a.setflags(write=False)
    return w, y, P, T


def fresh(accel_mod, Nx):
    w, y, _, _ = case(Nx)
    return accel_mod.Accel(2, w["plength"], w["x"], y)


def equal_bits(got, want, tag):
    assert len(got) == len(want), tag
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, k)
        if a.dtype == np.float64:
            a, b = bits(a), bits(b)
        assert np.array_equal(a, b), (tag, k)


# One step of part A: (name, chains, what to do with an open context) -> tuple of result arrays.
def _steps(Nx):
    w, _, P, T = case(Nx)
    idx = w["index_to_relax"]

    def plain(n, **kw):
        return lambda acc: acc.eval_batch(P[:n], T[:n], **kw)

    def with_vars(v, n):
        def f(acc):
            acc.set_vars(v)
            return acc.eval_batch(P[:n], T[:n], grad=True)
        return f

    def begin_end(n):
        def f(acc):
            acc.begin(P[:n], T[:n])
            return acc.end()
        return f

    def arm_fire_end(n):
        def f(acc):
            acc.arm(n)                  # (sizes the buffers itself where they are too small: the reserve inside _arm)
            acc.fire(P[:n], T[:n])
            return acc.end()
        return f

    return [("2 chains", plain(2)),
            ("7 chains, gradient", with_vars(idx, 7)),
            ("fewer variables, 7 chains, gradient", with_vars(idx[1::2], 7)),
            ("3 chains, 2 model rows", plain(3, model_rows=[2, 0])),
            ("7 chains, a model row each", plain(7, model_rows=list(range(7)))),
            ("begin / end, 9 chains", begin_end(9)),
            ("arm / fire / end, 9 chains", arm_fire_end(9)),
            ("arm / fire / end, 12 chains", arm_fire_end(12))]


@pytest.mark.parametrize("Nx", sorted(GRIDS))
def test_context_calls_of_growing_need(accel_mod, orc, Nx):
    w, y, P, T = case(Nx)
    with fresh(accel_mod, Nx) as acc:
        assert acc.geometry()["tiles"] == GRIDS[Nx]
        for name, step in _steps(Nx):
            got = step(acc)
            with fresh(accel_mod, Nx) as alone:
                want = step(alone)
            equal_bits(got, want, (Nx, name))
            assert np.all(got[1] == 0), (Nx, name)
            if name == "2 chains":
                rL, rst = orc.generate_batch(2, w["plength"], w["x"], y, P[:2], T[:2])
                assert np.array_equal(got[1], rst)
                check_logL(got[0], rL)
            if name == "7 chains, gradient":
                rL, rst = orc.generate_batch(2, w["plength"], w["x"], y, P[:7], T[:7])
                assert np.array_equal(got[1], rst)
                check_logL(got[0], rL)
                gradcheck.check_against_oracle(None, orc, 2, w, y, P[:7], T[:7], tag=f"Nx = {Nx}", g=got[2])


def test_group_calls_of_growing_need(accel_mod):
    """eval: one staging area and its device twin, and the members' own buffers through the group; begin / end: one mapped
    buffer per call parity, allocated half as large again as the call needs -- the totals 2, 3, 7, 12 allocate both and
    then outgrow both (7 > 1.5 * 2, 12 > 1.5 * 3; both members have the same row length)."""
    grids = sorted(GRIDS)
    cases = [case(Nx) for Nx in grids]

    def alone(counts):
        out = []
        for Nx, (w, y, P, T), n in zip(grids, cases, counts):
            if n == 0:
                out.append((np.empty(0), np.empty(0, dtype=np.int32)))
                continue
            with fresh(accel_mod, Nx) as acc:
                out.append(acc.eval_batch(P[:n], T[:n]))
        return [o[0] for o in out], [o[1] for o in out]

    with fresh(accel_mod, grids[0]) as a0, fresh(accel_mod, grids[1]) as a1:
        with capi.Group([a0, a1]) as g:
            for counts in [(2, 3), (6, 1), (0, 8)]:
                Pl = [c[2][:n] for c, n in zip(cases, counts)]
                Tl = [c[3][:n] for c, n in zip(cases, counts)]
                L, st = g.eval(Pl, Tl)
                rL, rst = alone(counts)
                equal_bits(L + st, rL + rst, ("eval", counts))
            for counts in [(1, 1), (2, 1), (3, 4), (5, 7)]:
                Pl = [c[2][:n] for c, n in zip(cases, counts)]
                Tl = [c[3][:n] for c, n in zip(cases, counts)]
                g.begin(Pl, Tl)
                L, st = g.end()
                rL, rst = alone(counts)
                equal_bits(L + st, rL + rst, ("begin / end", counts))


@pytest.mark.parametrize("Nx", sorted(GRIDS))
def test_summary_on_a_context_never_used_before(accel_mod, Nx):
    """Blocks of 3 samples: a push of 1, then of 7 (the context's buffers grow from nothing to 1 chain, then to 3),
    against one fresh summary on a fresh context given all 8 at once."""
    _, _, P, _ = case(Nx)
    with fresh(accel_mod, Nx) as acc, capi.Summary(acc, 3) as s:
        out = [s.push(P[:1]), s.push(P[1:8])]
        res = s.result()
    with fresh(accel_mod, Nx) as acc, capi.Summary(acc, 3) as s:
        L, st = s.push(P[:8])
        ref = s.result()
    assert ref["n_used"] == 8 and same(res, ref)
    equal_bits((np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])), (L, st), Nx)
