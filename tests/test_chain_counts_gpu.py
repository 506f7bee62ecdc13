"""The launches past 65 535 chains: N = 70 001 chains in one call on every launch path (fused one-tile, tiled in the three
launch orders, gradient, chi_square with model rows, the host paths begin / end and arm / fire / end, device pointers,
fit groups), where the largest batch elsewhere in the suite is 4096 one-tile chains and 480 chains on a tiled grid.

The oracle is exact: a chain's result depends neither on the batch nor on its position in it, so the 70 001 chains must
equal, bit for bit (logL, status, gradient), the same rows evaluated in batches of 4096 on a fresh context.  On top of
that a subset -- every 257th chain, chains 0, 65 534 ... 65 537 and N - 1 -- goes through the CPU oracle with the suite's
bars (check_logL 1e-10, gradcheck's entry bound, model rows at 1e-12 per bin).  No tolerance is new.

The chain-major order (TAMCMC_ORDER=0) puts the chain count into grid.y of the eval launch: 70 001 there is accepted by the
runtime and gives the same bits.  Device memory of the largest case (5 tiles, gradient, 70 001 chains), measured with
hipMemGetInfo around it on an MI355X: 1.19 GB (0.74 GB for 18 tiles without a gradient; the `DEVICE MEMORY` lines of
pytest -s); it must stay below 8 GB.

Fit groups: one member with 65 537 chains beside small ones, and a group of 67 small contexts -- past one wave's worth, no
power of two, 14 ... 40 members in each of the four prefix tables that tm_group_member searches (1 ... 4 elsewhere in the
suite) -- with 0 ... 6 chains per member, so that members own one workgroup, or none, and neighbours in a prefix are equal.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import gradcheck
import workloads as W
from support import in_torch_process
from tamcmc_amd import capi, synth
from test_group_gpu import assert_group_matches_solo, bits_equal, close_all, mixed_members
from test_parity_gpu import RTOL_MODEL, check_logL

pytestmark = pytest.mark.gpu

N = 70001
LINE = (65535, 65536, 65537)
SMALL = 4096
SUBSET = np.unique(np.concatenate([np.arange(0, N, 257), [0, 65534, 65535, 65536, 65537, N - 1]]))


def temperatures(n):
    return np.tile(synth.temperatures(8), n // 8 + 1)[:n]


def sigma_of(n):
    return 0.05 + 0.2 * np.abs(np.sin(np.arange(n)))    # tests/test_parity_gpu.py::test_chi_square_likelihood


def device_free_bytes():
    """hipMemGetInfo of the runtime the library has loaded."""
    capi.load_library()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert C.CDLL(path).hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def report_memory(tag, before):
    used = before - device_free_bytes()
    print(f"DEVICE MEMORY {tag}: {used / 1e9:.3f} GB")
    assert used < 8e9, (tag, used)


@functools.lru_cache(maxsize=None)
def workload(name):
    """(workload, spectrum, N rows, N temperatures), never changed."""
    from oracle import pyoracle as orc
    if name == "id11":
        w = W.any_model(11, Nx=600, trunc_c=20.0)                 # tests/test_parity_gpu.py, the 4096-chain test
    elif name == "id2":
        w = W.make(2, Nx=600)
    elif name == "five-tiles":
        w = W.layout(2, 2, Nmax=3, Nx=2560)                       # 5 units, 5 tiles, 9 multiplets
    elif name == "id9":
        w = W.any_model(9, Nx=9000)                               # tests/test_group_gpu.py::mixed_members
    m, st = orc.model(w["model_case"], w["params_true"], w["plength"], w["x"])
    assert st == 0
    y = synth.make_spectrum(m, seed=17)
    P = W.perturbed(w, N, scale=0.002, seed=70001)
    if name == "id9":                                             # the NaN row and the empty-window row of mixed_members
        off = np.concatenate([[0], np.cumsum(np.asarray(w["plength"]))])
        base = np.asarray(w["params_true"], dtype=float)
        nan, empty = base.copy(), base.copy()
        nan[off[7] + 1] = base[off[7]]
        empty[off[7]] = -base[off[7]]
        P[65535], P[65536], P[N - 1], P[65534] = nan, empty, nan, empty
    T = temperatures(N)
    for a in (y, P, T):
        a.setflags(write=False)
    return w, y, P, T


def open_ctx(accel_mod, name, like=0, grad=True):
    w, y, _, _ = workload(name)
    acc = accel_mod.Accel(w["model_case"], w["plength"], w["x"], y, sigma_y=sigma_of(y.size) if like else None, likelihood_case=like)
    if grad:
        acc.set_vars(w["index_to_relax"])
    return acc


_SMALL = {}


def in_small_batches(accel_mod, name, like=0, grad=False, n=N):
    """The first n chains in batches of 4096 on a fresh context in the default configuration: (logL, status[, grad]).
    Computed once per (case, likelihood, gradient) -- call it before a developer switch is set."""
    key = (name, like, grad)
    if key not in _SMALL:
        assert not any(k in os.environ for k in ("TAMCMC_ORDER", "TAMCMC_FUSED")), "the reference is the default configuration"
        _, _, P, T = workload(name)
        with open_ctx(accel_mod, name, like, grad) as acc:
            out = [acc.eval_batch(P[k:k + SMALL], T[k:k + SMALL], grad=grad) for k in range(0, N, SMALL)]
        _SMALL[key] = tuple(np.concatenate([o[j] for o in out]) for j in range(len(out[0])))
        for a in _SMALL[key]:
            a.setflags(write=False)
    return tuple(a[:n] for a in _SMALL[key])


def assert_same(tag, big, small):
    """(logL, status[, gradient]) of two evaluations bit for bit; names the first chains that differ."""
    assert np.array_equal(big[1], small[1]), (tag, "status", np.flatnonzero(big[1] != small[1])[:8])
    for j, what in ((0, "logL"), (2, "gradient")):
        if j < len(small):
            a, b = (np.ascontiguousarray(v, dtype=np.float64).view(np.int64) for v in (big[j], small[j]))
            assert a.shape == b.shape, (tag, what, a.shape, b.shape)
            bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
            assert bad.size == 0, (tag, what, "chains", bad[:8], "of", bad.size)


def against_oracle(orc, name, res, like=0, tag="", leave_out=()):
    """The subset against the CPU oracle with the suite's bars."""
    w, y, P, T = workload(name)
    sel = SUBSET[(SUBSET < len(res[0])) & ~np.isin(SUBSET, leave_out)]
    sigma = sigma_of(y.size) if like else None
    rL, rst = orc.generate_batch(w["model_case"], w["plength"], w["x"], y, P[sel], T[sel], sigma_y=sigma, likelihood_case=like)[:2]
    assert np.array_equal(res[1][sel], rst), tag
    ok = rst == 0
    check_logL(res[0][sel][ok], rL[ok])
    if len(res) > 2:
        gradcheck.check_against_oracle(None, orc, w["model_case"], w, y, P[sel], T[sel], sigma=sigma, like=like, tag=tag, g=res[2][sel])


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "two-launches"])
@pytest.mark.parametrize("name", ["id11", "id2"])
def test_one_tile_launch(accel_mod, orc, monkeypatch, name, fused):
    _, _, P, T = workload(name)
    small = in_small_batches(accel_mod, name)
    small_g = in_small_batches(accel_mod, name, grad=True)
    small_c = in_small_batches(accel_mod, name, like=1)
    monkeypatch.setenv("TAMCMC_FUSED", fused)
    with open_ctx(accel_mod, name) as acc:
        assert acc.geometry()["tiles"] == 1
        big = acc.eval_batch(P, T)
        big_g = acc.eval_batch(P, T, grad=True)
    assert_same(f"{name} likelihood", big, small)
    assert_same(f"{name} gradient", big_g, small_g)
    against_oracle(orc, name, big)
    against_oracle(orc, name, big_g, tag=f"{name}, {N} chains")
    # chi_square, model rows of the chains around the line
    w, y, _, _ = workload(name)
    want = [0, 65535, 65536, N - 1]
    with open_ctx(accel_mod, name, like=1, grad=False) as acc:
        L, st, rows = acc.eval_batch(P, T, model_rows=want)
        for j, k in enumerate(want):
            _, _, one = acc.eval_batch(P[k:k + 1], T[k:k + 1], model_rows=[0])
            assert bits_equal(rows[j], one[0]), (name, "model row of chain", k)
    assert_same(f"{name} chi_square", (L, st), small_c)
    against_oracle(orc, name, (L, st), like=1)
    rm = orc.generate_batch(w["model_case"], w["plength"], w["x"], y, P[want], T[want], sigma_y=sigma_of(y.size), likelihood_case=1,
                            want_models=True)[2]
    assert np.max(np.abs(rows - rm) / rm) <= RTOL_MODEL


@pytest.mark.parametrize("order", [None, "1", "0"], ids=["default", "order-1", "order-0"])     # the default mode first
def test_tiled_launch(accel_mod, orc, monkeypatch, order):
    """5 tiles per chain.  TAMCMC_ORDER=0 is the chain-major order: grid = (tiles, chains), the rotation masks the chain."""
    _, _, P, T = workload("five-tiles")
    small = in_small_batches(accel_mod, "five-tiles")
    small_g = in_small_batches(accel_mod, "five-tiles", grad=True)
    if order is not None:
        monkeypatch.setenv("TAMCMC_ORDER", order)
    before = device_free_bytes()
    with open_ctx(accel_mod, "five-tiles") as acc:
        assert acc.geometry()["tiles"] == 5 and acc.geometry()["n_multiplets"] == 9
        big = acc.eval_batch(P, T)
        big_g = acc.eval_batch(P, T, grad=True)
        report_memory(f"5 tiles, {N} chains, gradient, order {order}", before)
        again = acc.eval_batch(P[:7], T[:7])                       # the context after the large batch
    assert_same(f"order {order} likelihood", big, small)
    assert_same(f"order {order} gradient", big_g, small_g)
    assert bits_equal(again[0], small[0][:7])
    against_oracle(orc, "five-tiles", big)
    against_oracle(orc, "five-tiles", big_g, tag=f"5 tiles, {N} chains, order {order}")


def test_rejected_chains_at_the_line(accel_mod, orc):
    """Id 9 on 9000 bins: a NaN chain at 65 535 and N - 1, an empty truncation window at 65 534 and 65 536.  The NaN row is
    the width that overflows (tests/test_special_values_gpu.py, the documented exception): status 1 here, where the
    oracle's formula stays finite and loses the move by more than 1e3 in logL -- asserted as there."""
    _, _, P, T = workload("id9")
    small = in_small_batches(accel_mod, "id9")
    before = device_free_bytes()
    with open_ctx(accel_mod, "id9", grad=False) as acc:
        assert acc.geometry()["tiles"] > 1
        big = acc.eval_batch(P, T)
        report_memory(f"id 9, 9000 bins, {N} chains", before)
    assert_same("id 9", big, small)
    st = big[1]
    assert st[65535] == capi.CHAIN_NAN and st[N - 1] == capi.CHAIN_NAN and st[65534] == capi.CHAIN_EMPTY_WINDOW and st[65536] == capi.CHAIN_EMPTY_WINDOW
    assert st[65537] == 0 and st[0] == 0 and np.all(np.isnan(big[0][st != 0])) and np.all(np.isfinite(big[0][st == 0]))
    against_oracle(orc, "id9", big, leave_out=(65535, N - 1))
    w, y, _, _ = workload("id9")
    k = np.array([0, 65535, N - 1])
    rL, rst = orc.generate_batch(9, w["plength"], w["x"], y, P[k], T[k])[:2]
    assert np.all(rst == 0) and np.all(rL[1:] * T[k[1:]] < rL[0] * T[0] - 1e3)


@pytest.mark.parametrize("name", ["id11", "five-tiles"])
def test_host_paths(accel_mod, name):
    """begin / end and arm / fire / end watch 65 537 result slots arrive (tm_wait_slots)."""
    n = 65537
    _, _, P, T = workload(name)
    small = in_small_batches(accel_mod, name, n=n)
    with open_ctx(accel_mod, name, grad=False) as acc:
        ref = acc.eval_batch(P[:n], T[:n])
        assert_same("eval_batch", ref, small)
        acc.begin(P[:n], T[:n])
        assert_same("begin / end", acc.end(), ref)
        acc.arm(n)
        acc.fire(P[:n], T[:n])
        assert_same("arm / fire / end", acc.end(), ref)
        for m in LINE:                                             # smaller batches on the grown buffers, across the line
            acc.begin(P[:m], T[:m])
            assert_same(f"begin / end {m}", acc.end(), tuple(a[:m] for a in ref))


def _device_check():
    """Body of test_device_pointers, in a process where torch owns the device first (as bench.py)."""
    import torch
    import tamcmc_amd as accel_mod
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    w, _, P, T = workload("five-tiles")
    nv = len(w["index_to_relax"])
    with open_ctx(accel_mod, "five-tiles") as acc:
        host = acc.eval_batch(P, T)
        host_g = acc.eval_batch(P, T, grad=True)
        acc.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dP = torch.from_numpy(np.ascontiguousarray(P)).to(dev)
        dT = torch.from_numpy(np.ascontiguousarray(T)).to(dev)
        dL = torch.full((N,), 7.0, dtype=torch.float64, device=dev)
        dG = torch.full((N, nv), 7.0, dtype=torch.float64, device=dev)
        dS = torch.full((N,), -9, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()                                   # (the stream handed in may be the null stream = the context's own)
        acc.eval_batch_device(N, dP.data_ptr(), dT.data_ptr(), dL.data_ptr(), 0, dS.data_ptr())
        acc.synchronize()
        assert_same("device likelihood", (dL.cpu().numpy(), dS.cpu().numpy()), host)
        dL.fill_(3.0)
        dS.fill_(-9)
        torch.cuda.synchronize()
        acc.eval_batch_device(N, dP.data_ptr(), dT.data_ptr(), dL.data_ptr(), dG.data_ptr(), dS.data_ptr())
        acc.synchronize()
        assert_same("device gradient", (dL.cpu().numpy(), dS.cpu().numpy(), dG.cpu().numpy()), host_g)
        acc.set_stream(0)
    print("chain counts device path ok")


def test_device_pointers():
    in_torch_process("test_chain_counts_gpu", "_device_check", "chain counts device path ok")


@pytest.mark.parametrize("order", [None, "0"], ids=["default", "order-0"])
def test_group_with_a_long_member(accel_mod, monkeypatch, order):
    """65 537 chains of the 5-tile context beside the one-tile, id 1 and chi_square members of mixed_members: the group
    kernel recovers (chain, tile) of the long member from a linear workgroup id."""
    n = 65537
    _, _, P, T = workload("five-tiles")
    small = in_small_batches(accel_mod, "five-tiles", n=n)
    if order is not None:
        monkeypatch.setenv("TAMCMC_ORDER", order)
    everyone = mixed_members(accel_mod)
    names = ("one-tile", "id1", "chi2")
    mem = [m for m in everyone if m[0] in names]
    close_all([m for m in everyone if m[0] not in names])
    mem.insert(1, ("five-tiles", open_ctx(accel_mod, "five-tiles", grad=False), P[:n], T[:n]))
    accels = [m[1] for m in mem]
    with accel_mod.Group(accels) as g:
        L, st = assert_group_matches_solo(g, accels, [m[2] for m in mem], [m[3] for m in mem])
    assert_same("the long member in the group", (L[1], st[1]), small)
    close_all(mem)


def test_group_of_67_small_contexts(accel_mod):
    from oracle import pyoracle as orc
    kinds = ("fused-id11", "tiled-id2", "tiled-id1", "fused-id1", "tiled-chi2")
    rng, counts = np.random.default_rng(67), np.random.default_rng(670)
    mem = []
    for k in range(67):
        kind = kinds[k % len(kinds)]
        fused = kind.startswith("fused")
        Nx = int(rng.integers(600, 2049)) if fused else int(rng.integers(2049, 3001))
        mid = {"fused-id11": 11, "tiled-id2": 2, "tiled-id1": 1, "fused-id1": 1, "tiled-chi2": 2}[kind]
        w = W.any_model(mid, Nx=Nx)
        m, st = orc.model(mid, w["params_true"], w["plength"], w["x"])
        assert st == 0
        y = synth.make_spectrum(m, seed=100 + k)
        chi2 = kind == "tiled-chi2"
        acc = accel_mod.Accel(mid, w["plength"], w["x"], y, sigma_y=0.1 + 0.05 * np.abs(y) if chi2 else None, likelihood_case=int(chi2))
        assert (acc.geometry()["tiles"] == 1) == fused, (kind, Nx)
        mem.append((kind, acc, W.perturbed(w, 6, scale=0.003, seed=200 + k), np.linspace(1.0, 2.5, 6)))
    count = {kind: sum(m[0] == kind for m in mem) for kind in kinds}
    # the four tables of a call: setup (every tiled member), fused, specialised eval, generic eval
    assert min(count["tiled-id2"], count["tiled-id1"] + count["tiled-chi2"], count["fused-id11"] + count["fused-id1"]) >= 9
    accels = [m[1] for m in mem]
    with accel_mod.Group(accels) as g:
        for call in range(4):
            nc = counts.integers(0, 7, size=len(mem))
            assert np.any(nc == 0) and np.any(nc == 1) and nc.sum() > 0
            assert_group_matches_solo(g, accels, [m[2][:c] for m, c in zip(mem, nc)], [m[3][:c] for m, c in zip(mem, nc)])
    close_all(mem)


def test_a_batch_no_launch_can_take_is_refused(accel_mod, monkeypatch):
    """tamcmc_accel.h, next to tamcmc_eval_batch: workgroups x threads of every launch within 2^32 - 1, refused with
    TAMCMC_E_INVALID before anything is sized or read (the pointers below cover 3 chains), the context usable afterwards."""
    def refused(acc, n, P, T):
        L, st = np.zeros(3), np.zeros(3, dtype=np.int32)
        rc = acc._lib.tamcmc_eval_batch(acc._ctx, n, acc.Nparams, capi._dptr(P), capi._dptr(T), capi._dptr(L), None, 0, None, None,
                                        capi._iptr(st))
        assert rc == capi.E_INVALID, (n, rc)
        assert acc._lib.tamcmc_ctx_reserve(acc._ctx, n) == capi.E_INVALID
        assert acc._lib.tamcmc_eval_batch_arm(acc._ctx, n) == capi.E_INVALID

    for name, env, first_refused in (("id11", {}, 16777216), ("id11", {"TAMCMC_FUSED": "0"}, 8388608), ("five-tiles", {}, 3355444)):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _, _, P, T = workload(name)
        P3, T3 = np.ascontiguousarray(P[:3]), np.ascontiguousarray(T[:3])
        with open_ctx(accel_mod, name, grad=False) as acc:
            before = acc.eval_batch(P3, T3)
            refused(acc, first_refused, P3, T3)
            refused(acc, 2 ** 31 - 1, P3, T3)
            after = acc.eval_batch(P3, T3)
            assert_same("after a refusal", after, before)
        for k in env:
            monkeypatch.delenv(k)
