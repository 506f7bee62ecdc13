"""Fit groups (tamcmc_group_*, tamcmc_amd.Group): the likelihood batches of several contexts -- different grids, model
ids, likelihoods, layouts -- in one call.  The grouped kernels run the same bodies with the same tile geometry as a
context alone, so the oracle is exact: every chain's logL and status must equal its member's own eval_batch bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import workloads as W
from support import in_torch_process
from tamcmc_amd import capi, synth
from tamcmc_amd.setup_io import Setup, model_file_slices

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_inputs")
CFG = os.path.join(G, "Config_default")
TF_MODEL = os.path.join(G, "TF_3443483_local-v3.model")
TF_DATA = os.path.join(G, "TF_3443483_local-v3.data")


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def chains_around(s, n, seed=3, scale=0.3):
    rng = np.random.default_rng(seed)
    P = np.tile(s.inputs, (n, 1))
    P[1:, s.index_to_relax] += scale * s.err * rng.standard_normal((n - 1, s.Nvars))
    return P


def slices():
    out = []
    for k in range(len(model_file_slices(TF_MODEL))):
        s = Setup(CFG).load(TF_MODEL, TF_DATA, k)
        out.append((s, chains_around(s, 10, seed=10 + k), 1.7 ** np.arange(10)))
    return out


def slice_accel(accel_mod, s):
    return accel_mod.Accel(s.model_case, s.plength, s.x, s.y, likelihood_case=s.likelihood_case,
                           likelihood_p=s.likelihood_p)


def assert_group_matches_solo(group, accels, P_list, T_list):
    L, st = group.eval(P_list, T_list)
    for k, (acc, P, T) in enumerate(zip(accels, P_list, T_list)):
        assert L[k].shape == (len(P),) and st[k].shape == (len(P),)
        if len(P) == 0:
            continue
        rL, rst = acc.eval_batch(P, T)
        assert np.array_equal(st[k], rst), (k, st[k], rst)
        assert bits_equal(L[k], rL), (k, L[k], rL)
    return L, st


def test_local_fit_slices_in_one_group(accel_mod, orc):
    sl = slices()
    assert len(sl) == 8
    accels = [slice_accel(accel_mod, s) for s, _, _ in sl]
    with accel_mod.Group(accels) as g:
        L, st = assert_group_matches_solo(g, accels, [p for _, p, _ in sl], [t for _, _, t in sl])
    for (s, P, T), l, t in zip(sl, L, st):
        ref, rst = orc.generate_batch(s.model_case, s.plength, s.x, s.y, P, T, likelihood_p=s.likelihood_p)[:2]
        assert np.array_equal(t, rst) and np.all(t == 0)
        assert np.allclose(l, ref, rtol=1e-10, atol=0)
    for a in accels:
        a.close()


def _spectrum(mid, w, seed):
    from oracle import pyoracle as orc
    m, st = orc.model(mid, w["params_true"], w["plength"], w["x"])
    assert st == 0
    return synth.make_spectrum(m, seed=seed)


def mixed_members(accel_mod):
    """(name, Accel, P, T) of members that take every path of a group call."""
    out = []
    w = synth.workload_c2(Nx=100000)                                        # id 2, 196 units: 25 tiles
    acc = accel_mod.Accel(2, w["plength"], w["x"], _spectrum(2, w, 1))
    assert acc.geometry()["tiles"] == 25
    out.append(("id2-1e5", acc, synth.chain_params(w, 12), synth.temperatures(12)))
    w = W.make(3, Nx=30000)                                                  # id 3, another grid
    out.append(("id3", accel_mod.Accel(3, w["plength"], w["x"], _spectrum(3, w, 2)), W.perturbed(w, 5, seed=5),
                np.linspace(1.0, 4.0, 5)))
    w = W.any_model(9, Nx=9000)                                              # AppWidth: a NaN chain and an empty window
    pl = np.asarray(w["plength"])
    off = np.concatenate([[0], np.cumsum(pl)])
    base = np.asarray(w["params_true"], dtype=float)
    P = np.tile(base, (4, 1))
    P[1, off[7] + 1] = base[off[7]]        # exponent := nu_dip: the width overflows -> status 1
    P[2, off[7]] = -base[off[7]]           # negative width -> empty truncation window, status 2
    P[3] = W.perturbed(w, 2, seed=9)[1]
    out.append(("id9-special", accel_mod.Accel(9, w["plength"], w["x"], _spectrum(9, w, 3)), P, np.array([1.0, 1.5, 2.0, 2.5])))
    w = W.any_model(14, Nx=3000)                                             # local, id 14
    out.append(("id14", accel_mod.Accel(14, w["plength"], w["x"], _spectrum(14, w, 4)), W.perturbed(w, 6, seed=6),
                np.linspace(1.0, 2.0, 6)))
    w = W.make(2, Nx=8000)                                                   # chi_square: the generic launch
    y = _spectrum(2, w, 5)
    out.append(("chi2", accel_mod.Accel(2, w["plength"], w["x"], y, sigma_y=0.1 + 0.05 * np.abs(y), likelihood_case=1),
                W.perturbed(w, 5, seed=7), np.linspace(1.0, 3.0, 5)))
    w = W.any_model(1, Nx=4096)                                              # id 1 (Gaussian term): the generic launch
    out.append(("id1", accel_mod.Accel(1, w["plength"], w["x"], _spectrum(1, w, 6)), W.perturbed(w, 3, seed=8),
                np.array([1.0, 1.3, 1.9])))
    w = synth.workload_c2(Nx=20000)                                          # 3 spectra on one grid, a chain map
    acc = accel_mod.Accel(2, w["plength"], w["x"], _spectrum(2, w, 7))
    acc.set_spectra(np.stack([_spectrum(2, w, 70 + j) for j in range(3)]))
    acc.set_chain_spectrum([2, 0, 1, 1, 2, 0, 2])
    out.append(("3-spectra", acc, synth.chain_params(w, 7), synth.temperatures(7)))
    w = W.any_model(11, Nx=2000)                                             # one tile: the fused launch; 1 chain
    acc = accel_mod.Accel(11, w["plength"], w["x"], _spectrum(11, w, 8))
    assert acc.geometry()["tiles"] == 1
    out.append(("one-tile", acc, W.perturbed(w, 1, seed=10), np.array([1.0])))
    w = W.any_model(12, Nx=5000)                                             # sits the call out
    out.append(("idle", accel_mod.Accel(12, w["plength"], w["x"], _spectrum(12, w, 9)), np.empty((0, int(np.sum(w["plength"])))),
                np.empty(0)))
    return out


def close_all(members):
    for m in members:
        m[1].close()


# the developer switches that change a member's launch geometry, order or path (tamcmc_accel.h), read at create
SWITCHES = [{}, {"TAMCMC_ORDER": "0"}, {"TAMCMC_ORDER": "1"}, {"TAMCMC_PRIO": "1"}, {"TAMCMC_EQUAL_COST": "1"},
            {"TAMCMC_FUSED": "0"}]


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_mixed_group_matches_every_member_alone(accel_mod, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mem = mixed_members(accel_mod)
    accels = [m[1] for m in mem]
    with accel_mod.Group(accels) as g:
        L, st = assert_group_matches_solo(g, accels, [m[2] for m in mem], [m[3] for m in mem])
    k = [m[0] for m in mem].index("id9-special")
    assert st[k][1] == capi.CHAIN_NAN and st[k][2] == capi.CHAIN_EMPTY_WINDOW and st[k][0] == 0
    assert len(L[[m[0] for m in mem].index("idle")]) == 0
    close_all(mem)


def _device_check():
    """Body of test_device_entry_point_equals_host_path, in a process where torch owns the device first (as bench.py)."""
    import torch
    import tamcmc_amd as accel_mod
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    mem = mixed_members(accel_mod)
    accels = [m[1] for m in mem]
    P_list, T_list = [m[2] for m in mem], [m[3] for m in mem]
    n = np.array([len(p) for p in P_list], dtype=np.int32)
    with accel_mod.Group(accels) as g:
        L, st = g.eval(P_list, T_list)
        dP = torch.from_numpy(np.concatenate([p.ravel() for p in P_list])).to(dev)
        dT = torch.from_numpy(np.concatenate(T_list)).to(dev)
        dL = torch.full((int(n.sum()),), 7.0, dtype=torch.float64, device=dev)
        dS = torch.full((int(n.sum()),), -9, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        g.eval_device(n, dP.data_ptr(), dT.data_ptr(), dL.data_ptr(), dS.data_ptr())
        g.synchronize()
        assert bits_equal(dL.cpu().numpy(), np.concatenate(L))
        assert np.array_equal(dS.cpu().numpy(), np.concatenate(st))
        # again on the torch stream: the table of the first call is replaced in stream order
        g.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dL.fill_(3.0)
        g.eval_device(n, dP.data_ptr(), dT.data_ptr(), dL.data_ptr(), 0)
        assert bits_equal(dL.cpu().numpy(), np.concatenate(L))
    close_all(mem)
    print("device path ok")


def test_device_entry_point_equals_host_path():
    in_torch_process("test_group_gpu", "_device_check", "device path ok")


def _stream_order_check():
    """Solo and group device calls on the same members, each on its own stream, enqueued back to back without any
    synchronisation: solo(A) on the members' streams, group(B) on the group's stream, solo(C) on the members' streams.
    All three share each member's per-chain buffers, so only the event ordering keeps them apart."""
    import torch
    import tamcmc_amd as accel_mod
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    mem = [m for m in mixed_members(accel_mod) if len(m[2]) > 0]
    accels = [m[1] for m in mem]
    n = np.array([len(m[2]) for m in mem], dtype=np.int32)
    rng = np.random.default_rng(12)
    sets = []
    for j in range(3):
        P_list = [m[2] if j == 1 else m[2] * (1.0 + 1e-4 * rng.standard_normal(m[2].shape)) for m in mem]
        T_list = [m[3] for m in mem]
        if j != 1:      # a long solo batch on the 25-tile member (~0.5 ms), so that an unordered group launch would overlap it
            P_list[0] = mem[0][2][np.arange(480) % len(mem[0][2])] * (1.0 + 1e-4 * rng.standard_normal((480, mem[0][2].shape[1])))
            T_list = [synth.temperatures(480)] + T_list[1:]
        sets.append((P_list, T_list))
    ref = []
    for P_list, T_list in sets:
        ref.append([acc.eval_batch(P, T) for acc, P, T in zip(accels, P_list, T_list)])
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with accel_mod.Group(accels) as g:
        solo_bufs = []
        for j in (0, 2):
            P_list, T_list = sets[j]
            solo_bufs.append([(put(P), put(T), torch.full((len(P),), 5.0, dtype=torch.float64, device=dev),
                               torch.full((len(P),), -7, dtype=torch.int32, device=dev)) for P, T in zip(P_list, T_list)])
        gP = put(np.concatenate([P.ravel() for P in sets[1][0]]))
        gT = put(np.concatenate(sets[1][1]))
        gL = torch.full((int(n.sum()),), 5.0, dtype=torch.float64, device=dev)
        gS = torch.full((int(n.sum()),), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for acc, (dP, dT, dL, dS) in zip(accels, solo_bufs[0]):
            acc.eval_batch_device(len(dT), dP.data_ptr(), dT.data_ptr(), dL.data_ptr(), 0, dS.data_ptr())
        g.eval_device(n, gP.data_ptr(), gT.data_ptr(), gL.data_ptr(), gS.data_ptr())
        for acc, (dP, dT, dL, dS) in zip(accels, solo_bufs[1]):
            acc.eval_batch_device(len(dT), dP.data_ptr(), dT.data_ptr(), dL.data_ptr(), 0, dS.data_ptr())
        for acc in accels:
            acc.synchronize()
        g.synchronize()
        for k in range(len(mem)):
            for bufs, j in ((solo_bufs[0], 0), (solo_bufs[1], 2)):
                assert bits_equal(bufs[k][2].cpu().numpy(), ref[j][k][0]), (mem[k][0], j)
                assert np.array_equal(bufs[k][3].cpu().numpy(), ref[j][k][1]), (mem[k][0], j)
        cut = np.cumsum(n)[:-1]
        for k, (l, st) in enumerate(zip(np.split(gL.cpu().numpy(), cut), np.split(gS.cpu().numpy(), cut))):
            assert bits_equal(l, ref[1][k][0]) and np.array_equal(st, ref[1][k][1]), mem[k][0]
    close_all(mem)
    print("stream order ok")


def test_solo_and_group_device_calls_need_no_synchronisation():
    in_torch_process("test_group_gpu", "_stream_order_check", "stream order ok")


def test_solo_and_group_calls_alternate(accel_mod):
    mem = mixed_members(accel_mod)
    accels = [m[1] for m in mem]
    rng = np.random.default_rng(4)
    with accel_mod.Group(accels) as g:
        for it in range(4):
            # a different Nchains vector every call (0 .. all rows of each member; the map of the 3-spectrum member
            # covers its first 7 chains)
            P_list, T_list = [], []
            for name, acc, P, T in mem:
                n = int(rng.integers(0, len(P) + 1))
                if it == 3:
                    n = len(P)
                P_list.append(P[:n]); T_list.append(T[:n])
            if sum(len(p) for p in P_list) == 0:
                P_list[0], T_list[0] = mem[0][2][:1], mem[0][3][:1]
            solo = [acc.eval_batch(P, T) if len(P) else None for (_, acc, _, _), P, T in zip(mem, P_list, T_list)]
            L, st = g.eval(P_list, T_list)
            again = [acc.eval_batch(P, T) if len(P) else None for (_, acc, _, _), P, T in zip(mem, P_list, T_list)]
            for k in range(len(mem)):
                if solo[k] is None:
                    assert len(L[k]) == 0
                    continue
                assert bits_equal(L[k], solo[k][0]) and np.array_equal(st[k], solo[k][1]), (it, mem[k][0])
                assert bits_equal(again[k][0], solo[k][0]), (it, mem[k][0])
    close_all(mem)


def test_refusals(accel_mod):
    lib = capi.load_library()
    w = synth.workload_c2(Nx=100000)
    a = accel_mod.Accel(2, w["plength"], w["x"], _spectrum(2, w, 1))
    w2 = W.any_model(11, Nx=2000)
    b = accel_mod.Accel(11, w2["plength"], w2["x"], _spectrum(11, w2, 8))
    P, T = synth.chain_params(w, 4), synth.temperatures(4)
    Pb, Tb = W.perturbed(w2, 2), np.array([1.0, 2.0])
    # creation: empty, NULL member, the same ctx twice, too many members
    with pytest.raises(capi.AccelError) as e:
        accel_mod.Group([])
    assert e.value.code == capi.E_INVALID
    g = C.c_void_p()
    arr = (C.c_void_p * 2)(a._ctx.value, None)
    assert lib.tamcmc_group_create(C.byref(g), 2, arr) == capi.E_INVALID and not g.value
    with pytest.raises(capi.AccelError) as e:
        accel_mod.Group([a, b, a])
    assert e.value.code == capi.E_INVALID
    big = (C.c_void_p * 1025)(*([a._ctx.value] * 1025))
    assert lib.tamcmc_group_create(C.byref(g), 1025, big) == capi.E_INVALID
    if capi.device_count() >= 2:
        c1 = accel_mod.Accel(2, w["plength"], w["x"], _spectrum(2, w, 1), device_id=1)
        with pytest.raises(capi.AccelError):
            accel_mod.Group([a, c1])
        c1.close()
    grp = accel_mod.Group([a, b])
    n = np.array([4, 2], dtype=np.int32)

    def call(nch, npar=None):
        nch = np.ascontiguousarray(nch, dtype=np.int32)
        npar = np.ascontiguousarray(grp.Nparams if npar is None else npar, dtype=np.int32)
        Pc = np.concatenate([P.ravel(), Pb.ravel()])
        Tc = np.concatenate([T, Tb])
        out = np.empty(6)
        stt = np.empty(6, dtype=np.int32)
        return lib.tamcmc_group_eval(grp._g, capi._iptr(nch), capi._iptr(npar), capi._dptr(Pc), capi._dptr(Tc),
                                     capi._dptr(out), capi._iptr(stt))

    assert call(n) == capi.OK
    assert call([0, 0]) == capi.E_INVALID                               # nothing to do
    assert call([4, -1]) == capi.E_INVALID
    assert call(n, [grp.Nparams[0], grp.Nparams[1] + 1]) == capi.E_INVALID
    # a 1-D grid beyond 2^32 work-items (25 tiles x 700 000 chains): refused before anything is allocated
    huge = np.array([700000, 0], dtype=np.int32)
    assert lib.tamcmc_group_eval_device(grp._g, capi._iptr(huge), capi._iptr(grp.Nparams), C.c_void_p(8), C.c_void_p(8),
                                        C.c_void_p(8), None) == capi.E_INVALID
    # a member with a batch in flight, or armed
    a.begin(P, T)
    assert call(n) == capi.E_INVALID
    a.end()
    a.reserve(4)
    a.arm(4)
    assert call(n) == capi.E_INVALID
    a.disarm()
    assert call(n) == capi.OK
    # a multi-spectrum member whose map does not cover its batch
    a.set_spectra(np.stack([a.y, a.y]))
    assert call(n) == capi.E_INVALID
    a.set_chain_spectrum([0, 1, 1])
    assert call(n) == capi.E_INVALID
    a.set_chain_spectrum([0, 1, 1, 0])
    assert call(n) == capi.OK
    # destroy order: a grouped member is kept, the group still works; after the group, the member goes
    with pytest.raises(capi.AccelError) as e:
        a.close()
    assert e.value.code == capi.E_INVALID and a._ctx.value
    L, st = grp.eval([P, Pb], [T, Tb])
    rL, rst = a.eval_batch(P, T)
    assert bits_equal(L[0], rL) and np.array_equal(st[0], rst)
    grp.close()
    a.close()
    b.close()
    assert not a._ctx.value
